"""UPerNet (architecture='UPerNet') without a GPU: the functional reference against an independent torch.nn UPerNet, parameter names, shapes
and counts, the constructor, the refusals, checkpoints and the argument checks of the new native entry points."""
import ctypes
import math
import warnings

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import upernet_ref as ref


def _model(**kw):
    from interactive_unet.unet import UNet
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return UNet(architecture='UPerNet', pretrained=False, **kw)


# ---- an independent torch.nn UPerNet (pyramid pooling module + FPN top-down path + fused head on the project's encoder)
class Stage(nn.Module):
    def __init__(self, ci, co, dim):
        super().__init__()
        Conv, BN = (nn.Conv3d, nn.BatchNorm3d) if dim == 3 else (nn.Conv2d, nn.BatchNorm2d)
        self.conv1, self.bn1 = Conv(ci, co, 3, padding=1, bias=False), BN(co)
        self.conv2, self.bn2 = Conv(co, co, 3, padding=1, bias=False), BN(co)

    def forward(self, x):
        return torch.relu(self.bn2(self.conv2(torch.relu(self.bn1(self.conv1(x))))))


class ConvBnRelu(nn.Sequential):
    def __init__(self, ci, co, k, dim, norm=True):
        super().__init__()
        Conv, BN = (nn.Conv3d, nn.BatchNorm3d) if dim == 3 else (nn.Conv2d, nn.BatchNorm2d)
        self.add_module('conv', Conv(ci, co, k, padding=k // 2, bias=not norm))
        if norm:
            self.add_module('bn', BN(co))
        self.add_module('relu', nn.ReLU())


class TorchUPerNet(nn.Module):
    def __init__(self, dim=2, levels=4, base=32, cin=1, ncls=2, C=256):
        super().__init__()
        ch = [base * 2 ** l for l in range(levels)]
        self.dim, self.levels = dim, levels
        self.enc = nn.ModuleList(Stage(cin if l == 0 else ch[l - 1], ch[l], dim) for l in range(levels))
        self.psp = nn.ModuleDict({f'b{s}': ConvBnRelu(ch[-1], ch[-1] // 4, 1, dim, norm=s > 1) for s in (1, 2, 3, 6)})
        self.psp['out'] = ConvBnRelu(2 * ch[-1], C, 3, dim)
        self.lat = nn.ModuleDict({str(l): ConvBnRelu(ch[l], C, 1, dim) for l in range(levels - 2, 1, -1)})
        self.fuse = ConvBnRelu((levels - 2) * C, C, 3, dim)
        self.head = (nn.Conv3d if dim == 3 else nn.Conv2d)(C, ncls, 1)

    def named_canonical(self):
        out = {}
        for k, v in self.state_dict().items():
            if k.endswith('num_batches_tracked'):
                continue
            parts = k.split('.')
            if parts[0] in ('enc', 'lat'):
                k = f'{parts[0]}{parts[1]}.' + '.'.join(parts[2:])
            out[k] = v
        return out

    def load_canonical(self, p):
        keys = [k for k in self.state_dict() if not k.endswith('num_batches_tracked')]
        self.load_state_dict({key: p[k] for k, key in zip(self.named_canonical(), keys)}, strict=False)

    def forward(self, x):
        up = lambda t, size: F.interpolate(t, size=size, mode='trilinear' if self.dim == 3 else 'bilinear', align_corners=False)
        pool = nn.AdaptiveAvgPool3d if self.dim == 3 else nn.AdaptiveAvgPool2d
        feats, h = [], x
        for l, st in enumerate(self.enc):
            if l > 0:
                h = (F.max_pool3d if self.dim == 3 else F.max_pool2d)(h, 2)
            h = st(h)
            feats.append(h)
        B = self.levels - 1
        X = feats[B]
        U = torch.cat([X] + [up(self.psp[f'b{s}'](pool(s)(X)), X.shape[2:]) for s in (1, 2, 3, 6)], 1)
        P = {B: self.psp['out'](U)}
        for l in range(B - 1, 1, -1):
            P[l] = up(P[l + 1], feats[l].shape[2:]) + self.lat[str(l)](feats[l])
        T = feats[2].shape[2:]
        V = torch.cat([up(P[l], T) for l in range(B, 2, -1)] + [P[2]], 1)
        lc = self.head(self.fuse(V))
        return F.interpolate(lc, scale_factor=4, mode='trilinear' if self.dim == 3 else 'bilinear', align_corners=True)


def _recount(dim, L, base, cin, ncls, C):
    """The parameter count from the issue's definition, written out."""
    ch = [base * 2 ** l for l in range(L)]
    k = 3 ** dim
    n = 0
    for l in range(L):
        ci = cin if l == 0 else ch[l - 1]
        n += ci * ch[l] * k + 2 * ch[l] + ch[l] * ch[l] * k + 2 * ch[l]
    Cb, Cq = ch[-1], ch[-1] // 4
    n += Cb * Cq + Cq                                   # psp.b1: weight + bias, no norm
    n += 3 * (Cb * Cq + 2 * Cq)                         # psp.b2 / b3 / b6
    n += 2 * Cb * C * k + 2 * C                         # psp.out
    n += sum(ch[l] * C + 2 * C for l in range(2, L - 1))
    n += (L - 2) * C * C * k + 2 * C                    # fuse
    return n + C * ncls + ncls


def test_param_names_shapes_and_counts():
    from interactive_unet import unet
    for dim, count in ((2, 3632738), (3, 10692770)):
        mod = TorchUPerNet(dim=dim)
        want = {k: tuple(v.shape) for k, v in mod.named_canonical().items()}
        shapes = unet.param_shapes(dim, 4, 32, 1, 2, architecture='UPerNet')
        assert set(shapes) == set(want) and all(shapes[k] == want[k] for k in want)
        assert list(shapes) == list(ref.param_shapes(dim, 4, 32, 1, 2))
        n = sum(torch.Size(v).numel() for k, v in shapes.items() if not unet._is_buffer(k))
        assert n == sum(p.numel() for p in mod.parameters()) == _recount(dim, 4, 32, 1, 2, 256) == count
    m = unet.param_shapes(2, 6, 64, 2, 5, architecture='UPerNet', decoder_channels=96)
    assert list(m) == list(ref.param_shapes(2, 6, 64, 2, 5, 96)) and m == ref.param_shapes(2, 6, 64, 2, 5, 96)
    assert m['psp.b1.conv.weight'] == (512, 2048, 1, 1) and m['psp.b1.conv.bias'] == (512,) and 'psp.b1.bn.weight' not in m
    assert m['psp.out.conv.weight'] == (96, 4096, 3, 3) and m['lat4.conv.weight'] == (96, 1024, 1, 1) and m['lat2.conv.weight'] == (96, 256, 1, 1)
    assert m['fuse.conv.weight'] == (96, 384, 3, 3) and m['head.weight'] == (5, 96, 1, 1)
    assert 'lat5.conv.weight' not in m and 'lat1.conv.weight' not in m
    order = ['enc5.bn2.running_var', 'psp.b1.conv.weight', 'psp.b2.conv.weight', 'psp.b3.conv.weight', 'psp.b6.conv.weight', 'psp.out.conv.weight',
             'lat4.conv.weight', 'lat3.conv.weight', 'lat2.conv.weight', 'fuse.conv.weight', 'head.weight']
    names = list(m)
    assert [names.index(k) for k in order] == sorted(names.index(k) for k in order)


@pytest.mark.parametrize('dim,shape,levels', [(2, (2, 1, 48, 80), 4), (3, (2, 2, 16, 8, 24), 4), (2, (1, 3, 64, 96), 6)])
def test_reference_equals_torch_module(dim, shape, levels):
    cin = shape[1]
    mod = TorchUPerNet(dim=dim, levels=levels, base=32, cin=cin, ncls=3, C=64).double()
    p = ref.init_params(dim, levels, 32, cin, 3, 64, seed=2, randomize_bn=True)
    assert p['psp.b1.conv.bias'].abs().max() > 0
    mod.load_canonical({k: v.double() for k, v in p.items()})
    x = torch.rand(shape, dtype=torch.float64)
    mod.eval()
    with torch.no_grad():
        want = mod(x)
    got = ref.forward_logits(p, x, dim=dim, levels=levels)
    assert (got - want).abs().max().item() <= 1e-10
    mod.train()
    stats = {}
    with torch.no_grad():
        want = mod(x)
    got = ref.forward_logits(p, x, dim=dim, levels=levels, training=True, stats=stats)
    assert (got - want).abs().max().item() <= 1e-10
    for bn, m in (('fuse.bn', mod.fuse.bn), ('psp.b2.bn', mod.psp['b2'].bn), ('lat2.bn', mod.lat['2'].bn)):
        mean, var = stats[bn]
        assert torch.allclose(m.running_mean, 0.9 * p[bn + '.running_mean'].double() + 0.1 * mean)
        assert torch.allclose(m.running_var, 0.9 * p[bn + '.running_var'].double() + 0.1 * var)


def test_batch_one_trains_in_the_reference():
    """psp.b1 has no norm, so one sample is a legal training batch (every BatchNorm sees 4 or more values per channel)."""
    p = ref.init_params(2, 4, 32, 1, 2, 32, seed=1)
    y = ref.forward_logits(p, torch.rand((1, 1, 32, 32), dtype=torch.float64), 2, 4, training=True)
    assert y.shape == (1, 2, 32, 32) and bool(torch.isfinite(y).all())


def test_rounded_reference_stays_close():
    p = ref.init_params(2, 4, 32, 1, 3, 64, seed=3, randomize_bn=True)
    x = torch.rand((1, 1, 40, 24), dtype=torch.float64)
    base = torch.softmax(ref.forward_logits(p, x, 2, 4), 1)
    for T, gate in ((torch.float16, 5e-3), (torch.bfloat16, 3e-2)):
        assert (torch.softmax(ref.forward_logits(p, x, 2, 4, act=T), 1) - base).abs().max().item() <= gate


def test_constructor_hparams_and_init():
    m = _model(num_classes=3)
    assert m.architecture == 'UPerNet' and m.act_dtype == torch.float16 and m.infer_dtype == torch.float32
    assert m.hparams['decoder_channels'] == 256 and m.decoder_channels == 256
    assert 'decoder_segmentation_channels' not in m.hparams and 'decoder_atrous_rates' not in m.hparams
    t = m.named_tensors()
    assert list(t) == list(ref.param_shapes(2, 4, 32, 1, 3))
    assert torch.equal(t['psp.b1.conv.bias'], torch.zeros(64))
    for k in ('psp.b1.conv.weight', 'psp.out.conv.weight', 'lat2.conv.weight', 'fuse.conv.weight'):
        std = math.sqrt(2.0 / (t[k].shape[1] * math.prod(t[k].shape[2:])))
        assert abs(t[k].std().item() - std) < 0.1 * std, k
    assert torch.equal(t['fuse.bn.weight'], torch.ones(256)) and torch.equal(t['psp.b6.bn.bias'], torch.zeros(64))
    assert _model(infer_dtype='bf16').infer_dtype == torch.bfloat16
    assert _model(decoder_channels=64, levels=5).tensor('fuse.conv.weight').shape == (64, 192, 3, 3)


def test_other_architectures_unchanged():
    from interactive_unet.unet import UNet
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for arch in ('U-Net', 'U-Net++', 'LinkNet', 'Segformer'):
            assert 'decoder_channels' not in UNet(architecture=arch, pretrained=False).hparams, arch
        for arch in ('FPN', 'PSPNet', 'DeepLabV3+', 'upernet', 'UperNet'):
            with pytest.raises(NotImplementedError):
                UNet(architecture=arch, pretrained=False)


@pytest.mark.parametrize('kw', [dict(norm='group'), dict(weight_dtype='fp8_e4m3'), dict(act_dtype='fp32'), dict(act_dtype='fp16x2'),
                                dict(infer_dtype='fp16x2'), dict(infer_policy='x2m'), dict(levels=3), dict(levels=7), dict(base=48),
                                dict(num_channels=5), dict(num_classes=11), dict(decoder_channels=48), dict(decoder_channels=544),
                                dict(decoder_channels=0)])
def test_refusals(kw):
    with pytest.raises(NotImplementedError, match='UPerNet supports'):
        _model(**kw)


def test_process_group_refused_before_gpu_work():
    from interactive_unet.train_engine_f32 import make_train_engine
    m = _model()
    with pytest.raises(NotImplementedError, match='process_group'):
        make_train_engine(m, process_group=object())


def test_checkpoint_round_trip(tmp_path):
    from interactive_unet.unet import UNet
    m = _model(dim=3, levels=4, num_classes=4, num_channels=2, decoder_channels=64)
    m.load_named(ref.init_params(3, 4, 32, 2, 4, 64, seed=4, randomize_bn=True))
    path = tmp_path / 'model.ckpt'
    m.save_checkpoint(str(path))
    r = UNet.load_from_checkpoint(checkpoint_path=str(path))
    assert r.architecture == 'UPerNet' and r.dim == 3 and r.levels == 4 and r.decoder_channels == 64
    assert r.hparams['decoder_channels'] == 64
    for k, v in m.named_tensors().items():
        assert torch.equal(v, r.tensor(k)), k


def test_engine_needs_the_gpu():
    with pytest.raises(RuntimeError):
        _model().engine('eval')


def test_entry_points_check_their_arguments():
    from interactive_unet import _native as nv
    lib = nv.lib()
    ok = ctypes.c_void_p(16)
    LL, V = nv.ll_array, nv.ptr_array
    o4, s4 = V([16] * 4), LL([0] * 4)
    bad = [
        ('iunet_pn_resize', (3, 2, ok, 0, 1, 4, 4, None, None, None, 0, None, None, ok, 0, 1, 8, 8, 32, 2, None)),
        ('iunet_pn_resize', (0, 4, ok, 0, 1, 4, 4, None, None, None, 0, None, None, ok, 0, 1, 8, 8, 32, 2, None)),
        ('iunet_pn_resize', (0, 2, ok, 0, 2, 4, 4, None, None, None, 0, None, None, ok, 0, 1, 8, 8, 32, 2, None)),
        ('iunet_pn_resize', (0, 2, ok, 0, 1, 4, 4, None, None, None, 0, None, None, ok, 0, 1, 0, 8, 32, 2, None)),
        ('iunet_pn_resize', (0, 2, ok, 0, 1, 4, 4, None, None, None, 0, None, None, ok, 0, 1, 8, 8, 12, 2, None)),
        ('iunet_pn_resize', (0, 2, None, 0, 1, 4, 4, None, None, None, 0, None, None, ok, 0, 1, 8, 8, 32, 2, None)),
        ('iunet_pn_resize', (0, 2, ok, 0, 1, 4, 4, ok, None, None, 0, None, None, ok, 0, 1, 8, 8, 32, 2, None)),
        ('iunet_pn_resize', (0, 2, ok, 0, 1, 4, 4, None, None, None, 0, ok, ok, ok, 0, 1, 8, 8, 32, 2, None)),
        ('iunet_pn_resize', (0, 2, ok, 0, 1, 4, 4, None, None, ok, 0, ok, None, ok, 0, 1, 8, 8, 32, 2, None)),
        ('iunet_pn_resize', (0, 2, ok, 0, 1, 4, 4, None, None, None, 0, None, None, ok, 0, 1, 8, 8, 32, 0, None)),
        ('iunet_pn_resize_adjoint', (2, 2, ok, 0, 1, 8, 8, ok, 0, 1, 4, 4, 32, 2, 0, None)),
        ('iunet_pn_resize_adjoint', (0, 2, ok, 0, 1, 8, 8, ok, 0, 2, 4, 4, 32, 2, 0, None)),
        ('iunet_pn_resize_adjoint', (0, 2, ok, 0, 1, 8, 8, ok, 0, 1, 4, 4, 12, 2, 0, None)),
        ('iunet_pn_resize_adjoint', (0, 2, ok, 0, 1, 8, 8, None, 0, 1, 4, 4, 32, 2, 0, None)),
        ('iunet_pn_resize_adjoint', (0, 2, ok, 0, 1, 8, 8, ok, 0, 1, 4, 4, 32, 2, 2, None)),
        ('iunet_pn_pool', (3, 2, ok, 0, 1, 6, 6, o4, s4, 32, 2, None)),
        ('iunet_pn_pool', (0, 2, ok, 0, 2, 6, 6, o4, s4, 32, 2, None)),
        ('iunet_pn_pool', (0, 2, ok, 0, 1, 6, 6, V([16, 16, None, 16]), s4, 32, 2, None)),
        ('iunet_pn_pool', (0, 2, ok, 0, 1, 6, 6, None, s4, 32, 2, None)),
        ('iunet_pn_pool', (0, 2, ok, 0, 1, 6, 6, o4, s4, 36, 2, None)),
        ('iunet_pn_pool_bwd', (2, 2, None, 0, o4, s4, ok, 0, 1, 6, 6, 32, 2, None)),
        ('iunet_pn_pool_bwd', (0, 2, None, 0, o4, s4, None, 0, 1, 6, 6, 32, 2, None)),
        ('iunet_pn_pool_bwd', (0, 2, None, 0, V([None] * 4), s4, ok, 0, 1, 6, 6, 32, 2, None)),
        ('iunet_pn_pool_bwd', (0, 3, None, 0, o4, s4, ok, 0, 0, 6, 6, 32, 2, None)),
        ('iunet_pn_bias_relu_bwd', (2, ok, 0, ok, 0, ok, ok, 0, ok, 32, 2, 1, None)),
        ('iunet_pn_bias_relu_bwd', (0, ok, 0, ok, 0, None, ok, 0, ok, 32, 2, 1, None)),
        ('iunet_pn_bias_relu_bwd', (0, ok, 0, ok, 0, ok, ok, 0, ok, 32, 2, 0, None)),
        ('iunet_pn_bias_relu_bwd', (0, ok, 0, ok, 0, ok, ok, 0, ok, 20, 2, 1, None)),
    ]
    for name, args in bad:
        assert getattr(lib, name)(*args) == -1, (name, args)
