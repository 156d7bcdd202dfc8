"""DeepLabV3 (architecture='DeepLabV3') without a GPU: parameter names, shapes and counts against an independent torch.nn DeepLabV3, the
functional reference against that module (eval and training with the same dropout mask), the constructor, the refusals, checkpoints and
the argument checks of the new native entry points."""
import ctypes
import math
import warnings

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import deeplabv3_ref as ref


def _model(**kw):
    from interactive_unet.unet import UNet
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return UNet(architecture='DeepLabV3', pretrained=False, **kw)


# ---- an independent torch.nn DeepLabV3 (smp's ASPP / DeepLabV3Decoder / SegmentationHead on the project's encoder)
class ConvBnRelu(nn.Sequential):
    def __init__(self, ci, co, k, dim, dilation=1):
        Conv, BN = (nn.Conv3d, nn.BatchNorm3d) if dim == 3 else (nn.Conv2d, nn.BatchNorm2d)
        super().__init__()
        self.conv = Conv(ci, co, k, padding=dilation * (k // 2), dilation=dilation, bias=False)
        self.bn = BN(co)
        self.relu = nn.ReLU()


class Stage(nn.Module):
    def __init__(self, ci, co, dim):
        super().__init__()
        Conv, BN = (nn.Conv3d, nn.BatchNorm3d) if dim == 3 else (nn.Conv2d, nn.BatchNorm2d)
        self.conv1, self.bn1 = Conv(ci, co, 3, padding=1, bias=False), BN(co)
        self.conv2, self.bn2 = Conv(co, co, 3, padding=1, bias=False), BN(co)

    def forward(self, x):
        return torch.relu(self.bn2(self.conv2(torch.relu(self.bn1(self.conv1(x))))))


class ASPPPooling(nn.Module):
    def __init__(self, ci, co, dim):
        super().__init__()
        Conv, BN = (nn.Conv3d, nn.BatchNorm3d) if dim == 3 else (nn.Conv2d, nn.BatchNorm2d)
        self.dim = dim
        self.conv, self.bn = Conv(ci, co, 1, bias=False), BN(co)

    def forward(self, x):
        size = x.shape[2:]
        y = torch.relu(self.bn(self.conv(x.mean(dim=tuple(range(2, x.dim())), keepdim=True))))
        return F.interpolate(y, size=size, mode='trilinear' if self.dim == 3 else 'bilinear', align_corners=False)


class TorchDeepLabV3(nn.Module):
    def __init__(self, dim=2, levels=4, base=32, cin=1, ncls=2, C=256, rates=(12, 24, 36), p_drop=0.5):
        super().__init__()
        ch = [base * 2 ** l for l in range(levels)]
        self.dim, self.levels = dim, levels
        self.enc = nn.ModuleList(Stage(cin if l == 0 else ch[l - 1], ch[l], dim) for l in range(levels))
        self.b0 = ConvBnRelu(ch[-1], C, 1, dim)
        self.b1, self.b2, self.b3 = (ConvBnRelu(ch[-1], C, 3, dim, r) for r in rates)
        self.pool = ASPPPooling(ch[-1], C, dim)
        self.project = ConvBnRelu(5 * C, C, 1, dim)
        self.drop = nn.Dropout(p_drop)
        self.dec = ConvBnRelu(C, C, 3, dim)
        self.head = (nn.Conv3d if dim == 3 else nn.Conv2d)(C, ncls, 1)

    def named_canonical(self):
        out = {}
        for k, v in self.state_dict().items():
            if k.endswith('num_batches_tracked'):
                continue
            if k.startswith('enc.'):
                parts = k.split('.')
                k = f'enc{parts[1]}.' + '.'.join(parts[2:])
            elif k.split('.')[0] in ('b0', 'b1', 'b2', 'b3', 'pool', 'project'):
                k = 'aspp.' + k
            out[k] = v
        return out

    def load_canonical(self, p):
        own = self.named_canonical()
        sd = {}
        for (k, _), key in zip(own.items(), [k for k in self.state_dict() if not k.endswith('num_batches_tracked')]):
            sd[key] = p[k]
        self.load_state_dict(sd, strict=False)

    def forward(self, x, mask=None):
        h = x
        for l, st in enumerate(self.enc):
            if l > 0:
                h = (F.max_pool3d if self.dim == 3 else F.max_pool2d)(h, 2)
            h = st(h)
        P = self.project(torch.cat([self.b0(h), self.b1(h), self.b2(h), self.b3(h), self.pool(h)], 1))
        if self.training and mask is not None:
            P = P * mask.to(P.dtype) / (1.0 - self.drop.p)
        else:
            P = self.drop(P)
        lc = self.head(self.dec(P))
        return F.interpolate(lc, scale_factor=2 ** (self.levels - 1), mode='trilinear' if self.dim == 3 else 'bilinear', align_corners=True)


def test_param_names_shapes_and_count():
    from interactive_unet import unet
    for dim in (2, 3):
        mod = TorchDeepLabV3(dim=dim)
        want = {k: tuple(v.shape) for k, v in mod.named_canonical().items()}
        shapes = unet.param_shapes(dim, 4, 32, 1, 2, architecture='DeepLabV3')
        assert set(shapes) == set(want) and all(shapes[k] == want[k] for k in want)
        assert list(shapes) == list(ref.param_shapes(dim, 4, 32, 1, 2))
        count = sum(torch.Size(v).numel() for k, v in shapes.items() if not unet._is_buffer(k))
        assert count == sum(p.numel() for p in mod.parameters())
    m = unet.param_shapes(2, 3, 64, 2, 5, architecture='DeepLabV3', decoder_channels=96)
    assert m['aspp.project.conv.weight'] == (96, 480, 1, 1) and m['aspp.b1.conv.weight'] == (96, 256, 3, 3) and m['head.weight'] == (5, 96, 1, 1)
    assert unet.param_shapes(2, 4, 32, 1, 2) == unet.param_shapes(2, 4, 32, 1, 2, 'U-Net')


@pytest.mark.parametrize('dim,shape', [(2, (2, 1, 48, 40)), (3, (2, 2, 16, 8, 16))])
def test_reference_equals_torch_module(dim, shape):
    torch.manual_seed(0)
    cin = shape[1]
    mod = TorchDeepLabV3(dim=dim, levels=3, base=32, cin=cin, ncls=3, C=64, rates=(2, 5, 9), p_drop=0.3).double()
    p = ref.init_params(dim, 3, 32, cin, 3, 64, seed=2, randomize_bn=True)
    mod.load_canonical({k: v.double() for k, v in p.items()})
    x = torch.rand(shape, dtype=torch.float64)
    mod.eval()
    with torch.no_grad():
        want = mod(x)
    got = ref.forward_logits(p, x, dim=dim, levels=3, rates=(2, 5, 9))
    assert torch.allclose(got, want, atol=1e-10, rtol=1e-9)
    mod.train()
    grid = tuple(s // 4 for s in shape[2:])
    mask = (torch.rand((shape[0], 64) + grid) > 0.3).to(torch.uint8)
    stats = {}
    with torch.no_grad():
        want = mod(x, mask)
    got = ref.forward_logits(p, x, dim=dim, levels=3, rates=(2, 5, 9), training=True, mask=mask, p_drop=0.3, stats=stats)
    assert torch.allclose(got, want, atol=1e-10, rtol=1e-9)
    # the running statistics the module updated are those the reference reports
    rm = mod.pool.bn.running_mean
    m, v = stats['aspp.pool.bn']
    assert torch.allclose(rm, 0.9 * p['aspp.pool.bn.running_mean'].double() + 0.1 * m)


def test_constructor_hparams_and_init():
    m = _model(num_classes=3)
    assert m.architecture == 'DeepLabV3' and m.act_dtype == torch.float16 and m.infer_dtype == torch.float32
    assert m.hparams['decoder_channels'] == 256 and m.hparams['decoder_atrous_rates'] == [12, 24, 36]
    assert m.hparams['decoder_aspp_dropout'] == 0.5
    t = m.named_tensors()
    assert list(t) == list(ref.param_shapes(2, 4, 32, 1, 3))
    for prefix in ('aspp.b0', 'aspp.b2', 'aspp.pool', 'aspp.project', 'dec'):
        assert torch.equal(t[prefix + '.bn.weight'], torch.ones(256)) and torch.equal(t[prefix + '.bn.running_var'], torch.ones(256))
        assert torch.equal(t[prefix + '.bn.bias'], torch.zeros(256))
        w = t[prefix + '.conv.weight']
        std = math.sqrt(2.0 / (w.shape[1] * math.prod(w.shape[2:])))
        assert abs(w.std().item() - std) < 0.1 * std
    assert _model(infer_dtype='bf16').infer_dtype == torch.bfloat16
    m = _model(decoder_channels=64, decoder_atrous_rates=(1, 2, 3), decoder_aspp_dropout=0.0)
    assert m.tensor('aspp.project.conv.weight').shape == (64, 320, 1, 1)


def test_unet_hparams_unchanged():
    from interactive_unet.unet import UNet
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for arch in ('U-Net', 'U-Net++', 'LinkNet'):
            hp = UNet(architecture=arch, pretrained=False).hparams
            assert not any(k.startswith('decoder_') for k in hp), arch


@pytest.mark.parametrize('kw', [dict(norm='group'), dict(weight_dtype='fp8_e4m3'), dict(act_dtype='fp32'), dict(act_dtype='fp16x2'),
                                dict(infer_dtype='fp16x2'), dict(infer_policy='x2m'), dict(levels=7), dict(levels=1), dict(base=48),
                                dict(num_channels=5), dict(num_classes=11), dict(decoder_channels=48), dict(decoder_channels=544),
                                dict(decoder_channels=0), dict(decoder_atrous_rates=(12, 24)), dict(decoder_atrous_rates=(12, 0, 36)),
                                dict(decoder_atrous_rates=(12, 24.5, 36)), dict(decoder_atrous_rates=None)])
def test_refusals(kw):
    with pytest.raises(NotImplementedError, match='DeepLabV3 supports'):
        _model(**kw)


def test_deeplabv3_plus_and_others_still_refused():
    from interactive_unet.unet import UNet
    for arch in ('DeepLabV3+', 'deeplabv3', 'DeepLabV3 ', 'PSPNet', 'FPN'):
        with pytest.raises(NotImplementedError):
            UNet(architecture=arch, pretrained=False)


def test_checkpoint_round_trip(tmp_path):
    from interactive_unet.unet import UNet
    m = _model(dim=3, levels=3, num_classes=4, num_channels=2, decoder_channels=64, decoder_atrous_rates=(2, 3, 4), decoder_aspp_dropout=0.2)
    m.load_named(ref.init_params(3, 3, 32, 2, 4, 64, seed=4, randomize_bn=True))
    path = tmp_path / 'model.ckpt'
    m.save_checkpoint(str(path))
    r = UNet.load_from_checkpoint(checkpoint_path=str(path))
    assert r.architecture == 'DeepLabV3' and r.dim == 3 and r.levels == 3
    assert r.decoder_channels == 64 and r.decoder_atrous_rates == (2, 3, 4) and r.decoder_aspp_dropout == 0.2
    for k, v in m.named_tensors().items():
        assert torch.equal(v, r.tensor(k)), k


def test_engine_needs_the_gpu():
    with pytest.raises(RuntimeError):
        _model().engine('eval')


def test_entry_points_check_their_arguments():
    from interactive_unet import _native as nv
    lib = nv.lib()
    ok = ctypes.c_void_p(16)
    I = nv.int_array
    assert lib.iunet_dl_num_taps(3, 24, 16, 16, 16) == 1 and lib.iunet_dl_num_taps(3, 12, 16, 16, 16) == 27
    assert lib.iunet_dl_num_taps(2, 36, 1, 64, 64) == 9 and lib.iunet_dl_num_taps(2, 0, 1, 8, 8) == 1 and lib.iunet_dl_num_taps(4, 1, 1, 1, 1) == -1
    assert lib.iunet_dl_num_taps(2, 8, 1, 8, 9) == 3            # rows at +-8 leave an 8-row grid, columns at +-8 stay in a 9-wide one
    bad = [
        ('iunet_dl_pack', (3, 2, 0, 3, ok, None, None, None, None, 1e-5, ok, None, 64, 64, 64, 0, 0, 576, None)),
        ('iunet_dl_pack', (0, 2, 2, 3, ok, None, None, None, None, 1e-5, ok, None, 64, 64, 64, 0, 0, 576, None)),
        ('iunet_dl_pack', (0, 2, 0, 3, ok, None, None, None, None, 1e-5, ok, None, 64, 64, 64, 0, 0, 575, None)),
        ('iunet_dl_pack', (0, 2, 0, 1, None, None, None, None, None, 1e-5, ok, None, 64, 64, 64, 0, 0, 64, None)),
        ('iunet_dl_conv_fwd', (0, 2, ok, 0, ok, 0, ok, 576, 1, I([1]), I([0]), I([0]), None, None, None, None, 1.0, None, 0, 2, 1, 8, 8, 60, 64, None)),
        ('iunet_dl_conv_fwd', (0, 2, ok, 0, ok, 0, ok, 576, 1, I([1]), I([0]), I([0]), None, None, None, None, 1.0, None, 0, 2, 2, 8, 8, 64, 64, None)),
        ('iunet_dl_conv_fwd', (0, 2, ok, 0, ok, 0, ok, 512, 1, I([1]), I([0]), I([0]), None, None, None, None, 1.0, None, 0, 2, 1, 8, 8, 64, 64, None)),
        ('iunet_dl_conv_fwd', (0, 2, ok, 0, ok, 0, ok, 576, 5, I([1] * 5), I([0] * 5), I([0] * 5), None, None, None, None, 1.0, None, 0, 2, 1, 8, 8, 64, 64, None)),
        ('iunet_dl_conv_fwd', (0, 2, ok, 0, ok, 0, ok, 576, 1, I([1]), I([0]), I([0]), None, None, None, None, 1.0, None, 1, 2, 1, 8, 8, 64, 64, None)),
        ('iunet_dl_conv_fwd', (0, 2, ok, 0, ok, 0, ok, 576, 1, I([-1]), I([0]), I([0]), None, None, None, None, 1.0, None, 0, 2, 1, 8, 8, 64, 64, None)),
        ('iunet_dl_conv_fwd', (2, 2, ok, 0, ok, 0, ok, 576, 1, I([1]), I([0]), I([0]), None, None, None, None, 1.0, None, 0, 2, 1, 8, 8, 64, 64, None)),
        ('iunet_dl_wgrad', (0, 2, 1, ok, 0, 0, ok, 0, None, None, None, ok, 64, 0, 1.0, 2, 1, 8, 8, 64, 64, None)),
        ('iunet_dl_wgrad', (0, 2, 1, ok, 0, 0, ok, 0, None, None, ok, ok, 64, 8, 1.0, 2, 1, 8, 8, 64, 64, None)),
        ('iunet_dl_wgrad', (0, 2, 1, ok, 0, 4, ok, 0, None, None, ok, ok, 64, 0, 1.0, 2, 1, 8, 8, 64, 64, None)),
        ('iunet_dl_f32_conv_fwd', (2, 1, ok, 0, ok, 0, ok, 576, None, None, 2, 1, 8, 8, 64, 64, None)),
        ('iunet_dl_f32_conv_fwd', (2, 1, ok, 0, ok, 0, ok, 570, ok, None, 2, 1, 8, 8, 64, 64, None)),
        ('iunet_dl_chansum', (0, ok, 0, ok, 1.0, 12, 2, 64, None)),
        ('iunet_dl_chansum', (3, ok, 0, ok, 1.0, 16, 2, 64, None)),
        ('iunet_dl_pool_gemv', (None, ok, ok, None, 2, 64, 64, None)),
        ('iunet_dl_pool_psb', (ok, ok, None, None, None, None, None, 1e-5, ok, ok, None, None, ok, 2, 64, None)),
        ('iunet_dl_pool_psb', (ok, None, None, None, None, None, None, 1e-5, ok, ok, None, None, ok, 2, 64, None)),
        ('iunet_dl_pool_bwd', (ok,) * 15 + (1, 64, 64, None)),
        ('iunet_dl_pool_bwd', (ok,) * 14 + (None, 2, 64, 64, None)),
        ('iunet_dl_dropout', (0, 0, ok, 0, ok, 0, None, None, None, 0.5, 16, 2, 64, None)),
        ('iunet_dl_dropout', (0, 1, ok, 0, ok, 0, None, None, None, 1.0, 16, 2, 64, None)),
        ('iunet_dl_up_head', (2, ok, 11, 1, 8, 8, 8, None, None, ok, None, 1.0, 0, 2, None)),
        ('iunet_dl_up_head', (2, ok, 2, 2, 8, 8, 8, None, None, ok, None, 1.0, 0, 2, None)),
        ('iunet_dl_up_head', (2, ok, 2, 1, 8, 8, 8, ok, None, None, None, 1.0, 0, 2, None)),
        ('iunet_dl_up_loss_fwd', (2, ok, 2, 1, 8, 8, 8, ok, None, 0, 7, ok, ok, ok, 2, None)),
        ('iunet_dl_up_loss_fwd', (2, ok, 2, 1, 8, 8, 8, ok, None, 2, 0, ok, ok, ok, 2, None)),
        ('iunet_dl_up_loss_bwd', (2, ok, 2, 1, 8, 8, 8, ok, None, 0, ok, None, ok, ok, ok, 2, None)),
        ('iunet_dl_up_loss_bwd', (2, ok, 2, 1, 8, 8, 0, ok, None, 0, ok, ok, ok, ok, ok, 2, None)),
        ('iunet_dl_head_bwd', (0, ok, 0, 12, ok, ok, 2, ok, 0, ok, ok, ok, 2, 64, None)),
        ('iunet_dl_head_bwd', (0, ok, 0, 16, ok, ok, 1, ok, 0, ok, ok, ok, 2, 64, None)),
    ]
    for name, args in bad:
        assert getattr(lib, name)(*args) == -1, (name, args)
    assert lib.iunet_dl_wgrad_slab_floats(2, 1, 2, 1, 8, 8, 64, 64) > 0 and lib.iunet_dl_wgrad_slab_floats(2, -1, 2, 1, 8, 8, 64, 64) == -1
