"""Segformer (architecture='Segformer') without a GPU: the functional reference against an independent torch.nn Segformer, the collapsed
form and its backward formulas against float64 autograd of smp's literal order, parameter names, shapes and counts, the constructor, the
refusals, checkpoints and the argument checks of the new native entry points."""
import ctypes
import math
import warnings

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import segformer_ref as ref


def _model(**kw):
    from interactive_unet.unet import UNet
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return UNet(architecture='Segformer', pretrained=False, **kw)


# ---- an independent torch.nn Segformer (smp's SegformerDecoder / SegmentationHead(upsampling=4) on the project's encoder)
class Stage(nn.Module):
    def __init__(self, ci, co, dim):
        super().__init__()
        Conv, BN = (nn.Conv3d, nn.BatchNorm3d) if dim == 3 else (nn.Conv2d, nn.BatchNorm2d)
        self.conv1, self.bn1 = Conv(ci, co, 3, padding=1, bias=False), BN(co)
        self.conv2, self.bn2 = Conv(co, co, 3, padding=1, bias=False), BN(co)

    def forward(self, x):
        return torch.relu(self.bn2(self.conv2(torch.relu(self.bn1(self.conv1(x))))))


class MLP(nn.Module):
    def __init__(self, ci, co):
        super().__init__()
        self.linear = nn.Linear(ci, co)

    def forward(self, x):
        N, C = x.shape[:2]
        sp = x.shape[2:]
        y = self.linear(x.flatten(2).transpose(1, 2))
        return y.transpose(1, 2).reshape(N, -1, *sp)


class TorchSegformer(nn.Module):
    def __init__(self, dim=2, levels=4, base=32, cin=1, ncls=2, C=256):
        super().__init__()
        ch = [base * 2 ** l for l in range(levels)]
        Conv, BN = (nn.Conv3d, nn.BatchNorm3d) if dim == 3 else (nn.Conv2d, nn.BatchNorm2d)
        self.dim = dim
        self.enc = nn.ModuleList(Stage(cin if l == 0 else ch[l - 1], ch[l], dim) for l in range(levels))
        self.mlp = nn.ModuleList(MLP(c, C) for c in ch)
        self.fuse = nn.Sequential()
        self.fuse.add_module('conv', Conv(levels * C, C, 1, bias=False))
        self.fuse.add_module('bn', BN(C))
        self.fuse.add_module('relu', nn.ReLU())
        self.head = Conv(C, ncls, 1)
        self.up = nn.UpsamplingBilinear2d(scale_factor=4) if dim == 2 else None

    def named_canonical(self):
        out = {}
        for k, v in self.state_dict().items():
            if k.endswith('num_batches_tracked'):
                continue
            parts = k.split('.')
            if parts[0] == 'enc':
                k = f'enc{parts[1]}.' + '.'.join(parts[2:])
            elif parts[0] == 'mlp':
                k = f'mlp{parts[1]}.{parts[3]}'
            out[k] = v
        return out

    def load_canonical(self, p):
        keys = [k for k in self.state_dict() if not k.endswith('num_batches_tracked')]
        self.load_state_dict({key: p[k] for k, key in zip(self.named_canonical(), keys)}, strict=False)

    def forward(self, x):
        feats, h = [], x
        for l, st in enumerate(self.enc):
            if l > 0:
                h = (F.max_pool3d if self.dim == 3 else F.max_pool2d)(h, 2)
            h = st(h)
            feats.append(h)
        size = [d // 4 for d in feats[0].shape[2:]]
        mode = 'trilinear' if self.dim == 3 else 'bilinear'
        outs = [F.interpolate(m(f), size=size, mode=mode, align_corners=False) for m, f in zip(self.mlp, feats)]
        lc = self.head(self.fuse(torch.cat(outs[::-1], 1)))
        if self.up is not None:
            return self.up(lc)
        return F.interpolate(lc, scale_factor=4, mode='trilinear', align_corners=True)


def test_param_names_shapes_and_counts():
    from interactive_unet import unet
    for dim, count in ((2, 1559714), (3, 3901154)):
        mod = TorchSegformer(dim=dim)
        want = {k: tuple(v.shape) for k, v in mod.named_canonical().items()}
        shapes = unet.param_shapes(dim, 4, 32, 1, 2, architecture='Segformer')
        assert set(shapes) == set(want) and all(shapes[k] == want[k] for k in want)
        assert list(shapes) == list(ref.param_shapes(dim, 4, 32, 1, 2))
        n = sum(torch.Size(v).numel() for k, v in shapes.items() if not unet._is_buffer(k))
        assert n == sum(p.numel() for p in mod.parameters()) == count
    m = unet.param_shapes(2, 5, 64, 2, 5, architecture='Segformer', decoder_channels=96)
    assert m['mlp4.weight'] == (96, 1024) and m['fuse.conv.weight'] == (96, 480, 1, 1) and m['head.weight'] == (5, 96, 1, 1)
    names = list(m)
    assert names.index('enc4.bn2.running_var') < names.index('mlp0.weight') < names.index('mlp4.bias') < names.index('fuse.conv.weight') \
        < names.index('head.weight')


@pytest.mark.parametrize('dim,shape', [(2, (2, 1, 48, 40)), (3, (2, 2, 16, 8, 24))])
def test_reference_equals_torch_module(dim, shape):
    cin = shape[1]
    mod = TorchSegformer(dim=dim, levels=4, base=32, cin=cin, ncls=3, C=64).double()
    p = ref.init_params(dim, 4, 32, cin, 3, 64, seed=2, randomize_bn=True)
    mod.load_canonical({k: v.double() for k, v in p.items()})
    x = torch.rand(shape, dtype=torch.float64)
    mod.eval()
    with torch.no_grad():
        want = mod(x)
    got = ref.forward_logits(p, x, dim=dim, levels=4)
    assert torch.allclose(got, want, atol=1e-10, rtol=1e-9)
    mod.train()
    stats = {}
    with torch.no_grad():
        want = mod(x)
    got = ref.forward_logits(p, x, dim=dim, levels=4, training=True, stats=stats)
    assert torch.allclose(got, want, atol=1e-10, rtol=1e-9)
    m, _ = stats['fuse.bn']
    assert torch.allclose(mod.fuse.bn.running_mean, 0.9 * p['fuse.bn.running_mean'].double() + 0.1 * m)


@pytest.mark.parametrize('dim,shape,levels', [(2, (2, 1, 40, 24), 4), (3, (1, 1, 16, 32, 16), 5), (2, (1, 1, 20, 12), 3)])
def test_collapsed_form_and_backward_formulas(dim, shape, levels):
    """Z = sum_l M_l R_l(X^l) + beta and dW_l = W_f,l^T G_l, dW_f,l = G_l W_l^T + r b_l^T, db_l = W_f,l^T r, dX^l = R_l^T(M_l^T dZ),
    against float64 autograd of smp's literal order (encoder outputs as free inputs)."""
    C = 32
    p = ref.init_params(dim, levels, 32, 1, 2, C, seed=3, randomize_bn=True)
    p = {k: v.double() for k, v in p.items()}
    x = torch.rand(shape, dtype=torch.float64)
    size = ref.target_size(x)
    for training in (False, True):
        feats = [f.detach().requires_grad_(True) for f in ref.encoder(p, x, dim, levels, training)]
        pr = {k: v.clone().requires_grad_(k.startswith('mlp') or k == 'fuse.conv.weight') for k, v in p.items()}
        Z = ref.decoder_literal(pr, feats, size, dim)
        M, beta = ref.collapsed_ops(p, levels)
        R = [ref.resize(f.detach(), size, dim) for f in feats]
        Zc = sum(torch.einsum('kc,nc...->nk...', M[l], R[l]) for l in range(levels)) + beta.view((1, -1) + (1,) * dim)
        assert (Z - Zc).abs().max().item() <= 1e-10
        dZ = torch.randn(Z.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(int(training)))
        Z.backward(dZ)
        r = dZ.sum((0,) + tuple(range(2, 2 + dim)))
        wf = p['fuse.conv.weight'].reshape(C, levels * C)
        for l in range(levels):
            blk = wf[:, (levels - 1 - l) * C:(levels - l) * C]
            G = torch.einsum('nc...,nk...->ck', dZ, R[l])
            assert (pr[f'mlp{l}.weight'].grad - blk.t() @ G).abs().max().item() <= 1e-10
            assert (pr[f'mlp{l}.bias'].grad - blk.t() @ r).abs().max().item() <= 1e-10
            dwf = pr['fuse.conv.weight'].grad.reshape(C, levels * C)[:, (levels - 1 - l) * C:(levels - l) * C]
            assert (dwf - (G @ p[f'mlp{l}.weight'].t() + torch.outer(r, p[f'mlp{l}.bias']))).abs().max().item() <= 1e-10
            u = torch.einsum('kc,nk...->nc...', M[l], dZ)
            xl = torch.zeros_like(feats[l], requires_grad=True)
            (ref.resize(xl, size, dim) * u).sum().backward()
            assert (feats[l].grad - xl.grad).abs().max().item() <= 1e-10


def test_constructor_hparams_and_init():
    m = _model(num_classes=3)
    assert m.architecture == 'Segformer' and m.act_dtype == torch.float16 and m.infer_dtype == torch.float32
    assert m.hparams['decoder_segmentation_channels'] == 256 and m.decoder_segmentation_channels == 256
    assert 'decoder_channels' not in m.hparams
    t = m.named_tensors()
    assert list(t) == list(ref.param_shapes(2, 4, 32, 1, 3))
    for l in range(4):
        w = t[f'mlp{l}.weight']
        std = math.sqrt(2.0 / w.shape[1])
        assert abs(w.std().item() - std) < 0.1 * std
        assert torch.equal(t[f'mlp{l}.bias'], torch.zeros(256))
    w = t['fuse.conv.weight']
    assert abs(w.std().item() - math.sqrt(2.0 / 1024)) < 0.1 * math.sqrt(2.0 / 1024)
    assert torch.equal(t['fuse.bn.weight'], torch.ones(256)) and torch.equal(t['fuse.bn.bias'], torch.zeros(256))
    assert _model(infer_dtype='bf16').infer_dtype == torch.bfloat16
    assert _model(decoder_segmentation_channels=64, levels=3).tensor('fuse.conv.weight').shape == (64, 192, 1, 1)


def test_other_architectures_hparams_unchanged():
    from interactive_unet.unet import UNet
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for arch in ('U-Net', 'U-Net++', 'LinkNet', 'DeepLabV3'):
            hp = UNet(architecture=arch, pretrained=False).hparams
            assert 'decoder_segmentation_channels' not in hp, arch
        assert not any(k.startswith('decoder_') for k in UNet(architecture='U-Net', pretrained=False).hparams)


@pytest.mark.parametrize('kw', [dict(norm='group'), dict(weight_dtype='fp8_e4m3'), dict(act_dtype='fp32'), dict(act_dtype='fp16x2'),
                                dict(infer_dtype='fp16x2'), dict(infer_policy='x2m'), dict(levels=7), dict(levels=2), dict(base=48),
                                dict(num_channels=5), dict(num_classes=11), dict(num_classes=1), dict(decoder_segmentation_channels=48),
                                dict(decoder_segmentation_channels=544), dict(decoder_segmentation_channels=0),
                                dict(decoder_segmentation_channels=64.0)])
def test_refusals(kw):
    with pytest.raises(NotImplementedError, match='Segformer supports'):
        _model(**kw)


def test_process_group_refused_before_gpu_work():
    from interactive_unet.train_engine_f32 import make_train_engine
    m = _model()
    with pytest.raises(NotImplementedError, match='process_group'):
        make_train_engine(m, process_group=object())


def test_checkpoint_round_trip(tmp_path):
    from interactive_unet.unet import UNet
    m = _model(dim=3, levels=3, num_classes=4, num_channels=2, decoder_segmentation_channels=64)
    m.load_named(ref.init_params(3, 3, 32, 2, 4, 64, seed=4, randomize_bn=True))
    path = tmp_path / 'model.ckpt'
    m.save_checkpoint(str(path))
    r = UNet.load_from_checkpoint(checkpoint_path=str(path))
    assert r.architecture == 'Segformer' and r.dim == 3 and r.levels == 3 and r.decoder_segmentation_channels == 64
    for k, v in m.named_tensors().items():
        assert torch.equal(v, r.tensor(k)), k


def test_engine_needs_the_gpu():
    with pytest.raises(RuntimeError):
        _model().engine('eval')


def test_entry_points_check_their_arguments():
    from interactive_unet import _native as nv
    lib = nv.lib()
    ok = ctypes.c_void_p(16)
    I, LL, V = nv.int_array, nv.ll_array, nv.ptr_array
    x1, ss1, c1, d1 = V([16]), LL([0]), I([32]), I([1, 8, 8])
    assert lib.iunet_sf_stats_parts(2, 1, 8, 8) == 2 and lib.iunet_sf_stats_parts(0, 1, 8, 8) == -1
    assert lib.iunet_sf_wgrad_slab_floats(2, 1, 8, 8, 32, 64) > 0 and lib.iunet_sf_wgrad_slab_floats(2, 1, 8, 8, 0, 64) == -1
    ch = I([32, 64, 128])
    bad = [
        ('iunet_sf_pack', (3, 3, 64, ch, ok, V([16] * 3), V([16] * 3), None, None, None, None, 1e-5, ok, None, ok, None)),
        ('iunet_sf_pack', (0, 7, 64, I([32] * 7), ok, V([16] * 7), V([16] * 7), None, None, None, None, 1e-5, ok, None, ok, None)),
        ('iunet_sf_pack', (0, 3, 60, ch, ok, V([16] * 3), V([16] * 3), None, None, None, None, 1e-5, ok, None, ok, None)),
        ('iunet_sf_pack', (0, 3, 64, I([32, 60, 128]), ok, V([16] * 3), V([16] * 3), None, None, None, None, 1e-5, ok, None, ok, None)),
        ('iunet_sf_pack', (0, 3, 64, ch, ok, V([16, None, 16]), V([16] * 3), None, None, None, None, 1e-5, ok, None, ok, None)),
        ('iunet_sf_pack', (0, 3, 64, ch, ok, V([16] * 3), V([16] * 3), ok, None, None, None, 1e-5, ok, None, ok, None)),
        ('iunet_sf_pack', (0, 3, 64, ch, ok, V([16] * 3), V([16] * 3), None, None, None, None, 1e-5, None, None, ok, None)),
        ('iunet_sf_gemm', (3, 2, 1, x1, ss1, c1, d1, None, None, ok, ok, ok, 0, None, 0, 2, 1, 8, 8, 64, None)),
        ('iunet_sf_gemm', (0, 4, 1, x1, ss1, c1, d1, None, None, ok, ok, ok, 0, None, 0, 2, 1, 8, 8, 64, None)),
        ('iunet_sf_gemm', (0, 2, 1, x1, ss1, c1, d1, None, None, ok, ok, ok, 0, None, 0, 2, 2, 8, 8, 64, None)),
        ('iunet_sf_gemm', (0, 2, 0, x1, ss1, c1, d1, None, None, ok, ok, ok, 0, None, 0, 2, 1, 8, 8, 64, None)),
        ('iunet_sf_gemm', (0, 2, 7, V([16] * 7), LL([0] * 7), I([32] * 7), I([1, 8, 8] * 7), None, None, ok, ok, ok, 0, None, 0, 2, 1, 8, 8,
                           64, None)),
        ('iunet_sf_gemm', (0, 2, 1, x1, ss1, I([40]), d1, None, None, ok, ok, ok, 0, None, 0, 2, 1, 8, 8, 64, None)),
        ('iunet_sf_gemm', (0, 2, 1, x1, ss1, c1, I([2, 8, 8]), None, None, ok, ok, ok, 0, None, 0, 2, 1, 8, 8, 64, None)),
        ('iunet_sf_gemm', (0, 2, 1, x1, ss1, c1, I([1, 0, 8]), None, None, ok, ok, ok, 0, None, 0, 2, 1, 8, 8, 64, None)),
        ('iunet_sf_gemm', (0, 2, 1, V([None]), ss1, c1, d1, None, None, ok, ok, ok, 0, None, 0, 2, 1, 8, 8, 64, None)),
        ('iunet_sf_gemm', (0, 2, 1, x1, ss1, c1, d1, V([16]), None, ok, ok, ok, 0, None, 0, 2, 1, 8, 8, 64, None)),
        ('iunet_sf_gemm', (0, 2, 1, x1, ss1, c1, d1, None, None, ok, ok, ok, 0, None, 0, 2, 1, 8, 8, 72, None)),
        ('iunet_sf_gemm', (0, 2, 1, x1, ss1, c1, d1, None, None, ok, ok, ok, 0, None, 0, 2, 1, 8, 8, 528, None)),
        ('iunet_sf_gemm', (0, 2, 1, x1, ss1, c1, d1, None, None, ok, ok, ok, 0, None, 2, 2, 1, 8, 8, 64, None)),
        ('iunet_sf_gemm', (0, 2, 1, x1, ss1, c1, d1, None, None, ok, ok, ok, 0, ok, 1, 2, 1, 8, 8, 64, None)),
        ('iunet_sf_gemm', (0, 2, 1, x1, ss1, c1, d1, None, None, ok, None, ok, 0, None, 0, 2, 1, 8, 8, 64, None)),
        ('iunet_sf_wgrad', (2, 2, 1, x1, ss1, c1, d1, None, None, ok, 0, ok, ok, 2, 1, 8, 8, 64, None)),
        ('iunet_sf_wgrad', (0, 2, 1, x1, ss1, c1, d1, None, None, ok, 0, ok, ok, 2, 1, 8, 8, 60, None)),
        ('iunet_sf_wgrad', (0, 2, 1, x1, ss1, c1, d1, None, None, None, 0, ok, ok, 2, 1, 8, 8, 64, None)),
        ('iunet_sf_wgrad', (0, 3, 1, x1, ss1, c1, d1, None, None, ok, 0, ok, ok, 2, 0, 8, 8, 64, None)),
        ('iunet_sf_adjoint', (2, 2, ok, 0, 1, 4, 4, ok, 0, 1, 16, 16, 32, 2, None)),
        ('iunet_sf_adjoint', (0, 2, ok, 0, 1, 4, 4, ok, 0, 2, 16, 16, 32, 2, None)),
        ('iunet_sf_adjoint', (0, 2, ok, 0, 1, 4, 4, ok, 0, 1, 16, 16, 12, 2, None)),
        ('iunet_sf_adjoint', (0, 2, None, 0, 1, 4, 4, ok, 0, 1, 16, 16, 32, 2, None)),
        ('iunet_sf_param_grads', (3, 64, ch, ok, V([16] * 3), V([16] * 3), ok, ok, 0, V([16] * 3), V([16] * 3), ok, None)),
        ('iunet_sf_param_grads', (3, 64, ch, ok, V([16] * 3), V([16] * 3), None, ok, 2, V([16] * 3), V([16] * 3), ok, None)),
        ('iunet_sf_param_grads', (3, 64, ch, ok, V([16] * 3), V([16] * 3), ok, ok, 2, V([16, 16, None]), V([16] * 3), ok, None)),
        ('iunet_sf_param_grads', (0, 64, ch, ok, V([16] * 3), V([16] * 3), ok, ok, 2, V([16] * 3), V([16] * 3), ok, None)),
    ]
    for name, args in bad:
        assert getattr(lib, name)(*args) == -1, (name, args)
