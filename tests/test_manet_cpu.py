"""MA-Net (architecture='MA-Net') without a GPU: the entry points of csrc/manet.hip are declared, bound and refuse arguments no decoder has,
the benchmark's work count matches a recount; the functional reference against an independent torch.nn MA-Net, parameter names, shapes and
counts, the constructor, the refusals and checkpoints."""
import ctypes
import importlib.util
import math
import os
import warnings

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import manet_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = ('iunet_ma_attn_fwd', 'iunet_ma_f32_attn_fwd', 'iunet_ma_attn_bwd', 'iunet_ma_gate', 'iunet_ma_gate_bwd', 'iunet_ma_up_gate',
                'iunet_ma_up_gate_dg_parts', 'iunet_ma_up_gate_dg', 'iunet_ma_up_gate_bwd', 'iunet_ma_add_mean_grad')


def test_entry_points_are_declared_and_bound():
    from interactive_unet import _native as nv
    lib, sigs = nv.lib(), nv.signatures()
    for name in ENTRY_POINTS:
        assert name in sigs and getattr(lib, name).argtypes == sigs[name][1], name
    # the attention forward of the issue's contract: dtype, q, q_ss, bq, k, k_ss, bk, v, v_ss, x, x_ss, bv, y, y_ss, lse, Cb, T, N, stream
    assert len(sigs['iunet_ma_attn_fwd'][1]) == 19 and len(sigs['iunet_ma_f32_attn_fwd'][1]) == 18


def _attn(dtype=0, Cb=128, T=15, N=2, null=None):
    ok = ctypes.c_void_p(16)
    a = [dtype, ok, 0, ok, ok, 0, ok, ok, 0, ok, 0, ok, ok, 0, ok, Cb, T, N, None]
    if null is not None:
        a[null] = None
    return tuple(a)


def _attn_bwd(dtype=0, Cb=128, T=15, N=2, null=None):
    ok = ctypes.c_void_p(16)
    a = [dtype, ok, 0, ok, ok, 0, ok, ok, 0, ok, 0, ok, ok, ok, 0, ok, 0, ok, 0, Cb, T, N, None]
    if null is not None:
        a[null] = None
    return tuple(a)


def test_entry_points_check_their_arguments():
    """Every refusal returns before a launch (status -1 with a message), so none of this needs a GPU."""
    from interactive_unet import _native as nv
    lib = nv.lib()
    ok = ctypes.c_void_p(16)
    p10 = (ok,) * 10
    bad = [
        ('iunet_ma_attn_fwd', _attn(dtype=2)),                     # the fp32 form has its own entry point
        ('iunet_ma_attn_fwd', _attn(Cb=64)), ('iunet_ma_attn_fwd', _attn(Cb=192)), ('iunet_ma_attn_fwd', _attn(Cb=640)),
        ('iunet_ma_attn_fwd', _attn(T=0)), ('iunet_ma_attn_fwd', _attn(T=65537)), ('iunet_ma_attn_fwd', _attn(N=0)),
        ('iunet_ma_attn_fwd', _attn(null=3)), ('iunet_ma_attn_fwd', _attn(null=14)),
        ('iunet_ma_f32_attn_fwd', _attn(T=65537)[1:]), ('iunet_ma_f32_attn_fwd', _attn(Cb=100)[1:]), ('iunet_ma_f32_attn_fwd', _attn(null=1)[1:]),
        ('iunet_ma_attn_bwd', _attn_bwd(dtype=2)), ('iunet_ma_attn_bwd', _attn_bwd(Cb=96)), ('iunet_ma_attn_bwd', _attn_bwd(T=70000)),
        ('iunet_ma_attn_bwd', _attn_bwd(null=12)), ('iunet_ma_attn_bwd', _attn_bwd(null=17)),
        ('iunet_ma_gate', p10 + (ok, ok, ok, 0, 2, 2, None)), ('iunet_ma_gate', p10 + (ok, ok, ok, 32, 0, 2, None)),
        ('iunet_ma_gate', p10 + (ok, ok, ok, 32, 2, 0, None)), ('iunet_ma_gate', p10 + (ok, None, ok, 32, 2, 2, None)),
        ('iunet_ma_gate_bwd', (ok,) * 20 + (32, 64, 2, None)), ('iunet_ma_gate_bwd', (ok,) * 19 + (None, 32, 2, 2, None)),
        ('iunet_ma_up_gate', (3, 2, ok, 0, None, None, ok, ok, 0, 1, 3, 5, 32, 2, None)),
        ('iunet_ma_up_gate', (0, 4, ok, 0, None, None, ok, ok, 0, 1, 3, 5, 32, 2, None)),
        ('iunet_ma_up_gate', (0, 2, ok, 0, None, None, ok, ok, 0, 2, 3, 5, 32, 2, None)),
        ('iunet_ma_up_gate', (0, 2, ok, 0, ok, None, ok, ok, 0, 1, 3, 5, 32, 2, None)),
        ('iunet_ma_up_gate', (0, 2, ok, 0, None, None, ok, ok, 0, 1, 3, 5, 12, 2, None)),
        ('iunet_ma_up_gate', (0, 2, ok, 0, None, None, None, ok, 0, 1, 3, 5, 32, 2, None)),
        ('iunet_ma_up_gate_dg', (2, 2, ok, 0, ok, 0, None, None, ok, ok, 1, 3, 5, 32, 2, None)),
        ('iunet_ma_up_gate_dg', (0, 2, ok, 0, ok, 0, None, ok, ok, ok, 1, 3, 5, 32, 2, None)),
        ('iunet_ma_up_gate_dg', (0, 3, ok, 0, ok, 0, None, None, ok, ok, 0, 3, 5, 32, 2, None)),
        ('iunet_ma_up_gate_dg', (0, 2, ok, 0, ok, 0, None, None, None, ok, 1, 64, 64, 32, 2, None)),      # two parts need the workspace
        ('iunet_ma_up_gate_dg_parts', (4, 2, 1, 3, 5, 32)), ('iunet_ma_up_gate_dg_parts', (2, 2, 1, 3, 5, 12)),
        ('iunet_ma_up_gate_bwd', (2, 2, ok, 0, ok, None, ok, 0, 1, 3, 5, 32, 2, None)),
        ('iunet_ma_up_gate_bwd', (0, 2, ok, 0, None, None, ok, 0, 1, 3, 5, 32, 2, None)),
        ('iunet_ma_up_gate_bwd', (0, 2, ok, 0, ok, None, ok, 0, 1, 3, 5, 20, 2, None)),
        ('iunet_ma_add_mean_grad', (2, ok, 0, ok, 32, 2, 15, None)), ('iunet_ma_add_mean_grad', (0, ok, 0, None, 32, 2, 15, None)),
        ('iunet_ma_add_mean_grad', (0, ok, 0, ok, 32, 2, 0, None)), ('iunet_ma_add_mean_grad', (0, ok, 0, ok, 20, 2, 15, None)),
    ]
    for name, args in bad:
        assert getattr(lib, name)(*args) == -1, (name, args)
        assert name[len('iunet_'):] in lib.iunet_last_error().decode(), (name, lib.iunet_last_error())


def test_dg_parts():
    """One part up to 2048 coarse voxels, then one per 2048, at most 64."""
    from interactive_unet import _native as nv
    lib = nv.lib()
    assert [lib.iunet_ma_up_gate_dg_parts(2, 2, 1, h, w, 32) for h, w in ((3, 5), (32, 64), (32, 65), (256, 256), (1024, 1024))] == [1, 1, 2, 32, 64]
    assert lib.iunet_ma_up_gate_dg_parts(3, 1, 64, 64, 64, 64) == 64


def test_bench_work_count():
    """tools/bench_manet.py's count of the attention kernels' matrix work, recounted product by product for T = 4096, Cb = 256, N = 1."""
    spec = importlib.util.spec_from_file_location('bench_manet', os.path.join(ROOT, 'tools', 'bench_manet.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    T, Cb = 4096, 256
    mac = lambda depth: 2 * T * T * depth
    fwd = 2 * mac(64) + mac(Cb)                                   # S for each of the two 128-channel blocks, P V once over all channels
    rows = 2 * (mac(64) + mac(Cb)) + mac(64)                      # (S, dP) in both passes, dKc
    cols = 2 * (mac(64) + mac(128)) + (mac(64) + mac(Cb) + mac(64))    # per dV block: S and its 128 channels; dQ: S, dP, dQ
    assert mod.attention_flops(T, Cb, 1) == (fwd, rows, cols, fwd)




# ---------------------------------------------------------------------------------------------- the network
ATTN_SCALE = 0.25      # the module's own initial scale of the query / key weights against He-normal (sqrt(1 / 2) K^(-1/4), K = 64):
                       # the logits S of He-normal weights are in the hundreds, a one-hot softmax


def _model(**kw):
    from interactive_unet.unet import UNet
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return UNet(architecture='MA-Net', pretrained=False, **kw)


# ---- an independent torch.nn MA-Net (position attention block + gated decoder blocks on the project's encoder)
def _mods(dim):
    return (nn.Conv3d, nn.BatchNorm3d) if dim == 3 else (nn.Conv2d, nn.BatchNorm2d)


class Stage(nn.Module):
    def __init__(self, ci, co, dim):
        super().__init__()
        Conv, BN = _mods(dim)
        self.conv1, self.bn1 = Conv(ci, co, 3, padding=1, bias=False), BN(co)
        self.conv2, self.bn2 = Conv(co, co, 3, padding=1, bias=False), BN(co)

    def forward(self, x):
        return torch.relu(self.bn2(self.conv2(torch.relu(self.bn1(self.conv1(x))))))


class ConvBnRelu(nn.Sequential):
    def __init__(self, ci, co, k, dim):
        super().__init__()
        Conv, BN = _mods(dim)
        self.add_module('conv', Conv(ci, co, k, padding=k // 2, bias=False))
        self.add_module('bn', BN(co))
        self.add_module('relu', nn.ReLU())


class Biased(nn.Module):
    def __init__(self, ci, co, k, dim):
        super().__init__()
        self.conv = _mods(dim)[0](ci, co, k, padding=k // 2)

    def forward(self, x):
        return self.conv(x)


class PAB(nn.Module):
    def __init__(self, c, dim):
        super().__init__()
        self.top, self.center, self.bottom = Biased(c, 64, 1, dim), Biased(c, 64, 1, dim), Biased(c, c, 3, dim)
        self.out = ConvBnRelu(c, c, 3, dim)

    def attend(self, x):
        q, k, v = (m(x).flatten(2) for m in (self.top, self.center, self.bottom))          # [N, C, T]
        a = F.softmax(torch.bmm(k.transpose(1, 2), q), dim=2)                              # a[n][i][j] over the keys' tokens i
        return torch.bmm(v, a.transpose(1, 2)).reshape(x.shape), a                          # O[c][i] = sum_j a[i][j] V[c][j]

    def forward(self, x):
        return self.out(x + self.attend(x)[0])


class SE(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(c, max(c // 16, 1)), nn.Linear(max(c // 16, 1), c)

    def forward(self, x):
        return torch.sigmoid(self.fc2(torch.relu(self.fc1(x.flatten(2).mean(2)))))


class Block(nn.Module):
    def __init__(self, ci, c, dim):
        super().__init__()
        Conv, BN = _mods(dim)
        self.hl3, self.hl1 = ConvBnRelu(ci, ci, 3, dim), ConvBnRelu(ci, c, 1, dim)
        self.se_hl, self.se_ll = SE(c), SE(c)
        self.conv1, self.bn1 = Conv(2 * c, c, 3, padding=1, bias=False), BN(c)
        self.conv2, self.bn2 = Conv(c, c, 3, padding=1, bias=False), BN(c)

    def forward(self, x, skip):
        h = self.hl1(self.hl3(x))
        g = self.se_hl(h) + self.se_ll(skip)
        u = F.interpolate(h, scale_factor=2, mode='nearest') * g.reshape(g.shape + (1,) * (x.dim() - 2))
        y = torch.relu(self.bn1(self.conv1(torch.cat([skip, u], 1))))
        return torch.relu(self.bn2(self.conv2(y)))


class TorchMANet(nn.Module):
    def __init__(self, dim=2, levels=4, base=32, cin=1, ncls=2):
        super().__init__()
        ch = [base * 2 ** l for l in range(levels)]
        self.dim, self.levels = dim, levels
        self.enc = nn.ModuleList(Stage(cin if l == 0 else ch[l - 1], ch[l], dim) for l in range(levels))
        self.pab = PAB(ch[-1], dim)
        self.dec = nn.ModuleDict({str(l): Block(ch[l + 1], ch[l], dim) for l in range(levels - 2, -1, -1)})
        self.head = _mods(dim)[0](ch[0], ncls, 1)

    def named_canonical(self):
        out = {}
        for k, v in self.state_dict().items():
            if k.endswith('num_batches_tracked'):
                continue
            parts = k.split('.')
            if parts[0] in ('enc', 'dec'):
                k = f'{parts[0]}{parts[1]}.' + '.'.join(parts[2:])
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
        h = self.pab(feats[-1])
        for l in range(self.levels - 2, -1, -1):
            h = self.dec[str(l)](h, feats[l])
        return self.head(h)


def _recount(dim, L, base, cin, ncls):
    """The parameter count from the issue's definition, written out."""
    ch = [base * 2 ** l for l in range(L)]
    k = 3 ** dim
    n = 0
    for l in range(L):
        ci = cin if l == 0 else ch[l - 1]
        n += ci * ch[l] * k + 2 * ch[l] + ch[l] * ch[l] * k + 2 * ch[l]
    Cb = ch[-1]
    n += 2 * (Cb * 64 + 64) + Cb * Cb * k + Cb                  # queries, keys, values: weight + bias
    n += Cb * Cb * k + 2 * Cb                                   # pab.out
    for l in range(L - 1):
        c, ci, m = ch[l], ch[l + 1], max(ch[l] // 16, 1)
        n += ci * ci * k + 2 * ci + ci * c + 2 * c              # hl3, hl1
        n += 2 * (m * c + m + c * m + c)                        # the two gates
        n += 2 * c * c * k + 2 * c + c * c * k + 2 * c          # the stage on concat(skip, u)
    return n + ch[0] * ncls + ncls


def test_param_names_shapes_and_counts():
    from interactive_unet import unet
    for dim in (2, 3):
        mod = TorchMANet(dim=dim)
        want = {k: tuple(v.shape) for k, v in mod.named_canonical().items()}
        shapes = unet.param_shapes(dim, 4, 32, 1, 2, architecture='MA-Net')
        assert set(shapes) == set(want) and all(shapes[k] == want[k] for k in want)
        assert list(shapes) == list(ref.param_shapes(dim, 4, 32, 1, 2)) and shapes == ref.param_shapes(dim, 4, 32, 1, 2)
        n = sum(torch.Size(v).numel() for k, v in shapes.items() if not unet._is_buffer(k))
        assert n == sum(p.numel() for p in mod.parameters()) == _recount(dim, 4, 32, 1, 2)
    m = unet.param_shapes(2, 5, 32, 2, 5, architecture='MA-Net')
    assert m == ref.param_shapes(2, 5, 32, 2, 5) and list(m) == list(ref.param_shapes(2, 5, 32, 2, 5))
    assert m['pab.top.conv.weight'] == (64, 512, 1, 1) and m['pab.center.conv.bias'] == (64,) and m['pab.bottom.conv.weight'] == (512, 512, 3, 3)
    assert m['pab.out.conv.weight'] == (512, 512, 3, 3) and 'pab.out.conv.bias' not in m and 'pab.top.bn.weight' not in m
    assert m['dec3.hl3.conv.weight'] == (512, 512, 3, 3) and m['dec3.hl1.conv.weight'] == (256, 512, 1, 1)
    assert m['dec3.se_hl.fc1.weight'] == (16, 256) and m['dec3.se_ll.fc2.weight'] == (256, 16) and m['dec0.se_hl.fc1.weight'] == (2, 32)
    assert m['dec0.conv1.weight'] == (32, 64, 3, 3) and m['head.weight'] == (5, 32, 1, 1) and 'dec4.hl3.conv.weight' not in m
    order = ['enc4.bn2.running_var', 'pab.top.conv.weight', 'pab.center.conv.weight', 'pab.bottom.conv.weight', 'pab.out.conv.weight',
             'dec3.hl3.conv.weight', 'dec3.hl1.conv.weight', 'dec3.se_hl.fc1.weight', 'dec3.se_ll.fc1.weight', 'dec3.conv1.weight',
             'dec3.bn1.weight', 'dec3.conv2.weight', 'dec3.bn2.weight', 'dec2.hl3.conv.weight', 'dec0.bn2.running_var', 'head.weight']
    names = list(m)
    assert [names.index(k) for k in order] == sorted(names.index(k) for k in order)


@pytest.mark.parametrize('dim,shape,levels', [(2, (2, 1, 48, 80), 4), (3, (2, 2, 16, 8, 24), 4), (2, (1, 3, 32, 48), 3), (3, (2, 1, 8, 16, 16), 3)])
def test_reference_equals_torch_module(dim, shape, levels):
    cin = shape[1]
    mod = TorchMANet(dim=dim, levels=levels, base=32, cin=cin, ncls=3).double()
    p = ref.init_params(dim, levels, 32, cin, 3, seed=2, randomize_bn=True, attn_scale=ATTN_SCALE)
    assert p['pab.bottom.conv.bias'].abs().max() > 0 and p['dec0.se_ll.fc2.bias'].abs().max() > 0
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
    for bn, m in (('pab.out.bn', mod.pab.out.bn), ('dec0.hl1.bn', mod.dec['0'].hl1.bn), ('dec0.bn2', mod.dec['0'].bn2)):
        mean, var = stats[bn]
        assert torch.allclose(m.running_mean, 0.9 * p[bn + '.running_mean'].double() + 0.1 * mean)
        assert torch.allclose(m.running_var, 0.9 * p[bn + '.running_var'].double() + 0.1 * var)


def test_attention_rows_sum_to_one():
    """In the reference (float64 and with P rounded for the second product) and in the independent module; the softmax is neither flat nor
    one-hot for these parameters."""
    p = ref.init_params(2, 4, 32, 1, 2, seed=3, randomize_bn=True, attn_scale=ATTN_SCALE)
    x = torch.rand((2, 1, 40, 24), dtype=torch.float64)
    for act in (torch.float16, torch.bfloat16, None):
        keep = {}
        ref.forward_logits(p, x, 2, 4, act=act, keep=keep)
        assert keep['A'].shape == (2, 15, 15) and (keep['A'].sum(2) - 1).abs().max().item() <= 1e-12
    mod = TorchMANet(levels=4).double().eval()
    mod.load_canonical({k: v.double() for k, v in p.items()})
    with torch.no_grad():
        h = x
        for l, st in enumerate(mod.enc):
            h = st(F.max_pool2d(h, 2) if l else h)
        a = mod.pab.attend(h)[1]
    assert a.shape == (2, 15, 15) and (a.sum(2) - 1).abs().max().item() <= 1e-12
    assert (a - keep['A']).abs().max().item() <= 1e-12            # (the float64 run's weights)
    top = a.max(2).values
    print(f'largest weight of a row: {top.min().item():.3f} .. {top.max().item():.3f}')
    assert 1.5 / 15 < top.median().item() < 0.95


def test_batch_one_trains_in_the_reference():
    p = ref.init_params(2, 4, 32, 1, 2, seed=1)
    y = ref.forward_logits(p, torch.rand((1, 1, 32, 32), dtype=torch.float64), 2, 4, training=True)
    assert y.shape == (1, 2, 32, 32) and bool(torch.isfinite(y).all())


def test_rounded_reference_stays_close():
    """(the parameters of the GPU suite's forward cases)"""
    p = ref.init_params(2, 4, 32, 1, 3, seed=11, randomize_bn=True, attn_scale=ATTN_SCALE)
    x = torch.rand((1, 1, 40, 24), dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    base = torch.softmax(ref.forward_logits(p, x, 2, 4), 1)
    for T, gate in ((torch.float16, 5e-3), (torch.bfloat16, 3e-2)):
        assert (torch.softmax(ref.forward_logits(p, x, 2, 4, act=T), 1) - base).abs().max().item() <= gate


def test_constructor_hparams_and_init():
    m = _model(num_classes=3)
    assert m.architecture == 'MA-Net' and m.act_dtype == torch.float16 and m.infer_dtype == torch.float32
    assert not any(k.startswith('decoder') for k in m.hparams) and m.decoder_channels is None
    t = m.named_tensors()
    assert list(t) == list(ref.param_shapes(2, 4, 32, 1, 3))
    for k in ('pab.top.conv.weight', 'pab.center.conv.weight', 'pab.bottom.conv.weight', 'pab.out.conv.weight', 'dec2.hl3.conv.weight',
              'dec0.conv1.weight'):
        std = math.sqrt(2.0 / (t[k].shape[1] * math.prod(t[k].shape[2:])))
        if k.startswith(('pab.top.', 'pab.center.')):      # unit gain x K^(-1/4): the reference's attn_scale on He-normal weights
            std *= ATTN_SCALE
        assert abs(t[k].std().item() - std) < 0.1 * std, k
    assert t['dec2.se_hl.fc1.weight'].abs().max() > 0 and t['dec0.se_ll.fc2.weight'].abs().max() > 0
    assert torch.equal(t['pab.out.bn.weight'], torch.ones(256)) and torch.equal(t['pab.center.conv.bias'], torch.zeros(64))
    assert torch.equal(t['dec1.se_ll.fc2.bias'], torch.zeros(64)) and torch.equal(t['dec1.bn2.weight'], torch.ones(64))
    assert _model(infer_dtype='bf16').infer_dtype == torch.bfloat16
    assert _model(levels=5, encoder_name='resnet34').tensor('pab.top.conv.weight').shape == (64, 512, 1, 1)
    assert _model(levels=3, base=64, dim=3).tensor('pab.bottom.conv.weight').shape == (256, 256, 3, 3, 3)


def test_menu_and_other_architectures_unchanged():
    """'MA-Net' joins the menu; 'FPN', 'PSPNet', 'DeepLabV3+' and 'PAN' stay refused; no other architecture's hparams moved."""
    from interactive_unet import unet
    assert unet.ARCHITECTURES[-1] == 'MA-Net' and set(unet.ARCHITECTURES[:-1]) == {'U-Net', 'U-Net++', 'LinkNet', 'DeepLabV3', 'Segformer', 'UPerNet'}
    common = {'lr', 'num_channels', 'num_classes', 'loss_function', 'architecture', 'encoder_name', 'pretrained', 'dim', 'levels', 'base', 'act_dtype',
              'weight_dtype', 'norm', 'groups', 'infer_dtype', 'act_quant', 'infer_policy'}
    extra = {'DeepLabV3': {'decoder_channels', 'decoder_atrous_rates', 'decoder_aspp_dropout'}, 'UPerNet': {'decoder_channels'},
             'Segformer': {'decoder_segmentation_channels'}}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for arch in unet.ARCHITECTURES:
            assert set(unet.UNet(architecture=arch, pretrained=False).hparams) == common | extra.get(arch, set()), arch
        for arch in ('FPN', 'PSPNet', 'DeepLabV3+', 'PAN', 'manet', 'MANet'):
            with pytest.raises(NotImplementedError):
                unet.UNet(architecture=arch, pretrained=False)


@pytest.mark.parametrize('kw', [dict(norm='group'), dict(weight_dtype='fp8_e4m3'), dict(act_dtype='fp32'), dict(act_dtype='fp16x2'),
                                dict(infer_dtype='fp16x2'), dict(infer_policy='x2m'), dict(levels=2), dict(levels=6), dict(base=48),
                                dict(num_channels=5), dict(num_classes=11), dict(base=64, levels=5)])
def test_refusals(kw):
    with pytest.raises(NotImplementedError, match='MA-Net supports'):
        _model(**kw)


def test_process_group_refused_before_gpu_work():
    from interactive_unet.train_engine_f32 import make_train_engine
    m = _model()
    with pytest.raises(NotImplementedError, match='process_group'):
        make_train_engine(m, process_group=object())


def test_checkpoint_round_trip(tmp_path):
    from interactive_unet.unet import UNet
    m = _model(dim=3, levels=3, num_classes=4, num_channels=2)
    m.load_named(ref.init_params(3, 3, 32, 2, 4, seed=4, randomize_bn=True))
    path = tmp_path / 'model.ckpt'
    m.save_checkpoint(str(path))
    r = UNet.load_from_checkpoint(checkpoint_path=str(path))
    assert r.architecture == 'MA-Net' and r.dim == 3 and r.levels == 3 and r.hparams == m.hparams
    for k, v in m.named_tensors().items():
        assert torch.equal(v, r.tensor(k)), k


def test_engine_needs_the_gpu():
    with pytest.raises(RuntimeError):
        _model().engine('eval')
