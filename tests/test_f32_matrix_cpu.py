"""The case tables of tests/test_gpu_f32_matrix.py without a GPU.

  * Every body of that file runs once per case against a stub binding: the operands are built on the CPU, each call is checked
    against the prototype in include/iunet.h (argument count, and every argument through the ctypes type the binding derives), nothing
    is launched, and the assertions on the device's results are muted.  What remains are the file's plain asserts: every integer
    reference below 2^24, the tie shares, the 1 % and 0.5-margin conditions, the regime each case's id names, and the restated launch
    arithmetic against the library's host functions.  A table edit that leaves a regime, or a signature slip, fails here.
  * The arithmetic the read-back cases rest on, restated in plain torch: the conv of the delta input returns the operator; each
    operation of the BatchNorm fold is correctly rounded.
  * The arguments every fp32 entry point refuses with -1 instead of a launch."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tests.test_gpu_f32_matrix as M


@pytest.fixture(scope='module')
def nv():
    from interactive_unet import _native
    if not os.path.isfile(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    _native.lib()
    return _native


# ---------------------------------------------------------------------------------------------------------------- the stubbed run
class StubBinding:
    """interactive_unet._native with call() replaced by a check of the call against include/iunet.h; the host-only functions of lib() stay real."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        return getattr(self.real, name)

    def stream(self):
        return None

    def call(self, name, *args):
        restype, argtypes = self.real.signatures()[name]
        assert len(args) == len(argtypes), f'{name}: {len(args)} arguments, the header declares {len(argtypes)}'
        for k, (a, t) in enumerate(zip(args, argtypes)):
            try:
                t.from_param(a)
            except (TypeError, ctypes.ArgumentError) as e:
                raise AssertionError(f'{name}: argument {k} ({a!r}) is no {t.__name__}: {e}') from None
        self.calls.append(name)


def cases(fn):
    """The keyword arguments of every parametrised case of a test function."""
    sets = []
    for mark in getattr(fn, 'pytestmark', []):
        if mark.name != 'parametrize':
            continue
        names = [n.strip() for n in mark.args[0].split(',')]
        rows = []
        for v in mark.args[1]:
            vals = v.values if hasattr(v, 'values') else v if len(names) > 1 else (v,)
            assert len(vals) == len(names), (fn.__name__, names, vals)
            rows.append(dict(zip(names, vals)))
        sets.append(rows)
    return [dict(kv for d in combo for kv in d.items()) for combo in itertools.product(*sets)]


BODIES = sorted(k for k, v in vars(M).items() if k.startswith('test_') and callable(v))
ENTRY_POINTS = {'iunet_f32_conv_fwd', 'iunet_f32_pack_conv', 'iunet_f32_maxpool_fwd', 'iunet_f32_maxpool_bwd', 'iunet_f32_head_fwd', 'iunet_f32_head_loss_fwd',
                'iunet_f32_head_loss_bwd', 'iunet_f32_channel_sum', 'iunet_check_finite', 'iunet_div_f32', 'iunet_f32_wgrad', 'iunet_reduce_slab',
                'iunet_f32_bn_stats', 'iunet_f32_bn_relu_fwd', 'iunet_f32_bn_relu_bwd'}
SEEN = set()


@pytest.mark.parametrize('name', BODIES)
def test_gpu_bodies_against_the_header(nv, monkeypatch, name):
    monkeypatch.setattr(M, 'DEVICE', 'cpu')
    monkeypatch.setattr(M, 'verify', lambda cond, msg='': None)
    stub = StubBinding(nv)
    fn = getattr(M, name)
    rows = cases(fn)
    assert rows
    for kw in rows:
        fn(stub, **kw)
    assert stub.calls, f'{name} calls no entry point'
    SEEN.update(stub.calls)


def test_every_entry_point_of_the_issue_is_called():
    assert len(BODIES) >= 20
    if len(SEEN):          # filled by the test above (same process); a -k selection of this test alone has nothing to say
        assert SEEN == ENTRY_POINTS, SEEN ^ ENTRY_POINTS


def test_case_ids_are_unique_and_name_their_regime():
    for name in BODIES:
        for mark in getattr(getattr(M, name), 'pytestmark', []):
            ids = [v.id for v in mark.args[1] if hasattr(v, 'values') and v.id]
            assert len(ids) == len(set(ids)), (name, [i for i in ids if ids.count(i) > 1])
    for p in M.WGRAD:
        assert p.values[-1] in p.id
    for p in M.CONV0:
        assert M.chunk_name(p.values[1]) in p.id and p.values[3] in p.id


# ---------------------------------------------------------------------------------------------------------------- launch arithmetic
def test_restated_formulas_against_the_host_functions(nv):
    lib = nv.lib()
    for nd, grid in ((2, (18, 20)), (2, (1, 2341)), (2, (40, 60)), (2, (256, 256)), (3, (5, 6, 18)), (3, (16, 16, 64)), (3, (1, 1, 1))):
        D, H, W = M.dhw(nd, grid)
        for N in (1, 3, 4):
            for cin, cout in ((1, 32), (12, 40), (40, 3), (64, 64), (256, 64), (16, 32), (512, 512), (2048, 64)):
                assert lib.iunet_f32_wgrad_splits(nd, N, D, H, W, cin, cout) == M.wgrad_splits(nd, N, grid, cin, cout) >= 1
    assert lib.iunet_f32_wgrad_splits(4, 1, 1, 8, 8, 8, 8) == 0 and lib.iunet_f32_wgrad_splits(2, 1, 1, 8, 0, 8, 8) == 0
    for N in (1, 3):
        for vox in (1, 7, 285, 2047, 2048, 2049, 2341, 4096, 1 << 20):
            assert lib.iunet_f32_head_loss_num_parts(N, vox) == M.head_loss_parts(N, vox)
    for cout, cin, taps in ((32, 1, 9), (64, 12, 27), (32, 96, 1), (64, 64, 8), (32, 3, 4)):
        assert lib.iunet_f32_pack_conv_elems(cout, cin, taps) == M.pack_elems(cout, cin, taps)
    assert lib.iunet_f32_pack_conv_elems(48, 8, 9) == 0
    assert {M.reduce_branch(p, n) for _, p, n in M.REDUCE} == {'plain', 'tree', 'fold'}
    assert {M.wgrad_regime(*p.values[:5]) for p in M.WGRAD} == {'splits_eq_tiles', 'splits_eq_1024_per_blocks', 'splits_eq_cap256'}


# ---------------------------------------------------------------------------------------------------------------- read-back arithmetic
@pytest.mark.parametrize('nd', [2, 3])
def test_delta_input_returns_the_operator(nd):
    g = M.gen(nd)
    w = torch.randn((32, 3) + (3,) * nd, generator=g)
    got = M.conv_nd(nd)(M.delta_input(nd, M.GRID[nd]), w, padding=1)
    assert torch.equal(got, M.delta_conv_expected(nd, w))
    wt = torch.randn((3, 32) + (2,) * nd, generator=g)
    got = (F.conv_transpose2d if nd == 2 else F.conv_transpose3d)(M.delta_input(nd, M.TGRID[nd]), wt, stride=2)
    assert torch.equal(got, M.delta_convT_expected(nd, wt))


def half_ulp(got32, exact64):
    ulp = torch.tensor(np.spacing(got32.abs().numpy()).astype(np.float64))
    return bool(((got32.double() - exact64).abs() <= 0.5 * ulp).all())


def test_fold_operations_are_each_correctly_rounded():
    """fold_ref's five fp32 operations, each against the same operation in float64 on the same fp32 operands: within half a unit."""
    g = M.gen(5)
    gamma, beta, mean, var = M.bn_vectors(g, 64)
    w = torch.randn(64, 3, 27, generator=g)
    eps = torch.tensor(1e-5, dtype=torch.float32)
    s = var + eps
    r = M.sqrt_rn(s)
    assert torch.equal(r, torch.from_numpy(np.sqrt(s.numpy())))
    a = gamma / r
    assert half_ulp(s, var.double() + eps.double()) and half_ulp(r, torch.sqrt(s.double())) and half_ulp(a, gamma.double() / r.double())
    wf, bias = M.fold_ref(w, (gamma, beta, mean, var), 1e-5, 0)
    assert half_ulp(wf, w.double() * a.double().view(-1, 1, 1))
    ma = mean * a
    assert half_ulp(ma, mean.double() * a.double()) and half_ulp(bias, beta.double() - ma.double()) and torch.equal(bias, beta - ma)
    wt = torch.randn(3, 64, 8, generator=g)
    assert torch.equal(M.fold_ref(wt, (gamma, beta, mean, var), 1e-5, 1)[0], wt * a.view(1, -1, 1))


def test_u8_quotient_and_first_maximum_on_the_cpu():
    """What the exact rows take from torch on the CPU: uint8.float() / 255 is the correctly rounded quotient for all 256 bytes, and
    max-pool backward routes to the first maximum in scan order under ties."""
    b = torch.arange(256, dtype=torch.uint8)
    assert half_ulp(b.float() / 255, b.double() / 255)
    for nd in (2, 3):
        z = torch.zeros((1, 1) + (2,) * nd, requires_grad=True)          # one window, all tied
        M.pool_nd(nd)(z, 2).backward(torch.ones((1, 1) + (1,) * nd))
        assert z.grad.reshape(-1).tolist() == [1.0] + [0.0] * (2 ** nd - 1)


# ---------------------------------------------------------------------------------------------------------------- refused arguments
def test_entry_points_check_their_arguments(nv):
    """Every row violates one documented precondition and is answered with -1 (IUNET_ERR_ARG) before anything is launched."""
    lib = nv.lib()
    ok = ctypes.c_void_p(16)
    st = nv.ll_array([64, 64, 64, 8, 1])
    bad = [
        # iunet_f32_pack_conv(w, dst, bias_out, gamma, beta, mean, var, eps, Cout, Cin, taps, transposed, stream)
        ('iunet_f32_pack_conv', (ok, ok, None, None, None, None, None, 1e-5, 48, 8, 9, 0, None)),          # Cout = 48
        ('iunet_f32_pack_conv', (ok, ok, None, None, None, None, None, 1e-5, 32, 8, 5, 0, None)),          # taps = 5
        ('iunet_f32_pack_conv', (ok, ok, None, None, None, None, None, 1e-5, 32, 8, 9, 1, None)),          # transposed taps = 9
        ('iunet_f32_pack_conv', (ok, ok, None, ok, ok, ok, ok, 1e-5, 32, 8, 9, 0, None)),                  # a fold without bias_out
        ('iunet_f32_pack_conv', (None, ok, None, None, None, None, None, 1e-5, 32, 8, 9, 0, None)),
        ('iunet_f32_pack_conv', (ok, ok, None, None, None, None, None, 1e-5, 32, 0, 9, 0, None)),
        # iunet_f32_conv_fwd(nd, x, in_dtype, in_strides, y, y_ss, wpk, bias, N, D, H, W, Cin, Cout, relu, transposed, stream)
        ('iunet_f32_conv_fwd', (4, ok, 0, st, ok, 64, ok, None, 1, 1, 8, 8, 8, 32, 0, 0, None)),           # nd = 4
        ('iunet_f32_conv_fwd', (2, ok, 0, st, ok, 64, ok, None, 1, 1, 8, 8, 8, 48, 0, 0, None)),           # Cout = 48
        ('iunet_f32_conv_fwd', (2, ok, 4, st, ok, 64, ok, None, 1, 1, 8, 8, 8, 32, 0, 0, None)),           # in_dtype = 4
        ('iunet_f32_conv_fwd', (2, ok, 0, st, ok, 64, ok, None, 1, 2, 8, 8, 8, 32, 0, 0, None)),           # 2-D with D = 2
        ('iunet_f32_conv_fwd', (2, ok, 0, st, ok, 64, ok, None, 1, 1, 8, 8, 8, 32, 0, 3, None)),           # transposed = 3
        ('iunet_f32_conv_fwd', (3, ok, 0, st, ok, 64, ok, None, 1, 8, 8, 8, 8, 32, 0, -1, None)),
        ('iunet_f32_conv_fwd', (2, None, 0, st, ok, 64, ok, None, 1, 1, 8, 8, 8, 32, 0, 0, None)),
        ('iunet_f32_conv_fwd', (2, ok, 0, None, ok, 64, ok, None, 1, 1, 8, 8, 8, 32, 0, 0, None)),
        ('iunet_f32_conv_fwd', (2, ok, 0, st, ok, 64, ok, None, 1, 1, 8, 0, 8, 32, 0, 0, None)),           # W = 0
        ('iunet_f32_conv_fwd', (2, ok, 0, st, ok, 64, ok, None, 0, 1, 8, 8, 8, 32, 0, 0, None)),
        # iunet_f32_maxpool_fwd(nd, x, x_ss, y, y_ss, C, N, Do, Ho, Wo, stream)
        ('iunet_f32_maxpool_fwd', (4, ok, 64, ok, 64, 3, 1, 1, 4, 4, None)),
        ('iunet_f32_maxpool_fwd', (2, ok, 64, None, 64, 3, 1, 1, 4, 4, None)),
        ('iunet_f32_maxpool_fwd', (2, ok, 64, ok, 64, 3, 1, 1, 0, 4, None)),
        # iunet_f32_head_fwd(x, x_ss, C0, w, bias, ncls, logits, probs, cls, out_strides, divisor, accumulate, N, D, H, W, stream)
        ('iunet_f32_head_fwd', (ok, 64, 32, ok, ok, 1, ok, ok, ok, st, 1.0, 0, 1, 1, 8, 8, None)),          # ncls = 1
        ('iunet_f32_head_fwd', (ok, 64, 32, ok, ok, 11, ok, ok, ok, st, 1.0, 0, 1, 1, 8, 8, None)),         # ncls = 11
        ('iunet_f32_head_fwd', (ok, 64, 32, ok, ok, 2, None, None, None, st, 1.0, 0, 1, 1, 8, 8, None)),    # no output
        ('iunet_f32_head_fwd', (ok, 64, 32, ok, ok, 2, ok, ok, ok, st, 0.0, 0, 1, 1, 8, 8, None)),          # divisor = 0
        ('iunet_f32_head_fwd', (ok, 64, 0, ok, ok, 2, ok, ok, ok, st, 1.0, 0, 1, 1, 8, 8, None)),           # C0 = 0
        ('iunet_f32_head_fwd', (ok, 64, 32, ok, ok, 2, ok, ok, ok, st, 1.0, 0, 0, 1, 8, 8, None)),          # N = 0
        ('iunet_f32_head_fwd', (ok, 64, 32, ok, ok, 2, ok, ok, ok, st, 1.0, 0, 1, 0, 8, 8, None)),
        ('iunet_f32_head_fwd', (ok, 64, 32, ok, ok, 2, ok, ok, ok, st, 1.0, 0, 1, 1, -8, 8, None)),
        ('iunet_f32_head_fwd', (ok, 64, 32, ok, ok, 2, ok, ok, ok, st, 1.0, 0, 1, 1, 8, 0, None)),
        ('iunet_f32_head_fwd', (None, 64, 32, ok, ok, 2, ok, ok, ok, st, 1.0, 0, 1, 1, 8, 8, None)),
        ('iunet_f32_head_fwd', (ok, 64, 32, ok, None, 2, ok, ok, ok, st, 1.0, 0, 1, 1, 8, 8, None)),
        ('iunet_f32_head_fwd', (ok, 64, 32, ok, ok, 2, ok, ok, ok, None, 1.0, 0, 1, 1, 8, 8, None)),
        # iunet_f32_bn_stats(y, y_ss, C, N, vox, eps, momentum, mean, stdv, run_mean, run_var, stream)
        ('iunet_f32_bn_stats', (ok, 64, 3, 1, 8, 1e-5, 0.1, ok, ok, ok, None, None)),                      # one running vector only
        ('iunet_f32_bn_stats', (ok, 64, 3, 1, 8, 1e-5, 0.1, ok, ok, None, ok, None)),
        ('iunet_f32_bn_stats', (None, 64, 3, 1, 8, 1e-5, 0.1, ok, ok, None, None, None)),
        ('iunet_f32_bn_stats', (ok, 64, 3, 1, 8, 1e-5, 0.1, ok, None, None, None, None)),
        ('iunet_f32_bn_stats', (ok, 64, 3, 1, 0, 1e-5, 0.1, ok, ok, None, None, None)),
        ('iunet_f32_bn_stats', (ok, 64, 0, 1, 8, 1e-5, 0.1, ok, ok, None, None, None)),
        # iunet_f32_bn_relu_fwd(y, y_ss, z, z_ss, mean, stdv, gamma, beta, C, N, vox, stream)
        ('iunet_f32_bn_relu_fwd', (ok, 64, None, 64, ok, ok, ok, ok, 3, 1, 8, None)),
        ('iunet_f32_bn_relu_fwd', (ok, 64, ok, 64, ok, ok, ok, None, 3, 1, 8, None)),
        ('iunet_f32_bn_relu_fwd', (ok, 64, ok, 64, ok, ok, ok, ok, 3, 0, 8, None)),
        ('iunet_f32_bn_relu_fwd', (ok, 64, ok, 64, ok, ok, ok, ok, 3, 1, 0, None)),
        # iunet_f32_bn_relu_bwd(dz, dz_ss, y, y_ss, dy, dy_ss, mean, stdv, gamma, beta, dgamma, dbeta, C, N, vox, stream)
        ('iunet_f32_bn_relu_bwd', (None, 64, ok, 64, ok, 64, ok, ok, ok, ok, ok, ok, 3, 1, 8, None)),
        ('iunet_f32_bn_relu_bwd', (ok, 64, ok, 64, ok, 64, ok, ok, ok, ok, ok, None, 3, 1, 8, None)),
        ('iunet_f32_bn_relu_bwd', (ok, 64, ok, 64, ok, 64, ok, ok, ok, ok, ok, ok, 0, 1, 8, None)),
        ('iunet_f32_bn_relu_bwd', (ok, 64, ok, 64, ok, 64, ok, ok, ok, ok, ok, ok, 3, 1, 0, None)),
        # iunet_f32_maxpool_bwd(nd, z, z_ss, dpool, dp_ss, dz, dz_ss, C, N, Do, Ho, Wo, accumulate, stream)
        ('iunet_f32_maxpool_bwd', (4, ok, 64, ok, 64, ok, 64, 3, 1, 1, 4, 4, 0, None)),
        ('iunet_f32_maxpool_bwd', (2, ok, 64, None, 64, ok, 64, 3, 1, 1, 4, 4, 0, None)),
        ('iunet_f32_maxpool_bwd', (2, ok, 64, ok, 64, ok, 64, 3, 1, 1, 4, 0, 0, None)),
        ('iunet_f32_maxpool_bwd', (3, ok, 64, ok, 64, ok, 64, 0, 1, 1, 4, 4, 0, None)),
        # iunet_f32_wgrad(nd, x, x_ss, dy, dy_ss, slab, N, D, H, W, Cin, Cout, taps, stream)
        ('iunet_f32_wgrad', (4, ok, 64, ok, 64, ok, 1, 1, 8, 8, 8, 8, 9, None)),
        ('iunet_f32_wgrad', (2, ok, 64, ok, 64, ok, 1, 1, 8, 8, 8, 8, 5, None)),                           # taps = 5
        ('iunet_f32_wgrad', (2, ok, 64, ok, 64, ok, 1, 1, 8, 8, 8, 8, 27, None)),
        ('iunet_f32_wgrad', (2, ok, 64, ok, 64, ok, 1, 2, 8, 8, 8, 8, 9, None)),                           # 2-D with D = 2
        ('iunet_f32_wgrad', (2, ok, 64, ok, 64, None, 1, 1, 8, 8, 8, 8, 9, None)),
        ('iunet_f32_wgrad', (2, ok, 64, ok, 64, ok, 1, 1, 8, 0, 8, 8, 9, None)),
        ('iunet_f32_wgrad', (2, ok, 64, ok, 64, ok, 1, 1, 8, 8, 0, 8, 9, None)),
        # iunet_f32_head_loss_fwd(x, x_ss, C0, w, bias, ncls, target, weight, tdtype, kind, slab, out4, coef, N, vox, stream)
        ('iunet_f32_head_loss_fwd', (ok, 64, 32, ok, ok, 1, ok, None, 0, 0, ok, ok, ok, 1, 8, None)),      # ncls = 1
        ('iunet_f32_head_loss_fwd', (ok, 64, 32, ok, ok, 11, ok, None, 0, 0, ok, ok, ok, 1, 8, None)),     # ncls = 11
        ('iunet_f32_head_loss_fwd', (ok, 64, 32, ok, ok, 2, ok, None, 2, 0, ok, ok, ok, 1, 8, None)),      # tdtype = 2
        ('iunet_f32_head_loss_fwd', (ok, 64, 32, ok, ok, 2, ok, None, 0, 7, ok, ok, ok, 1, 8, None)),      # kind = 7
        ('iunet_f32_head_loss_fwd', (ok, 64, 32, ok, ok, 2, None, None, 0, 0, ok, ok, ok, 1, 8, None)),
        ('iunet_f32_head_loss_fwd', (ok, 64, 32, ok, ok, 2, ok, None, 0, 0, ok, ok, ok, 1, 0, None)),
        ('iunet_f32_head_loss_fwd', (ok, 64, 0, ok, ok, 2, ok, None, 0, 0, ok, ok, ok, 1, 8, None)),
        # iunet_f32_head_loss_bwd(x, x_ss, C0, w, bias, ncls, target, weight, tdtype, coef, dlogits, dl_ss, dx, dx_ss, N, vox, stream)
        ('iunet_f32_head_loss_bwd', (ok, 64, 32, ok, ok, 1, ok, None, 0, ok, ok, 64, ok, 64, 1, 8, None)),
        ('iunet_f32_head_loss_bwd', (ok, 64, 32, ok, ok, 11, ok, None, 0, ok, ok, 64, ok, 64, 1, 8, None)),
        ('iunet_f32_head_loss_bwd', (ok, 64, 32, ok, ok, 2, ok, None, 2, ok, ok, 64, ok, 64, 1, 8, None)),
        ('iunet_f32_head_loss_bwd', (ok, 64, 32, ok, ok, 2, ok, None, 0, None, ok, 64, ok, 64, 1, 8, None)),
        ('iunet_f32_head_loss_bwd', (ok, 64, 32, ok, ok, 2, ok, None, 0, ok, ok, 64, None, 64, 1, 8, None)),
        ('iunet_f32_head_loss_bwd', (ok, 64, 32, ok, ok, 2, ok, None, 0, ok, ok, 64, ok, 64, 0, 8, None)),
        # iunet_f32_channel_sum(t, t_ss, out, C, N, vox, stream)
        ('iunet_f32_channel_sum', (None, 64, ok, 3, 1, 8, None)),
        ('iunet_f32_channel_sum', (ok, 64, None, 3, 1, 8, None)),
        ('iunet_f32_channel_sum', (ok, 64, ok, 0, 1, 8, None)),
        ('iunet_f32_channel_sum', (ok, 64, ok, 3, 1, 0, None)),
        # iunet_div_f32(p, n, d, stream); iunet_check_finite(g, n, flag, stream); iunet_reduce_slab(slab, nparts, n, out, alpha, accumulate, stream)
        ('iunet_div_f32', (None, 8, 3.0, None)),
        ('iunet_div_f32', (ok, 0, 3.0, None)),
        ('iunet_check_finite', (None, 8, ok, None)),
        ('iunet_check_finite', (ok, 8, None, None)),
        ('iunet_check_finite', (ok, -1, ok, None)),
        ('iunet_reduce_slab', (None, 4, 8, ok, 1.0, 0, None)),
        ('iunet_reduce_slab', (ok, 4, 8, None, 1.0, 0, None)),
    ]
    for name, args in bad:
        assert getattr(lib, name)(*args) == -1, (name, args, lib.iunet_last_error())
    assert {name for name, _ in bad} == ENTRY_POINTS
    assert lib.iunet_check_finite(ok, 0, ok, None) == 0          # n = 0: nothing to look at, nothing launched
