"""The case tables of tests/test_gpu_x2_matrix.py without a GPU (the layout of tests/test_f32_matrix_cpu.py).

  * Every body of that file runs once per case against a stub binding: the operands are built on the CPU, each call is checked against the
    prototype in include/iunet.h (argument count, and every argument through the ctypes type the binding derives), nothing is launched, and the
    assertions on the device's results are muted.  What remains are the file's plain asserts: the exactness conditions of the data
    (tests/contract_data.py), the tie shares of the pool data, the regime each case's id names, unique ids.
  * The restated launch arithmetic against the library's host functions where they report the same numbers: the slot table through
    iunet_conv3_stats_parts, kc through iunet_x2_convT_kc, the slab size through iunet_gn_precise_slab_bytes.  brick_shape, the slot groups
    and the `small` rule are held to iunet_conv3_sample_stats_rows in the GPU file (test_restated_launch_arithmetic_against_the_library: that
    host function asks the runtime for the current device and answers 0 without one).  A restatement ONLY, with no host function to hold
    it to: the `small` rule WITHOUT the Cout factor (the fused head), that launch_x2m has no slot groups in 3-D, and nchunks / cap / the grid
    of the transposed conv.
  * The e4m3 interval rule and the 24-bit pool key on the CPU codec.
  * The arguments these entry points refuse with -1 instead of a launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import tests.test_gpu_x2_matrix as M
from tests import contract_data as cd
from tests.test_f32_matrix_cpu import StubBinding, cases


@pytest.fixture(scope='module')
def nv():
    from interactive_unet import _native
    if not os.path.isfile(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    _native.lib()
    return _native


BODIES = sorted(k for k, v in vars(M).items() if k.startswith('test_') and callable(v))
ENTRY_POINTS = {'iunet_x2m_conv_fwd', 'iunet_x2_conv3_fwd_flag', 'iunet_x2m_conv_pool_fwd', 'iunet_x2m_conv_head_fwd', 'iunet_x2_head_fwd',
                'iunet_x2_maxpool_fwd', 'iunet_x2m_maxpool_fwd', 'iunet_x2m_make8', 'iunet_x2_first_conv_fwd', 'iunet_x2m_first_conv_fwd',
                'iunet_x2_convT_fwd', 'iunet_x2m_convT_fwd', 'iunet_x2_gn_relu_fwd', 'iunet_x2m_gn_relu_fwd', 'iunet_x2m_first_stage_fwd'}
PREPARATION = {'iunet_x2_prep', 'iunet_x2m_prep_nd', 'iunet_pack_conv3', 'iunet_pack_convT', 'iunet_pack_first_conv'}
SEEN = set()


@pytest.mark.parametrize('name', BODIES)
def test_gpu_bodies_against_the_header(nv, monkeypatch, name):
    monkeypatch.setattr(M, 'DEVICE', 'cpu')
    monkeypatch.setattr(M, 'verify', lambda cond, msg='': None)
    stub = StubBinding(nv)
    fn = getattr(M, name)
    rows = cases(fn) or [{}]
    for kw in rows:
        fn(stub, **kw)
    assert stub.calls or name == 'test_restated_launch_arithmetic_against_the_library', f'{name} calls no entry point'
    SEEN.update(stub.calls)


def test_every_entry_point_of_the_issue_is_called():
    assert len(BODIES) >= 18
    if len(SEEN):          # filled by the test above (same process); a -k selection of this test alone has nothing to say
        assert SEEN == ENTRY_POINTS | PREPARATION, SEEN ^ (ENTRY_POINTS | PREPARATION)


def test_case_ids_are_unique_and_name_their_regime():
    for name in BODIES:
        for mark in getattr(getattr(M, name), 'pytestmark', []):
            if mark.name != 'parametrize':
                continue
            ids = [v.id for v in mark.args[1] if hasattr(v, 'values') and v.id]
            assert len(ids) == len(mark.args[1]) and len(ids) == len(set(ids)), (name, [i for i in ids if ids.count(i) > 1])
    for p in M.X2M_3D + M.X2_3D:
        assert ('small_tile' if p.values[4] else 'big_tile') in p.id
    for p in M.X2M_POOL:
        assert p.values[5] is None or ('small_tile' if p.values[5] else 'big_tile') in p.id
    for p in M.X2M_2D:
        assert f'N{p.values[0]}-' in p.id + '-' and (f'groups{p.values[6]}' in p.id or p.values[6] == 1)
    for p in M.CONVT:
        assert ('resident' if p.values[5][1] == 1 else 'streamed') in p.id and ('capped' in p.id) == p.values[6]
    assert {p.values[5] for p in M.CONVT} == {(1, 1), (2, 1), (1, 3), (2, 2)}
    assert {(p.values[0], p.values[1], p.values[2]) for p in M.FIRST} == {(nd, c, d) for nd in (2, 3) for c in (1, 2, 3, 4) for d in M.IN_DTYPES}


# ---------------------------------------------------------------------------------------------------------------- launch arithmetic
def test_restated_formulas_against_the_host_functions(nv):
    lib = nv.lib()
    for ncob in (1, 2, 3, 4, 8):
        assert lib.iunet_conv3_stats_parts(3, 1, 8, 8, 8, 32 * ncob, 2) == lib.iunet_conv3_stats_parts(2, 1, 1, 8, 8, 32 * ncob, 2) == M.slot_table(ncob)
    for cin in (32, 64, 96, 128, 160, 256):
        assert lib.iunet_x2_convT_kc(cin) == M.regimeT(2, 1, (4, 16), cin, 32)['kc']
    for N, C, vox in ((2, 32, 315), (1, 256, 64), (2, 32, 20001), (1, 8, 8192), (1, 8, 8193), (1, 8, 1 << 23)):
        assert lib.iunet_gn_precise_slab_bytes(N, C, vox) == N * C * min(max(M.ceil(vox, 8192), 1), 512) * 16


# ---------------------------------------------------------------------------------------------------------------- the codec rules
def test_interval_rule_on_the_cpu_codec():
    """The rule accepts the byte of the exact residual for 10^5 random residuals, and rejects both neighbouring codes wherever the interval
    holds a single code."""
    g = cd.gen(77)
    res = (torch.randn(100000, generator=g) * torch.exp2(torch.randint(-12, 5, (100000,), generator=g).float())).clamp(-16, 16)
    lo = res.half().float()
    exact = cd.e4m3_codes(16.0 * res)
    assert cd.lo8_in_interval(exact, lo) == 0
    dn, up = cd.lo8_interval(lo)
    single = (dn == up) & (lo != 0)
    assert int(single.sum()) > 50000
    code = cd.e4m3_codes(dn)[single].int()
    mag = code & 0x7F
    for step in (1, -1):
        ok = (mag + step >= 0) & (mag + step <= 0x7E)          # stay off the NaN code and on this side of zero
        nb = ((code & 0x80) | (mag + step).clamp(0, 0x7E)).to(torch.uint8)
        assert int(ok.sum()) > 40000 and cd.lo8_in_interval(nb[ok], lo[single][ok]) == int(ok.sum())


def test_pool_key_order_is_the_order_of_the_values():
    """The 24-bit key orders pairs (hi, lo8) as hi + lo8 / 16 does wherever |lo8 / 16| is below half an ulp of hi: all pairs of a set of hi words
    (both zero signs, subnormals, the largest) x every lo8 code under that bound."""
    hs = torch.tensor([0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -14, 0.5, -0.5, 1.0, 1.0 + 2.0 ** -10, -1.0, 3.0, 1000.0, -1000.0, 65504.0, -65504.0], dtype=torch.float16)
    codes = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)
    H, Cc = hs[:, None].expand(len(hs), len(codes)).contiguous(), codes[None, :].expand(len(hs), len(codes)).contiguous()
    l = cd.e4m3_values(Cc.contiguous()).double() / 16
    _, e = np.frexp(np.abs(H.numpy()).astype(np.float64))
    ulp = torch.tensor(np.ldexp(1.0, np.where(H.numpy() == 0, -14, np.maximum(e - 1, -14)) - 10))          # fp16: 10 fraction bits, subnormals below 2^-14
    keep = (l.abs() < ulp / 2).reshape(-1)
    h, c, v = H.reshape(-1)[keep], Cc.reshape(-1)[keep], (H.double() + l).reshape(-1)[keep]
    assert int(keep.sum()) > 500
    k = cd.pool_key(h, c)
    ki, kj, vi, vj = k[:, None], k[None, :], v[:, None], v[None, :]
    assert bool(((ki < kj) <= (vi <= vj)).all()) and bool(((vi < vj) <= (ki < kj)).all())
    h2, c2 = cd.pool_unkey(k)
    assert torch.equal(h2.view(torch.int16), h.contiguous().view(torch.int16)) and torch.equal(c2, c)


# ---------------------------------------------------------------------------------------------------------------- refused arguments
def test_entry_points_check_their_arguments(nv):
    """Every row violates one documented precondition and is answered with -1 before anything is launched."""
    lib = nv.lib()
    ok = ctypes.c_void_p(16)
    st = nv.ll_array([64, 64, 64, 8, 1])
    conv = lambda nd=3, D=8, ci=32, co=32, epi=0: (nd, ok, 64, ok, 64, ok, 64, 4, ok, 64, ok, ok, ok, ok, 1, D, 8, 16, ci, co, epi, None, None)
    pool = lambda nd=3, D=8, H=8, W=16, co=32: (nd, ok, 64, ok, 64, ok, 64, -1, ok, 64, ok, 64, ok, 64, ok, ok, ok, ok, 1, D, H, W, 32, co, 2, None, None)
    head = lambda nd=3, ncls=2, act=64.0, ci=32: (nd, ok, 64, ok, 64, ok, ok, ok, ok, ok, ok, act, ncls, ok, ok, ok, st, 1.0, 0, 1, 8 if nd == 3 else 1, 8, 16, ci, None, None)
    x2conv = lambda nd=3, ci=32, co=32, epi=0: (nd, ok, 64, 4, ok, 64, 4, ok, ok, ok, 1, 8 if nd == 3 else 1, 8, 16, ci, co, epi, None, None)
    first = lambda nd=3, act=64.0, cin=1, co=32, dt=0: (nd, ok, dt, st, ok, 64, 4, ok, 64, ok, ok, ok, act, 1, 8 if nd == 3 else 1, 8, 16, cin, co, 1, None, None)
    convT = lambda nd=3, ci=32, co=32: (nd, ok, 64, 4, ok, 64, 4, ok, 64, ok, ok, ok, 1, 8 if nd == 3 else 1, 8, 16, ci, co, None, None)
    gn = lambda C=32, groups=8, x_lo=4: (ok, 64, x_lo, ok, 64, 4, ok, 64, ok, ok, groups, 1e-5, 64.0, ok, ok, ok, C, 1, 64, None, None)
    stage = lambda act=64.0, H=8, W=16, py=ok: (ok, 0, st, ok, ok, ok, act, ok, 64, -1, ok, 64, py, 64, py, 64, ok, ok, ok, ok, 1, H, W, None, None)
    bad = [
        ('iunet_x2m_conv_fwd', conv(nd=4)), ('iunet_x2m_conv_fwd', conv(nd=1)), ('iunet_x2m_conv_fwd', conv(nd=2)),          # 2-D with D = 8
        ('iunet_x2m_conv_fwd', conv(ci=48)), ('iunet_x2m_conv_fwd', conv(co=16)), ('iunet_x2m_conv_fwd', conv(epi=3)),
        ('iunet_x2m_conv_pool_fwd', pool(nd=4)), ('iunet_x2m_conv_pool_fwd', pool(D=7)), ('iunet_x2m_conv_pool_fwd', pool(H=9)),
        ('iunet_x2m_conv_pool_fwd', pool(W=15)), ('iunet_x2m_conv_pool_fwd', pool(co=48)),
        ('iunet_x2m_conv_head_fwd', head(nd=4)), ('iunet_x2m_conv_head_fwd', head(ncls=1)), ('iunet_x2m_conv_head_fwd', head(ncls=4)),
        ('iunet_x2m_conv_head_fwd', head(act=48.0)), ('iunet_x2m_conv_head_fwd', head(ci=40)),
        ('iunet_x2_conv3_fwd_flag', x2conv(nd=1)), ('iunet_x2_conv3_fwd_flag', x2conv(ci=24)), ('iunet_x2_conv3_fwd_flag', x2conv(co=40)),
        ('iunet_x2_conv3_fwd_flag', x2conv(epi=-1)),
        ('iunet_x2_maxpool_fwd', (4, ok, 64, 4, ok, 64, 4, 8, 1, 1, 4, 4, None)), ('iunet_x2_maxpool_fwd', (2, ok, 64, 4, ok, 64, 4, 12, 1, 1, 4, 4, None)),
        ('iunet_x2_maxpool_fwd', (2, ok, 64, 4, ok, 64, 4, 8, 1, 1, 0, 4, None)),
        ('iunet_x2m_maxpool_fwd', (1, ok, 64, ok, 64, ok, 64, ok, 64, 16, 1, 1, 4, 4, None)), ('iunet_x2m_maxpool_fwd', (2, ok, 64, ok, 64, ok, 64, ok, 64, 24, 1, 1, 4, 4, None)),
        ('iunet_x2m_maxpool_fwd', (2, ok, 64, ok, 64, ok, 64, None, 64, 16, 1, 1, 4, 4, None)),
        ('iunet_x2m_make8', (ok, 64, 2, ok, 64, 24, 1, 1, 4, 4, None)), ('iunet_x2m_make8', (ok, 64, 2, None, 64, 16, 1, 1, 4, 4, None)),
        ('iunet_x2m_make8', (ok, 64, 2, ok, 64, 16, 1, 1, 0, 4, None)),
        ('iunet_x2m_first_conv_fwd', first(nd=4)), ('iunet_x2m_first_conv_fwd', first(act=100.0)), ('iunet_x2m_first_conv_fwd', first(cin=5)),
        ('iunet_x2m_first_conv_fwd', first(co=48)), ('iunet_x2m_first_conv_fwd', first(dt=4)),
        ('iunet_x2_first_conv_fwd', (3, ok, 0, st, ok, 64, -1, ok, ok, ok, 64.0, 1, 8, 8, 16, 1, 32, 1, None)),          # the fp16x2 form needs its lo planes
        ('iunet_x2_first_conv_fwd', (5, ok, 0, st, ok, 64, 4, ok, ok, ok, 64.0, 1, 8, 8, 16, 1, 32, 1, None)),
        ('iunet_x2m_convT_fwd', convT(nd=4)), ('iunet_x2m_convT_fwd', convT(ci=48)), ('iunet_x2m_convT_fwd', convT(co=16)),
        ('iunet_x2_convT_fwd', (3, ok, 64, 4, ok, 64, -1, ok, ok, ok, 1, 8, 8, 16, 32, 32, None)), ('iunet_x2_convT_fwd', (2, ok, 64, 4, ok, 64, 4, ok, ok, ok, 1, 1, 8, 16, 32, 40, None)),
        ('iunet_x2m_gn_relu_fwd', gn(C=24)), ('iunet_x2m_gn_relu_fwd', gn(groups=5)), ('iunet_x2m_gn_relu_fwd', gn(x_lo=0)),
        ('iunet_x2_gn_relu_fwd', (ok, 64, 4, ok, 64, 0, ok, ok, 8, 1e-5, 64.0, ok, ok, ok, 32, 1, 64, None, None)),
        ('iunet_x2_gn_relu_fwd', (ok, 64, 4, ok, 64, 4, ok, ok, 5, 1e-5, 64.0, ok, ok, ok, 32, 1, 64, None, None)),
        ('iunet_x2m_first_stage_fwd', stage(act=3.0)), ('iunet_x2m_first_stage_fwd', stage(H=9)), ('iunet_x2m_first_stage_fwd', stage(W=17)),
        ('iunet_x2_head_fwd', (ok, 64, 4, 32, ok, ok, 64.0, 1, ok, ok, ok, st, 1.0, 0, 1, 1, 8, 8, None)),
    ]
    for name, args in bad:
        assert getattr(lib, name)(*args) == -1, (name, args, lib.iunet_last_error())
    assert {name for name, _ in bad} == ENTRY_POINTS
    # an activation scale that is no power of two is refused where the operator is prepared, too
    assert lib.iunet_x2_prep(ok, ok, ok, ok, None, None, None, None, None, 1e-5, 48.0, 64.0, 32, 32, 27, 0, 16, None) == -1
    assert lib.iunet_x2m_prep_nd(3, ok, ok, ok, ok, ok, None, None, None, None, 1e-5, 64.0, 3.0, 32, 32, None) == -1
    assert lib.iunet_x2m_prep_nd(3, ok, ok, ok, ok, ok, None, None, None, None, 1e-5, 64.0, 64.0, 48, 32, None) == -1
