"""The split-precision prediction kernels -- the fp16x2 form (csrc/split16.hip, the SPL path of conv3_v4.hip, gn_precise.hip) and the x2m
form (csrc/conv3_x2m.hip), what the benchmark's prediction leg runs -- one entry point at a time, across host dispatch branch x buffer
placement, through the C ABI.

The rules are those of tests/test_gpu_f32_matrix.py.  Every activation sits in a NaN-sentinel arena as the networks lay it out
(tests/arena.py: SplitOperand, M8Operand): `tight`, `gap` (sample stride + 37 x 16 bytes, 5 x 16 bytes in), and the two halves `skip` / `up`
of a concat buffer [skip_hi | up_hi | skip_lo | up_lo] of 2 C channels (y_lo = 2 C / 8, the m8 planes of `up` C / 16 granule planes in).
Each case runs at `tight` first and then once per further row, and asserts
  1. the tight result against a reference that owes nothing to the library;
  2. the same bits at every other row;
  3. intact sentinels around outputs (the other half of a concat buffer included), inputs unchanged bit for bit;
  4. no unwritten fp16 word, and a range flag (`sat`) of 0.
Most rows are EXACT (tests/contract_data.py states and asserts the conditions): the kernels consume WORDS, so hand-made planes whose
products and sums are small multiples of a power of two make every partial sum exact in fp32 in any order, and the reference is the
float64 sum of the terms the kernel computes (fp16x2: x_hi w_hi + x_lo w_hi + x_hi w_lo; x2m: x_hi w_hi + x_lo8 w_hi8 + x_hi8 w_lo8).  Rows
on random data go against float64 on the values the split words hold, at the bars the project already states: 3e-6 (fp16x2 convs), 6e-5
(x2m convs), 2e-6 x max(1, |want|) (GroupNorm); a lo8 byte beside non-exact words obeys the interval rule (contract_data.lo8_interval).

Each id names its regime, asserted from a restatement of the launchers' arithmetic written once below (brick_shape, the `small` rule,
slot groups, kc / nchunks / cap of the transposed conv).  Every assertion on what the DEVICE produced goes through verify();
tests/test_x2_matrix_cpu.py runs every body once against a stub binding (DEVICE = 'cpu', verify muted), where only the plain asserts and the
binding's argument checks can fail.  Needs an MI355X: run with -m gpu."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import contract_data as cd
from tests.arena import SENTINEL, M8Operand, Operand, SplitOperand, StridedInput, StridedOutput, bits, scratch as _scratch, unblocked

pytestmark = pytest.mark.gpu

F32, F16, U8 = torch.float32, torch.float16, torch.uint8
DEVICE = 'cuda'
A = 64.0          # act_scale of the networks
TIGHT = 'tight'


@pytest.fixture(scope='module')
def nv():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from interactive_unet import _native
    _native.lib()
    return _native


# ---------------------------------------------------------------------------------------------------------------- helpers
def verify(cond, msg=''):
    assert cond, msg


def sync():
    if DEVICE == 'cuda':
        torch.cuda.synchronize()


def dhw(nd, grid):
    return tuple(grid) if nd == 3 else (1,) + tuple(grid)


def vol(grid):
    return int(np.prod(grid))


def ceil(a, b):
    return -(-a // b)


def vec(t, name, dtype=None):
    t = t.reshape(1, -1)
    return Operand(1, t.numel(), dtype or t.dtype, TIGHT, t, device=DEVICE, name=name)


def scratch(n, name, dtype=F32):
    return _scratch(n, dtype, DEVICE, name)


def preset(t, name, dtype=None):
    """A buffer the library reads AND writes: preset contents, watched like an output."""
    o = vec(t, name, dtype)
    o.is_input = False
    return o


def sat_word():
    return preset(torch.zeros(1), 'sat')


def sat_of(o):
    return int(bits(o.logical()).reshape(-1)[0])


def split_in(hi, lo, place, name, lo_at=None):
    """An input of the fp16x2 form [N, C, *sp] (lo None: hi planes alone, the lo planes it would have hold the sentinel)."""
    N, C = hi.shape[:2]
    return SplitOperand(N, C, hi[0, 0].numel(), place, hi, lo, own_lo=lo is not None, lo_at=lo_at, device=DEVICE, name=name)


def m8_in(codes, place, name):
    N, C = codes.shape[:2]
    return M8Operand(N, C, codes[0, 0].numel(), place, codes, device=DEVICE, name=name)


def split_out(N, C, vox, place, name, own_lo=True):
    return SplitOperand(N, C, vox, place, own_lo=own_lo, device=DEVICE, name=name)


def m8_out(N, C, vox, place, name):
    return M8Operand(N, C, vox, place, device=DEVICE, name=name)


def unwritten(t):
    """fp16 words that still hold the sentinel, a NaN no kernel stores (0xA5 is an ordinary e4m3 byte: the m8 planes are held by value)."""
    return int((bits(t) == SENTINEL[F16]).sum()) if t.dtype == F16 else 0


def over_rows(run, rows):
    """run(row) -> (read, operands): launches; read() -> {name: CPU tensor} once the stream is idle.  rows[0] is the all-tight row.  Asserts 2.,
    3. and 4. of the module docstring for every row.  A name a row does not produce -- lo words at y_lo = -1, a null y8 -- is skipped there, and
    the first row that produces a name is the one the later rows are held to; -> those first tensors."""
    base = {}
    for row in rows:
        read, ops = run(row)
        sync()
        for o in ops:
            o.check()
        got = read()
        sat = got.pop('sat', None)
        verify(sat is None or sat == 0, f'range flag {sat} at row {row}')
        for k, t in got.items():
            verify(unwritten(t) == 0, f'{k} [{row}]: {unwritten(t)} words never written')
        for k in got:
            if k in base:
                verify(torch.equal(bits(base[k]), bits(got[k])), f'{k}: row {row} changes the result ({int((bits(base[k]) != bits(got[k])).sum())} elements)')
            else:
                base[k] = got[k]
    return base


def same_value(got, ref, what):
    got, ref = got.reshape(-1).float(), ref.reshape(-1).float()
    verify(got.numel() == ref.numel() and not bool(torch.isnan(got).any()) and torch.equal(got, ref),
           f'{what}: {int((got != ref).sum()) if got.numel() == ref.numel() else "size"} of {ref.numel()} elements differ')


def same_bits(got, ref, what):
    verify(got.shape == ref.shape and torch.equal(bits(got), bits(ref)), f'{what}: {int((bits(got) != bits(ref)).sum()) if got.shape == ref.shape else "shape"} elements differ in their bits')


def rel_close(got, want, bar, what):
    """max |got - want| <= bar x max |want| (the form of the project's conv bars), NaN refused."""
    err = float((got.double() - want.double()).abs().max()) / float(want.abs().max())
    print(f'[{what}] max rel err {err:.2e} (bar {bar:.0e})')
    verify(err <= bar, f'{what}: max rel err {err:.3e} over the bar {bar:.0e}')


def exact_store(got, v, what, sp, C):
    """An exact row: hi = f16(v), hi + lo = v, lo8 = e4m3(16 (v - hi)) -- for whichever of hi / lo / m8 the row produced."""
    hi_ref, lo_ref = cd.split_words_of(v)
    hi = unblocked(got['hi'].float(), C, sp, 8)
    same_value(hi, hi_ref.reshape(hi.shape), f'{what}: hi words')
    if 'lo' in got:
        same_value(unblocked(got['lo'].float(), C, sp, 8), lo_ref.reshape(hi.shape), f'{what}: lo words')
    if 'm8' in got:
        same_value(cd.e4m3_values(unblocked(got['m8'], C, sp, 16)), cd.e4m3_round(16.0 * lo_ref).reshape(hi.shape), f'{what}: lo8 bytes')


def reader(yo, y8o=None, sat=None):
    def read():
        h, l = yo.logical()
        out = {'hi': h}
        if l is not None:
            out['lo'] = l
        if y8o is not None:
            out['m8'] = y8o.logical()
        if sat is not None:
            out['sat'] = sat_of(sat)
        return out
    return read


# ---------------------------------------------------------------------------------------------------------------- the launchers' arithmetic
def p2(v):
    r = 1
    while r * 2 <= v:
        r *= 2
    return r


def brick_shape(nd, ncob, tz, ty, tx):
    """common.h: iunet_brick_shape (without its A/B switch) -> (bz, by, bx)."""
    if nd == 3:
        z, y, x = (2, 4, 4) if ncob == 1 else (2, 4, 2) if ncob == 2 else (2, 2, 2) if ncob <= 4 else (1, 2, 2)
    else:
        z = 1
        y, x = (4, 8) if ncob == 1 else (4, 4) if ncob == 2 else (2, 4) if ncob <= 4 else (2, 2)
    want = z * y * x
    mz, my, mx = (p2(tz) if nd == 3 else 1), p2(ty), p2(tx)
    z, y, x = min(z, mz), min(y, my), min(x, mx)
    while z * y * x < want:
        if y * 2 <= my:
            y *= 2
        elif x * 2 <= mx:
            x *= 2
        elif z * 2 <= mz:
            z *= 2
        else:
            break
    return z, y, x


def slot_table(ncob):
    """iunet_conv3_v4_stats_parts: workgroups of one Cout tile over the 8 XCDs."""
    return 8 * (32 if ncob == 1 else 16 if ncob == 2 else 8 if ncob <= 4 else 4)


def halve(groups, nbricks):
    while groups > 1 and nbricks // 8 < groups:
        groups >>= 1
    return max(groups, 1)


def regime3(N, grid, cout, cob_in_rule=True, groups=False):
    """The 3-D stage convs (x2m_conv_impl, iunet_conv3_v4_x2_launch; cob_in_rule=False: iunet_x2m_conv_head_fwd, whose rule has no Cout factor;
    groups=True: launch_v4's slot groups, which launch_x2m does not have)."""
    D, H, W = grid
    big_tiles = N * ceil(D, 4) * ceil(H, 8) * ceil(W, 16)
    ncob = cout // 32
    small = big_tiles * (ncob if cob_in_rule else 1) < 128
    tz, ty, tx = ceil(D, 2 if small else 4), ceil(H, 8), ceil(W, 16)
    bz, by, bx = brick_shape(3, ncob, tz, ty, tx)
    nbricks = N * ceil(tz, bz) * ceil(ty, by) * ceil(tx, bx)
    g = halve(slot_table(ncob) // 8 // (bz * by * bx), nbricks) if groups else 1
    return dict(small=small, big_tiles=big_tiles, tiles=N * tz * ty * tx, ncob=ncob, brick=(bz, by, bx), nbricks=nbricks, groups=g, gx=8 * bz * by * bx * g)


def regime2(N, grid, cout):
    """The 2-D stage convs (launch_x2m_2d, launch_v4<2>): 16 x 32 tiles, slot groups."""
    H, W = grid
    ty, tx, ncob = ceil(H, 16), ceil(W, 32), cout // 32
    _, by, bx = brick_shape(2, ncob, 1, ty, tx)
    nbricks = N * ceil(ty, by) * ceil(tx, bx)
    g0 = slot_table(ncob) // 8 // (by * bx)
    g = halve(g0, nbricks)
    return dict(tiles=N * ty * tx, ncob=ncob, brick=(by, bx), nbricks=nbricks, groups0=g0, groups=g, gx=8 * by * bx * g, table=slot_table(ncob))


def regimeT(nd, N, grid, cin, cout):
    """iunet_x2m_convT_fwd: kc, chunks, the resident form, the wanted and the capped grid."""
    D, H, W = dhw(nd, grid)
    waves = N * D * H * ceil(W, 16)
    kc = 2 if (cin // 32) % 2 == 0 else 1
    nchunks = cin // 32 // kc
    chb = 2 * kc * (8 if nd == 3 else 4) * 2 * 1024
    lds = chb + 256 if nchunks == 1 else 2 * chb
    cap = max((2 if lds <= 80 * 1024 else 1) * 256 // (cout // 32), 1)
    want = ceil(waves, 8)
    gx = min(want, cap)
    passes = ceil(waves, gx * 8)
    return dict(kc=kc, nchunks=nchunks, resident=nchunks == 1, waves=waves, want=want, cap=cap, gx=gx, capped=want > cap,
                last_pass_partly_empty=waves % (gx * 8) != 0 and passes > 1)


def test_restated_launch_arithmetic_against_the_library(nv):
    """brick_shape, the slot groups and the `small` rule against iunet_conv3_sample_stats_rows: the rows of a per-sample launch of the 16-bit
    conv (layout 2: the tiles, bricks and groups of the split launches) are its grid, 8 x brick x groups on ONE sample's bricks -- or 0 below 8
    bricks.  (The function asks the runtime for the device: without one it answers 0, so these go through verify().)"""
    lib, checked = nv.lib(), 0
    for grid in ((16, 16), (17, 33), (64, 256), (40, 72), (130, 260), (512, 512), (33, 1000)):
        for cout in (32, 64, 128, 256):
            rg = regime2(1, grid, cout)
            rows = lib.iunet_conv3_sample_stats_rows(0, 2, 3, 1, grid[0], grid[1], 64, cout, 2)
            verify(rows == (rg['gx'] if rg['nbricks'] >= 8 else 0), f'2-D {grid} -> {cout}: {rows} rows, restated {rg}')
            checked += rg['nbricks'] >= 8
    for grid in ((13, 29, 61), (5, 9, 17), (32, 32, 32), (64, 64, 64), (16, 128, 128), (8, 200, 40), (24, 24, 48)):
        for cout in (32, 64, 128, 256):          # (Cin = 64: streamed weights, the launch the `small` rule applies to)
            rg = regime3(1, grid, cout, groups=True)
            rows = lib.iunet_conv3_sample_stats_rows(0, 3, 2, *grid, 64, cout, 2)
            verify(rows == (rg['gx'] if rg['nbricks'] >= 8 else 0), f'3-D {grid} -> {cout}: {rows} rows, restated {rg}')
            checked += rg['nbricks'] >= 8
    assert checked >= 30


# ---------------------------------------------------------------------------------------------------------------- operators
def prep_x2m(nv, nd, w, bn=None, act_out=A):
    """iunet_x2m_prep_nd + iunet_pack_conv3 into exactly sized scratch -> dict(w16, w8, osc, bias, whi, ops)."""
    co, ci = w.shape[:2]
    taps = 3 ** nd
    wo, whi = vec(w, 'w'), scratch(co * ci * taps, 'whi')
    nb = int(nv.lib().iunet_x2m_w8_bytes_nd(nd, co, ci))
    w8 = preset(torch.zeros(nb, dtype=U8), 'w8')          # (the K = 128 operator's padding bytes are the caller's zeros)
    osc, b = scratch(co, 'oscale'), scratch(co, 'bias_out')
    bnv = [vec(t, k) for t, k in zip(bn, ('gamma', 'beta', 'mean', 'var'))] if bn is not None else []
    bnp = [nv.ptr(o.t) for o in bnv] if bn is not None else [None] * 4
    nv.call('iunet_x2m_prep_nd', nd, nv.ptr(wo.t), nv.ptr(whi.t), nv.ptr(w8.t), nv.ptr(osc.t), nv.ptr(b.t), *bnp, 1e-5, A, float(act_out), co, ci, nv.stream())
    pm = 2 if nd == 3 else 6
    w16 = scratch(nv.pack_conv3_elems(co, ci, taps, pm), 'w16', F16)
    nv.call('iunet_pack_conv3', 0, nv.ptr(whi.t), None, nv.ptr(w16.t), co, ci, taps, pm, nv.stream())
    sync()
    return dict(w16=w16, w8=w8, osc=osc, bias=b, whi=whi, ops=[wo, whi, w8, osc, b, w16] + bnv)


def prep_x2(nv, nd, w, transposed=False, bias=None, bn=None, act_out=cd.X2_ACT_OUT, first=False):
    """iunet_x2_prep + the pack of its virtual operator -> dict(wpk, osc, bias, wv, kc, ops)."""
    ci, co = (w.shape[:2] if transposed else w.shape[1::-1])
    taps = vol(w.shape[2:])
    kc = int(nv.lib().iunet_x2_convT_kc(ci)) if transposed else (ci if first else 16 if nd == 3 else 32)
    wo, wv = vec(w, 'w'), scratch((2 if transposed else 3) * ci * co * taps, 'wv')
    osc, b = scratch(co, 'oscale'), scratch(co, 'bias_out')
    bo = vec(bias, 'bias_in') if bias is not None else None
    bnv = [vec(t, k) for t, k in zip(bn, ('gamma', 'beta', 'mean', 'var'))] if bn is not None else []
    bnp = [nv.ptr(o.t) for o in bnv] if bn is not None else [None] * 4
    nv.call('iunet_x2_prep', nv.ptr(wo.t), nv.ptr(wv.t), nv.ptr(osc.t), nv.ptr(b.t), *bnp, nv.ptr(bo.t) if bo is not None else None, 1e-5, A, float(act_out),
            co, ci, taps, 2 if transposed else 0, 0 if transposed else kc, nv.stream())
    if transposed:
        wpk = scratch(2 * ci * co * taps, 'wpk', F16)
        nv.call('iunet_pack_convT', 0, nv.ptr(wv.t), nv.ptr(wpk.t), 2 * ci, co, taps, nv.stream())
    elif first:
        wpk = scratch(int(nv.lib().iunet_pack_first_conv_elems(co, 3 * ci, taps)), 'wpk', F16)
        nv.call('iunet_pack_first_conv', 0, nv.ptr(wv.t), None, nv.ptr(wpk.t), co, 3 * ci, taps, nv.stream())
    else:
        pm = int(nv.lib().iunet_x2_pack_mode(nd))
        assert pm == (2 if nd == 3 else 6)
        wpk = scratch(nv.pack_conv3_elems(co, 3 * ci, taps, pm), 'wpk', F16)
        nv.call('iunet_pack_conv3', 0, nv.ptr(wv.t), None, nv.ptr(wpk.t), co, 3 * ci, taps, pm, nv.stream())
    sync()
    return dict(wpk=wpk, osc=osc, bias=b, wv=wv, kc=kc, ops=[wo, wv, osc, b, wpk] + bnv + ([bo] if bo is not None else []))


def bn_vectors(g, C, shift=0.0):
    return (0.75 + 0.5 * torch.rand(C, generator=g), 0.1 * torch.randn(C, generator=g) + shift, 0.2 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g))


def canonical_split(x):
    """fp32 values -> hi = f16(A x), lo = f16(A x - hi) (fp32 tensors of fp16 values) and the float64 value the two words hold, / A."""
    v = x * A
    hi = v.half().float()
    lo = (v - hi).half().float()
    return hi, lo, (hi.double() + lo.double()) / A


# ---------------------------------------------------------------------------------------------------------------- 1., 2. the x2m stage conv
def x2m_conv_call(nv, nd, xo, x8o, yo, y8o, op, N, grid, ci, co, epi, sat):
    D, H, W = dhw(nd, grid)
    nv.call('iunet_x2m_conv_fwd', nd, nv.ptr(xo.t), xo.ss, nv.ptr(x8o.t), x8o.ss, nv.ptr(yo.t), yo.ss, yo.lo, nv.ptr(y8o.t) if y8o is not None else None,
            y8o.ss if y8o is not None else 0, nv.ptr(op['w16'].t), nv.ptr(op['w8'].t), nv.ptr(op['osc'].t), nv.ptr(op['bias'].t) if epi else None,
            N, D, H, W, ci, co, epi, nv.ptr(sat.t), nv.stream())


# x / x8 / y / y8 placements, y_lo >= 0 or -1, y8 present or null
X2M_ROWS = [dict(x=TIGHT, x8=TIGHT, y=TIGHT, y8=TIGHT, lo=True, m8=True),
            dict(x='gap', x8='up', y='up', y8='up', lo=True, m8=True),
            dict(x='skip', x8='gap', y='skip', y8='skip', lo=False, m8=True),
            dict(x='up', x8='skip', y='gap', y8=None, lo=True, m8=False)]


def x2m_conv_rows(nv, nd, N, grid, ci, co, X, codes, op, epi, rows=X2M_ROWS):
    vox = vol(grid)

    def run(r):
        xo, x8o = split_in(X, None, r['x'], 'x'), m8_in(codes, r['x8'], 'x8')
        yo = split_out(N, co, vox, r['y'], 'y', own_lo=r['lo'])
        y8o = m8_out(N, co, vox, r['y8'], 'y8') if r['m8'] else None
        sat = sat_word()
        x2m_conv_call(nv, nd, xo, x8o, yo, y8o, op, N, grid, ci, co, epi, sat)
        return reader(yo, y8o, sat), [xo, x8o, yo, sat] + ([y8o] if y8o is not None else []) + op['ops']
    return over_rows(run, rows)


def x2m_exact_case(nv, nd, N, grid, ci, co):
    a, b, w = cd.x2m_exact_operator(nd, co, ci, 11 + nd)
    X, L8 = cd.x2m_exact_input(N, ci, grid, 100 * nd + N + ci)
    want = cd.x2m_exact_ref(nd, X, L8, a, b)
    op = prep_x2m(nv, nd, w, act_out=1.0)
    same_value(op['whi'].logical(), 16.0 * a, 'w_hi of the prepared operator')          # the row scale is 1
    same_value(op['osc'].logical(), torch.full((co,), 1.0 / 64), 'oscale')
    got = x2m_conv_rows(nv, nd, N, grid, ci, co, X, cd.e4m3_codes(L8), op, 0)
    exact_store(got, want / 64.0, f'x2m conv {nd}-D', grid, co)


X2M_3D = [pytest.param(2, (5, 9, 17), 32, 32, True, '', id='small_tile-ragged_zyx-N2-32to32'),
          pytest.param(2, (13, 29, 61), 32, 32, False, 'threshold', id='big_tile-threshold_128tiles_4bricks-N2-32to32'),
          pytest.param(1, (13, 29, 61), 96, 64, False, '2cob', id='big_tile-2cob_3chunkpairs-N1-96to64'),
          pytest.param(5, (13, 29, 61), 32, 32, False, '320tiles', id='big_tile-320tiles_on_256wg-N5-32to32')]


def assert_regime3(N, grid, co, small, rg=None):
    rg = rg or regime3(N, grid, co)
    assert rg['small'] == small, rg
    tz = 2 if small else 4
    assert grid[0] % tz and grid[1] % 8 and grid[2] % 16, 'ragged on all three axes'
    return rg


@pytest.mark.parametrize('N,grid,ci,co,small,tag', X2M_3D)
def test_x2m_conv_3d_exact(nv, N, grid, ci, co, small, tag):
    rg = assert_regime3(N, grid, co, small)
    cid = tag
    if 'threshold' in cid:
        assert rg['big_tiles'] * rg['ncob'] == 128 and rg['nbricks'] == 4 < 8
    if '2cob' in cid:
        assert rg['ncob'] == 2 and rg['big_tiles'] * 2 == 128 and (ci // 32) % 2 == 1
    if '320tiles' in cid:
        assert rg['tiles'] == 320 and rg['gx'] == 256
    x2m_exact_case(nv, 3, N, grid, ci, co)


@functools.lru_cache(maxsize=None)
def x2m_random(nd, N, grid, ci, co, seed):
    """Random data for the x2m conv (epilogue 2 with a BatchNorm fold): hi words, the lo8 codes of the canonical residual, and the float64 conv
    of the values those words hold for a 3^d consumer: (hi + lo8 / 16) / A."""
    g = cd.gen(seed)
    x = torch.rand((N, ci) + tuple(grid), generator=g) * 2
    w = torch.randn((co, ci) + (3,) * nd, generator=g) * (2.0 / (ci * 3 ** nd)) ** 0.5
    bn = bn_vectors(g, co)
    hi, lo, xq = canonical_split(x)
    wf, bf = cd.fold_ref(w, bn, 1e-5, False)
    want = torch.relu(cd.conv_nd(nd)(xq, wf.double(), bf.double(), padding=1))
    return hi, cd.e4m3_codes(16.0 * lo), w, bn, want


def test_x2m_conv_3d_random_small_and_big_tile_give_the_same_bits(nv):
    """Epilogue 2 with a BatchNorm fold on random data at the 6e-5 bar; sample 0 of the N = 1 launch (small tile) and of the N = 2 launch (big
    tile) of the same data: one summation order per voxel whatever the tile, so the same bits in hi, lo and m8."""
    grid, ci, co = (13, 29, 61), 32, 32
    assert regime3(1, grid, co)['small'] and not regime3(2, grid, co)['small']
    hi, codes, w, bn, want = x2m_random(3, 2, grid, ci, co, 12)
    op = prep_x2m(nv, 3, w, bn)
    rows = [X2M_ROWS[0], X2M_ROWS[1]]
    big = x2m_conv_rows(nv, 3, 2, grid, ci, co, hi, codes, op, 2, rows)
    small = x2m_conv_rows(nv, 3, 1, grid, ci, co, hi[:1], codes[:1], op, 2, rows)
    got = (unblocked(big['hi'].float(), co, grid, 8).double() + unblocked(big['lo'].float(), co, grid, 8).double()) / A
    rel_close(got, want, 6e-5, 'x2m conv 3-D random, big tile')
    verify(cd.lo8_in_interval(unblocked(big['m8'], co, grid, 16), unblocked(big['lo'].float(), co, grid, 8)) == 0, 'lo8 bytes outside the interval of their lo words')
    for k in ('hi', 'lo', 'm8'):
        same_bits(small[k][0], big[k][0], f'sample 0, small tile against big tile: {k}')


X2M_2D = [pytest.param(5, (16, 16), 32, 32, (1, 1), 32, 1, id='groups1_halved_from_32-N5-16x16'),
          pytest.param(16, (16, 16), 32, 32, (1, 1), 32, 2, id='groups2-N16-16x16'),
          pytest.param(256, (16, 16), 32, 32, (1, 1), 32, 32, id='groups32-N256-16x16'),
          pytest.param(3, (17, 33), 32, 32, (2, 2), 8, 1, id='brick_clamped_2x2-groups8_halved_to_1-N3-17x33'),
          pytest.param(8, (64, 256), 32, 32, (4, 8), 1, 1, id='brick_4x8-one_brick_per_xcd-N8-64x256'),
          pytest.param(2, (40, 72), 64, 64, (2, 2), 4, 1, id='2cob_table16-N2-40x72-64to64')]


def assert_regime2(N, grid, co, brick, groups0, groups):
    rg = regime2(N, grid, co)
    assert (rg['brick'], rg['groups0'], rg['groups']) == (brick, groups0, groups), rg
    return rg


@pytest.mark.parametrize('N,grid,ci,co,brick,groups0,groups', X2M_2D)
def test_x2m_conv_2d_exact(nv, N, grid, ci, co, brick, groups0, groups):
    rg = assert_regime2(N, grid, co, brick, groups0, groups)
    if grid == (64, 256):
        assert rg['nbricks'] == 8
    if co == 64:
        assert rg['table'] == 8 * 16
    x2m_exact_case(nv, 2, N, grid, ci, co)


def test_x2m_conv_2d_random_batches_share_a_slice(nv):
    """The slice that the N = 256 batch (32 slot groups) and the N = 5 batch (one) share has the same bits in both."""
    grid, ci, co = (16, 16), 32, 32
    assert regime2(256, grid, co)['groups'] == 32 and regime2(5, grid, co)['groups'] == 1
    hi, codes, w, bn, want = x2m_random(2, 256, grid, ci, co, 32)
    op = prep_x2m(nv, 2, w, bn)
    rows = [X2M_ROWS[0], X2M_ROWS[1]]
    many = x2m_conv_rows(nv, 2, 256, grid, ci, co, hi, codes, op, 2, rows)
    few = x2m_conv_rows(nv, 2, 5, grid, ci, co, hi[:5], codes[:5], op, 2, rows)
    got = (unblocked(many['hi'].float(), co, grid, 8).double() + unblocked(many['lo'].float(), co, grid, 8).double()) / A
    rel_close(got, want, 6e-5, 'x2m conv 2-D random, 32 slot groups')
    for k in ('hi', 'lo', 'm8'):
        same_bits(few[k], many[k][:5], f'the shared slices, N = 5 against N = 256: {k}')


# ---------------------------------------------------------------------------------------------------------------- 3. the fp16x2 stage conv
def x2_conv_call(nv, nd, xo, yo, op, N, grid, ci, co, epi, sat):
    D, H, W = dhw(nd, grid)
    nv.call('iunet_x2_conv3_fwd_flag', nd, nv.ptr(xo.t), xo.ss, xo.lo, nv.ptr(yo.t), yo.ss, yo.lo, nv.ptr(op['wpk'].t), nv.ptr(op['osc'].t),
            nv.ptr(op['bias'].t) if epi else None, N, D, H, W, ci, co, epi, nv.ptr(sat.t) if sat is not None else None, nv.stream())


# x / y placement and the distance of x's lo planes at tight / gap (None: C / 8; the concat halves have 2 C / 8 by construction)
X2_ROWS = [dict(x=TIGHT, y=TIGHT, lo_at=None), dict(x='gap', y='up', lo_at=2), dict(x='skip', y='gap', lo_at=None), dict(x='up', y='skip', lo_at=None)]


def x2_conv_rows(nv, nd, N, grid, ci, co, xh, xl, op, epi, rows=X2_ROWS):
    vox = vol(grid)

    def run(r):
        xo = split_in(xh, xl, r['x'], 'x', lo_at=r['lo_at'] and r['lo_at'] * ci // 8)
        assert xo.lo == (ci // 8 if r['x'] in (TIGHT, 'gap') and not r['lo_at'] else 2 * ci // 8)
        yo, sat = split_out(N, co, vox, r['y'], 'y'), sat_word()
        x2_conv_call(nv, nd, xo, yo, op, N, grid, ci, co, epi, sat)
        return reader(yo, None, sat), [xo, yo, sat] + op['ops']
    return over_rows(run, rows)


def x2_exact_case(nv, nd, N, grid, ci, co, epi):
    h, r = cd.split_exact_operator((co, ci) + (3,) * nd, 0, 300 + nd + ci)
    xh, xl = cd.split_exact_input(N, ci, grid, 310 + nd + N)
    bias = torch.randint(-4, 5, (co,), generator=cd.gen(320 + co)).float()
    acc = cd.split_exact_ref(nd, xh, xl, h, r, False)
    v = cd.split_store(acc, bias if epi else torch.zeros(co))
    if epi == 2:
        v = torch.relu(v)
        assert 0.2 < float((v == 0).float().mean()) < 0.8          # the ReLU is at work
    op = prep_x2(nv, nd, h + r, bias=bias)
    taps = 3 ** nd
    same_value(op['wv'].logical(), cd.x2_virtual_conv(h.reshape(co, ci, taps), r.reshape(co, ci, taps), op['kc']), 'the prepared virtual operator [w_hi | w_hi | w_lo]')
    same_value(op['osc'].logical(), torch.full((co,), cd.X2_ACT_OUT / cd.X2_ACT_IN), 'oscale')          # the row scale is 1
    same_value(op['bias'].logical(), cd.X2_ACT_OUT * bias, 'bias_out')
    got = x2_conv_rows(nv, nd, N, grid, ci, co, xh, xl, op, epi)
    exact_store(got, v, f'fp16x2 conv {nd}-D epi {epi}', grid, co)


X2_3D = [pytest.param(2, (5, 9, 17), 32, 32, True, 2, id='small_tile-ragged_zyx-N2-32to32-epi2'),
         pytest.param(2, (5, 9, 17), 32, 32, True, 0, id='small_tile-ragged_zyx-N2-32to32-epi0'),
         pytest.param(2, (13, 29, 61), 32, 32, False, 1, id='big_tile-threshold_128tiles-N2-32to32-epi1'),
         pytest.param(1, (13, 29, 61), 96, 64, False, 2, id='big_tile-2cob-N1-96to64-epi2')]


@pytest.mark.parametrize('N,grid,ci,co,small,epi', X2_3D)
def test_x2_conv_3d_exact(nv, N, grid, ci, co, small, epi):
    """Nonzero lo words that are independent of the hi words: an error in lo-plane addressing shows."""
    assert_regime3(N, grid, co, small, regime3(N, grid, co, groups=True))
    x2_exact_case(nv, 3, N, grid, ci, co, epi)


X2_2D = [pytest.param(*p.values, e, id=f'{p.id}-epi{e}') for p, e in zip(X2M_2D, (2, 0, 1, 2, 1, 2))]


@pytest.mark.parametrize('N,grid,ci,co,brick,groups0,groups,epi', X2_2D)
def test_x2_conv_2d_exact(nv, N, grid, ci, co, brick, groups0, groups, epi):
    assert_regime2(N, grid, co, brick, groups0, groups)          # (launch_v4 halves its slot groups by the same rule on the same tiles)
    x2_exact_case(nv, 2, N, grid, ci, co, epi)


@functools.lru_cache(maxsize=None)
def x2_random(nd, N, grid, ci, co, seed):
    g = cd.gen(seed)
    x = torch.rand((N, ci) + tuple(grid), generator=g) * 2
    w = torch.randn((co, ci) + (3,) * nd, generator=g) * (2.0 / (ci * 3 ** nd)) ** 0.5
    bn = bn_vectors(g, co)
    hi, lo, xq = canonical_split(x)
    wf, bf = cd.fold_ref(w, bn, 1e-5, False)
    return hi, lo, w, bn, torch.relu(cd.conv_nd(nd)(xq, wf.double(), bf.double(), padding=1))


@pytest.mark.parametrize('nd,grid,Ns', [pytest.param(3, (13, 29, 61), (1, 2), id='3d-small_tile_N1-against-big_tile_N2'),
                                        pytest.param(2, (16, 16), (5, 256), id='2d-groups1_N5-against-groups32_N256')])
def test_x2_conv_random_launches_share_their_bits(nv, nd, grid, Ns):
    """The fp16x2 conv on random data at the 3e-6 bar, and the samples two launches of different regimes share: the same bits."""
    ci = co = 32
    if nd == 3:
        assert regime3(Ns[0], grid, co)['small'] and not regime3(Ns[1], grid, co)['small']
    else:
        assert regime2(Ns[0], grid, co)['groups'] == 1 and regime2(Ns[1], grid, co)['groups'] == 32
    hi, lo, w, bn, want = x2_random(nd, Ns[1], grid, ci, co, 40 + nd)
    op = prep_x2(nv, nd, w, bn=bn, act_out=A)
    rows = [X2_ROWS[0], X2_ROWS[1]]
    many = x2_conv_rows(nv, nd, Ns[1], grid, ci, co, hi, lo, op, 2, rows)
    few = x2_conv_rows(nv, nd, Ns[0], grid, ci, co, hi[:Ns[0]], lo[:Ns[0]], op, 2, rows)
    got = (unblocked(many['hi'].float(), co, grid, 8).double() + unblocked(many['lo'].float(), co, grid, 8).double()) / A
    rel_close(got, want, 3e-6, f'fp16x2 conv {nd}-D random')
    for k in ('hi', 'lo'):
        same_bits(few[k], many[k][:Ns[0]], f'the shared samples, N = {Ns[0]} against N = {Ns[1]}: {k}')


# ---------------------------------------------------------------------------------------------------------------- 4. conv + pool in one launch
# The issue's (12, 28, 60) shapes have 48 big tiles per sample, 96 per launch: by the launcher's rule (>= 128) they run the SMALL tile, and
# their ids say so; (14, 30, 62) -- 64 per sample -- is the smallest even ragged grid that reaches the big tile with these N and Cout.
X2M_POOL = [pytest.param(3, 1, (4, 8, 16), 32, 32, True, id='3d-small_tile-one_tile-N1'),
            pytest.param(3, 2, (12, 28, 60), 32, 32, True, id='3d-small_tile-96_big_tiles-N2-32to32'),
            pytest.param(3, 1, (12, 28, 60), 32, 64, True, id='3d-small_tile-96_big_tiles-N1-32to64'),
            pytest.param(3, 2, (14, 30, 62), 32, 32, False, id='3d-big_tile-128_tiles-N2-32to32'),
            pytest.param(3, 1, (14, 30, 62), 32, 64, False, id='3d-big_tile-2cob-N1-32to64'),
            pytest.param(2, 3, (18, 34), 32, 32, None, id='2d-ragged_2x2_tiles-N3'),
            pytest.param(2, 8, (64, 256), 32, 32, None, id='2d-brick_4x8-N8')]
POOL_ROWS = [dict(y=TIGHT, y8=TIGHT, py=TIGHT, py8=TIGHT), dict(y='gap', y8='up', py='skip', py8='skip'),
             dict(y='skip', y8='gap', py='up', py8='up'), dict(y='up', y8='skip', py='gap', py8='gap')]


@pytest.mark.parametrize('nd,N,grid,ci,co,small', X2M_POOL)
def test_x2m_conv_pool_exact(nv, nd, N, grid, ci, co, small):
    """y / y8 against the reference conv (epilogue 2, integer biases, ReLU zeros), the pooled pair against the CPU maximum of the 24-bit keys."""
    assert all(s % 2 == 0 for s in grid)
    if nd == 3:
        assert regime3(N, grid, co)['small'] == small
    a, b, w = cd.x2m_exact_operator(nd, co, ci, 11 + nd)
    X, L8 = cd.x2m_exact_input(N, ci, grid, 400 * nd + N + co)
    bias = torch.randint(-8, 9, (co,), generator=cd.gen(410 + co)).float()
    v = torch.relu(cd.x2m_exact_ref(nd, X, L8, a, b) / 64.0 + bias.double().view([1, -1] + [1] * nd))
    assert 0.2 < float((v == 0).float().mean()) < 0.8
    hi_ref, lo_ref = cd.split_words_of(v)
    code_ref = cd.e4m3_codes(16.0 * lo_ref)
    ph_ref, p8_ref = cd.pool_by_key(hi_ref.half(), code_ref, nd)
    op = prep_x2m(nv, nd, w, act_out=1.0)
    bo = vec(bias, 'bias')
    vox, pgrid = vol(grid), tuple(s // 2 for s in grid)
    D, H, W = dhw(nd, grid)
    codes = cd.e4m3_codes(L8)

    def run(r):
        xo, x8o = split_in(X, None, TIGHT, 'x'), m8_in(codes, TIGHT, 'x8')
        yo, y8o = split_out(N, co, vox, r['y'], 'y', own_lo=False), m8_out(N, co, vox, r['y8'], 'y8')
        po, p8o = split_out(N, co, vol(pgrid), r['py'], 'py', own_lo=False), m8_out(N, co, vol(pgrid), r['py8'], 'py8')
        sat = sat_word()
        nv.call('iunet_x2m_conv_pool_fwd', nd, nv.ptr(xo.t), xo.ss, nv.ptr(x8o.t), x8o.ss, nv.ptr(yo.t), yo.ss, -1, nv.ptr(y8o.t), y8o.ss,
                nv.ptr(po.t), po.ss, nv.ptr(p8o.t), p8o.ss, nv.ptr(op['w16'].t), nv.ptr(op['w8'].t), nv.ptr(op['osc'].t), nv.ptr(bo.t),
                N, D, H, W, ci, co, 2, nv.ptr(sat.t), nv.stream())
        read = lambda: {'hi': yo.logical()[0], 'm8': y8o.logical(), 'pooled hi': po.logical()[0], 'pooled m8': p8o.logical(), 'sat': sat_of(sat)}
        return read, [xo, x8o, yo, y8o, po, p8o, sat, bo] + op['ops']

    got = over_rows(run, POOL_ROWS)
    exact_store(got, v, f'x2m conv + pool {nd}-D: y', grid, co)
    same_bits(unblocked(got['pooled hi'], co, pgrid, 8), ph_ref.reshape((N, co) + pgrid), 'pooled hi words against the key maximum')
    same_value(cd.e4m3_values(unblocked(got['pooled m8'], co, pgrid, 16)), cd.e4m3_values(p8_ref), 'pooled lo8 bytes against the key maximum')


# ---------------------------------------------------------------------------------------------------------------- 5. the head in the conv's epilogue
class HeadOutputs:
    """logits and probs as class planes of wider channels-last tensors, cls tight (tests/test_gpu_head_contract.py: Outputs) on DEVICE."""

    def __init__(self, N, ncls, grid):
        self.logits = StridedOutput((N, ncls) + grid, device=DEVICE, name='logits')
        self.probs = StridedOutput((N, ncls) + grid, device=DEVICE, name='probs')
        self.cls = Operand(N, vol(grid), U8, TIGHT, None, device=DEVICE, name='cls')
        self.strides = self.probs.strides


def head_contract(call, N, ncls, grid):
    """run_contract of tests/test_gpu_head_contract.py (the accumulate and divisor pass, cls = the first maximum, intact sentinels) on the
    device; against the stub binding the two calls alone."""
    if DEVICE == 'cuda':
        from tests.test_gpu_head_contract import run_contract
        return run_contract(call, N, ncls, grid)
    o = HeadOutputs(N, ncls, grid)
    call(o, 1.0, 0)
    call(o, 3.0, 1)
    return o.logits.logical(), o.probs.logical(), o.cls.logical()


X2M_HEAD = [pytest.param(3, 2, (13, 29, 61), 2, id='3d-big_tile-N2-ncls2'), pytest.param(3, 2, (13, 29, 61), 3, id='3d-big_tile-N2-ncls3'),
            pytest.param(2, 16, (16, 16), 3, id='2d-groups2-N16-ncls3')]


@pytest.mark.parametrize('nd,N,grid,ncls', X2M_HEAD)
def test_x2m_conv_head_is_conv_plus_head_bit_for_bit(nv, nd, N, grid, ncls):
    ci = co = 32
    if nd == 3:
        assert not regime3(N, grid, co, cob_in_rule=False)['small']
    else:
        assert regime2(N, grid, co)['groups'] == 2
    hi, codes, w, bn, _ = x2m_random(nd, N, grid, ci, co, 50 + nd)
    g = cd.gen(55 + ncls)
    hw, hb = vec(torch.randn((ncls, co), generator=g) * 0.3, 'head_w'), vec(torch.randn(ncls, generator=g) * 0.1, 'head_b')
    op = prep_x2m(nv, nd, w, bn)
    D, H, W = dhw(nd, grid)
    xo, x8o = split_in(hi, None, 'gap', 'x'), m8_in(codes, 'up', 'x8')
    yo = split_out(N, co, vol(grid), TIGHT, 'y')
    x2m_conv_call(nv, nd, xo, x8o, yo, None, op, N, grid, ci, co, 2, sat_word())

    def unfused(o, divisor, accumulate):
        nv.call('iunet_x2_head_fwd', nv.ptr(yo.t), yo.ss, yo.lo, co, nv.ptr(hw.t), nv.ptr(hb.t), A, ncls, nv.ptr(o.logits.t), nv.ptr(o.probs.t), nv.ptr(o.cls.t),
                nv.ll_array(o.strides), float(divisor), accumulate, N, D, H, W, nv.stream())

    def fused(o, divisor, accumulate):
        nv.call('iunet_x2m_conv_head_fwd', nd, nv.ptr(xo.t), xo.ss, nv.ptr(x8o.t), x8o.ss, nv.ptr(op['w16'].t), nv.ptr(op['w8'].t), nv.ptr(op['osc'].t),
                nv.ptr(op['bias'].t), nv.ptr(hw.t), nv.ptr(hb.t), A, ncls, nv.ptr(o.logits.t), nv.ptr(o.probs.t), nv.ptr(o.cls.t), nv.ll_array(o.strides),
                float(divisor), accumulate, N, D, H, W, ci, None, nv.stream())

    g3 = dhw(nd, grid)
    l0, p0, c0 = head_contract(unfused, N, ncls, g3)
    l1, p1, c1 = head_contract(fused, N, ncls, g3)
    for o in [xo, x8o, yo, hw, hb] + op['ops']:
        o.check()
    same_bits(l1, l0, 'logits, fused against conv + head')
    same_bits(p1, p0, 'probabilities, fused against conv + head')
    same_bits(c1, c0, 'class map, fused against conv + head')
    verify(float(l0.abs().max()) > 0.1, 'the logits are all but zero')


# ---------------------------------------------------------------------------------------------------------------- 6. max-pools
POOLS = [pytest.param(2, 2, 1, (9, 31), id='2d-1chunk-out9x31'), pytest.param(2, 2, 6, (9, 31), id='2d-C96-out9x31'),
         pytest.param(3, 2, 1, (3, 5, 7), id='3d-1chunk-out3x5x7'), pytest.param(3, 2, 6, (3, 5, 7), id='3d-C96-out3x5x7')]
MP_ROWS = [dict(x=TIGHT, y=TIGHT), dict(x='skip', y='up'), dict(x='up', y='skip'), dict(x='gap', y='gap')]


@pytest.mark.parametrize('nd,N,chunks,ogrid', POOLS)
def test_x2m_maxpool(nv, nd, N, chunks, ogrid):
    """The pooled (hi, lo8) pair is the window's largest 24-bit key: both words, bit for bit, on data full of ties."""
    C, igrid = 16 * chunks, tuple(2 * s for s in ogrid)
    assert vol(ogrid) % 256 and (chunks == 1 or vol(ogrid) * chunks > 256)
    hi, lo = cd.pool_tie_data(N, C, igrid, 600 + nd + C)
    codes = cd.e4m3_codes(lo)
    ph_ref, p8_ref = cd.pool_by_key(hi, codes, nd)
    Do, Ho, Wo = dhw(nd, ogrid)

    def run(r):
        xo, x8o = split_in(hi, None, r['x'], 'x'), m8_in(codes, r['x'], 'x8')
        yo, y8o = split_out(N, C, vol(ogrid), r['y'], 'y', own_lo=False), m8_out(N, C, vol(ogrid), r['y'], 'y8')
        nv.call('iunet_x2m_maxpool_fwd', nd, nv.ptr(xo.t), xo.ss, nv.ptr(x8o.t), x8o.ss, nv.ptr(yo.t), yo.ss, nv.ptr(y8o.t), y8o.ss, C, N, Do, Ho, Wo, nv.stream())
        return reader(yo, y8o), [xo, x8o, yo, y8o]

    got = over_rows(run, MP_ROWS)
    same_bits(unblocked(got['hi'], C, ogrid, 8), ph_ref, 'pooled hi words')
    same_bits(unblocked(got['m8'], C, ogrid, 16), p8_ref, 'pooled lo8 bytes')


@pytest.mark.parametrize('nd,N,chunks,ogrid', POOLS)
def test_x2_maxpool(nv, nd, N, chunks, ogrid):
    """fp16x2: the pooled value is the window maximum of hi + lo and the pooled pair is one of the window's pairs (x_lo = 2 C / 8 in the concat
    placements, as the networks call it)."""
    C, igrid = (8 if chunks == 1 else 96), tuple(2 * s for s in ogrid)
    assert vol(ogrid) % 256
    hi, lo = cd.pool_tie_data(N, C, igrid, 620 + nd + C)
    val = cd.windows(hi.float() + lo, nd)
    want = val.max(-1).values
    hb, lb = cd.windows(hi.view(torch.int16).int(), nd), cd.windows(lo.half().view(torch.int16).int(), nd)
    Do, Ho, Wo = dhw(nd, ogrid)

    def run(r):
        xo, yo = split_in(hi.float(), lo, r['x'], 'x'), split_out(N, C, vol(ogrid), r['y'], 'y')
        assert r['x'] in (TIGHT, 'gap') or xo.lo == 2 * C // 8
        nv.call('iunet_x2_maxpool_fwd', nd, nv.ptr(xo.t), xo.ss, xo.lo, nv.ptr(yo.t), yo.ss, yo.lo, C, N, Do, Ho, Wo, nv.stream())
        return reader(yo), [xo, yo]

    got = over_rows(run, MP_ROWS)
    gh, gl = unblocked(got['hi'], C, ogrid, 8), unblocked(got['lo'], C, ogrid, 8)
    same_value(gh.float() + gl.float(), want, 'pooled value')
    member = ((hb == gh.view(torch.int16).int().unsqueeze(-1)) & (lb == gl.view(torch.int16).int().unsqueeze(-1))).any(-1)
    verify(bool(member.all()), f'{int((~member).sum())} pooled pairs are no pair of their window')


# ---------------------------------------------------------------------------------------------------------------- 7. make8
M8_ROWS = [dict(x=TIGHT, lo_at=None, y=TIGHT), dict(x='gap', lo_at=2, y='up'), dict(x='skip', lo_at=None, y='gap'), dict(x='up', lo_at=None, y='skip'),
           dict(x=TIGHT, lo_at=2, y='gap')]


@pytest.mark.parametrize('C,grid', [pytest.param(16, (3, 5, 19), id='C16-vox285'), pytest.param(48, (1, 7, 43), id='C48-vox301')])
def test_x2m_make8(nv, C, grid):
    """The bytes are exactly e4m3(16 lo) by the CPU codec, with the lo planes C / 8 and 2 C / 8 planes behind the hi planes."""
    N, vox = 2, vol(grid)
    assert vox % 256 and vox > 256
    g = cd.gen(700 + C)
    x = torch.randn((N, C) + grid, generator=g) * torch.exp2(torch.randint(-6, 9, (N, C) + grid, generator=g).float()) / A
    hi, lo, _ = canonical_split(x)
    lo[0, 0, 0, 0, :4] = torch.tensor([0.0, -0.0, 30.0, -30.0])          # zero signs, and 16 lo beyond +-448: the conversion saturates
    want = cd.e4m3_codes(16.0 * lo)
    assert len(torch.unique(want)) > 100

    def run(r):
        xo = split_in(hi, lo, r['x'], 'x', lo_at=r['lo_at'] and r['lo_at'] * C // 8)
        assert xo.lo == (C // 8 if r['x'] in (TIGHT, 'gap') and not r['lo_at'] else 2 * C // 8)
        yo = m8_out(N, C, vox, r['y'], 'x8')
        nv.call('iunet_x2m_make8', nv.ptr(xo.t), xo.ss, xo.lo, nv.ptr(yo.t), yo.ss, C, N, *grid, nv.stream())
        return (lambda: {'m8': yo.logical()}), [xo, yo]

    got = over_rows(run, M8_ROWS)
    same_bits(unblocked(got['m8'], C, grid, 16), want, 'lo8 bytes')


# ---------------------------------------------------------------------------------------------------------------- 8. first conv
IN_DTYPES = {'f32': (0, F32), 'f16': (1, F16), 'u8': (2, U8), 'bf16': (3, torch.bfloat16)}
FIRST_GRID = {3: ((5, 9, 17), (3, 7, 13)), 2: ((17, 33), (9, 21))}          # two workgroups per axis, every second one ragged; one ragged tile
FIRST = [pytest.param(nd, cin, dt, FIRST_GRID[nd][cin % 2], id=f'{nd}d-cin{cin}-{dt}-{"x".join(map(str, FIRST_GRID[nd][cin % 2]))}')
         for nd in (2, 3) for cin in (1, 2, 3, 4) for dt in IN_DTYPES]
FIRST_ROWS = [dict(fn='x2', y=TIGHT), dict(fn='x2', y='up'), dict(fn='x2m', y='gap', y8=TIGHT, lo=True), dict(fn='x2m', y='skip', y8='up', lo=False),
              dict(fn='x2m', y='up', y8='gap', lo=True)]


@pytest.mark.parametrize('nd,cin,dt,grid', FIRST)
def test_first_conv(nv, nd, cin, dt, grid):
    """f32 / f16 / bf16 inputs hold k / 64, k in -1..1: act_scale x is the integer, the result exact in hi, lo and lo8.  u8 inputs go against
    float64 at the 3e-6 bar, their lo8 bytes by the interval rule.  The x2m form with y_lo = -1 writes no lo plane."""
    N, co = 2, 32
    code, dtype = IN_DTYPES[dt]
    tile = (4, 8, 16) if nd == 3 else (16, 32)
    assert all(s % t for s, t in zip(grid, tile))
    D, H, W = dhw(nd, grid)
    vox = vol(grid)
    if dt == 'u8':
        g = cd.gen(800 + nd + cin)
        xin = torch.randint(0, 256, (N, cin) + grid, generator=g, dtype=U8)
        w = torch.randn((co, cin) + (3,) * nd, generator=g) * (2.0 / (cin * 3 ** nd)) ** 0.5
        bn = bn_vectors(g, co)
        wf, bf = cd.fold_ref(w, bn, 1e-5, False)
        want = torch.relu(cd.conv_nd(nd)(xin.double() / 255.0, wf.double(), bf.double(), padding=1))
        assert torch.equal((xin.float() / 255).double(), (xin.double() / 255).float().double())          # torch's quotient is the correctly rounded one
        op = prep_x2(nv, nd, w, bn=bn, act_out=A, first=True)
    else:
        h, r = cd.split_exact_operator((co, cin) + (3,) * nd, 0, 810 + nd + cin)
        k, _ = cd.split_exact_input(N, cin, grid, 820 + nd + cin)
        xin = (k / A).to(dtype)
        assert torch.equal(xin.float() * A, k)
        bias = torch.randint(-4, 5, (co,), generator=cd.gen(830)).float()
        v = torch.relu(cd.split_store(cd.split_exact_ref(nd, k, torch.zeros_like(k), h, r, False), bias))
        op = prep_x2(nv, nd, h + r, bias=bias, first=True)
        same_value(op['osc'].logical(), torch.full((co,), cd.X2_ACT_OUT / cd.X2_ACT_IN), 'oscale')

    def run(r):
        xo = StridedInput(xin.reshape((N, cin, D, H, W)), device=DEVICE)
        yo = split_out(N, co, vox, r['y'], 'y', own_lo=r.get('lo', True))
        y8o = m8_out(N, co, vox, r['y8'], 'y8') if r['fn'] == 'x2m' else None
        sat = sat_word()
        tail = (nv.ptr(op['wpk'].t), nv.ptr(op['osc'].t), nv.ptr(op['bias'].t), A, N, D, H, W, cin, co, 1)
        if r['fn'] == 'x2':
            nv.call('iunet_x2_first_conv_fwd', nd, nv.ptr(xo.t), code, nv.ll_array(xo.strides), nv.ptr(yo.t), yo.ss, yo.lo, *tail, nv.stream())
        else:
            nv.call('iunet_x2m_first_conv_fwd', nd, nv.ptr(xo.t), code, nv.ll_array(xo.strides), nv.ptr(yo.t), yo.ss, yo.lo, nv.ptr(y8o.t), y8o.ss, *tail,
                    nv.ptr(sat.t), nv.stream())
        return reader(yo, y8o, sat), [xo, yo, sat] + ([y8o] if y8o is not None else []) + op['ops']

    got = over_rows(run, FIRST_ROWS)          # (the x2m rows are held to the fp16x2 form's hi and lo bits)
    if dt == 'u8':
        val = (unblocked(got['hi'].float(), co, grid, 8).double() + unblocked(got['lo'].float(), co, grid, 8).double()) / A
        rel_close(val, want, 3e-6, f'first conv {nd}-D cin {cin} u8')
        verify(cd.lo8_in_interval(unblocked(got['m8'], co, grid, 16), unblocked(got['lo'].float(), co, grid, 8)) == 0, 'lo8 bytes outside the interval of their lo words')
    else:
        exact_store(got, v, f'first conv {nd}-D cin {cin} {dt}', grid, co)


# ---------------------------------------------------------------------------------------------------------------- 9. transposed conv
CONVT = [pytest.param(nd, 2, g, cin, 32, (kc, nch), False, id=f'{nd}d-cin{cin}-kc{kc}_chunks{nch}-{"resident" if nch == 1 else "streamed"}')
         for nd, g in ((3, (3, 5, 18)), (2, (7, 21))) for cin, kc, nch in ((32, 1, 1), (64, 2, 1), (96, 1, 3), (128, 2, 2))]
CONVT += [pytest.param(3, 3, (6, 10, 40), 128, 128, (2, 2), True, id='3d-capped_68_on_64-N3-128to128-streamed'),
          pytest.param(2, 2, (33, 250), 64, 128, (2, 1), True, id='2d-capped_132_on_128-N2-64to128-resident')]
CONVT_ROWS = [dict(fn='x2', x=TIGHT, y=TIGHT), dict(fn='x2m', x='gap', y='up', y8='up', lo=True), dict(fn='x2m', x='up', y='up', y8=TIGHT, lo=False),
              dict(fn='x2', x='skip', y='up'), dict(fn='x2m', x=TIGHT, y=TIGHT, y8='gap', lo=True)]


@pytest.mark.parametrize('nd,N,grid,cin,co,branch,capped', CONVT)
def test_convT_exact(nv, nd, N, grid, cin, co, branch, capped):
    rg = regimeT(nd, N, grid, cin, co)
    assert (rg['kc'], rg['nchunks']) == branch and rg['capped'] == capped and grid[-1] % 16, rg
    if capped:
        assert rg['last_pass_partly_empty'] and (rg['want'], rg['cap']) == ((68, 64) if nd == 3 else (132, 128))
    npos = 2 ** nd
    h, r = cd.split_exact_operator((cin, co) + (2,) * nd, 1, 900 + nd + cin)
    xh, xl = cd.split_exact_input(N, cin, grid, 910 + nd + cin)
    bias = torch.randint(-4, 5, (co,), generator=cd.gen(920 + co)).float()
    v = cd.split_store(cd.split_exact_ref(nd, xh, xl, h, r, True), bias)
    op = prep_x2(nv, nd, h + r, transposed=True, bias=bias)
    assert op['kc'] == rg['kc']
    same_value(op['wv'].logical(), cd.x2_chunked_convT(h.reshape(cin, co, npos), r.reshape(cin, co, npos), op['kc']), 'the prepared operator [chunk][hi | lo]')
    same_value(op['osc'].logical(), torch.full((co,), cd.X2_ACT_OUT / cd.X2_ACT_IN), 'oscale')
    ogrid = tuple(2 * s for s in grid)
    D, H, W = dhw(nd, grid)

    def run(row):
        xo = split_in(xh, xl, row['x'], 'x')
        yo = split_out(N, co, vol(ogrid), row['y'], 'y', own_lo=row.get('lo', True))
        y8o = m8_out(N, co, vol(ogrid), row['y8'], 'y8') if row['fn'] == 'x2m' else None
        sat = sat_word()
        tail = (nv.ptr(op['wpk'].t), nv.ptr(op['osc'].t), nv.ptr(op['bias'].t), N, D, H, W, cin, co)
        if row['fn'] == 'x2':
            nv.call('iunet_x2_convT_fwd', nd, nv.ptr(xo.t), xo.ss, xo.lo, nv.ptr(yo.t), yo.ss, yo.lo, *tail, nv.stream())
        else:
            nv.call('iunet_x2m_convT_fwd', nd, nv.ptr(xo.t), xo.ss, xo.lo, nv.ptr(yo.t), yo.ss, yo.lo, nv.ptr(y8o.t), y8o.ss, *tail, nv.ptr(sat.t), nv.stream())
        return reader(yo, y8o, sat), [xo, yo, sat] + ([y8o] if y8o is not None else []) + op['ops']

    got = over_rows(run, CONVT_ROWS[:3] if capped else CONVT_ROWS)          # (the x2m rows are held to the fp16x2 form's hi and lo bits)
    exact_store(got, v, f'transposed conv {nd}-D {cin} -> {co}', ogrid, co)


# ---------------------------------------------------------------------------------------------------------------- 10. GroupNorm + ReLU
GN = [pytest.param(2, 32, 8, 315, id='N2-C32-g8-vox315'), pytest.param(3, 64, 8, 1320, id='N3-C64-g8-vox1320'),
      pytest.param(1, 256, 8, 64, id='N1-C256-g8-vox64'), pytest.param(2, 32, 4, 20001, id='N2-C32-g4-vox20001')]
GN_ROWS = [dict(fn='x2', y=TIGHT), dict(fn='x2', y='up'), dict(fn='x2', y='skip'),
           dict(fn='x2m', y=TIGHT, y8=TIGHT, lo=True), dict(fn='x2m', y='up', y8='up', lo=True), dict(fn='x2m', y='skip', y8='skip', lo=False)]


@pytest.mark.parametrize('N,C,groups,vox', GN)
def test_gn_relu(nv, N, C, groups, vox):
    """Both entry points against float64 at 2e-6 x max(1, |want|); the x2m form writes the fp16x2 form's hi bits (and lo bits where y_lo >= 0), its
    lo8 bytes obey the interval rule; the slab has exactly iunet_gn_precise_slab_bytes bytes."""
    g = cd.gen(1000 + C + vox)
    x = torch.randn((N, C, vox), generator=g) * (0.5 + torch.rand((1, C, 1), generator=g)) + 0.3 * torch.randn((1, C, 1), generator=g)
    gamma, beta = 0.5 + torch.rand(C, generator=g), 0.3 * torch.randn(C, generator=g)
    hi, lo, xq = canonical_split(x)
    want = F.relu(F.group_norm(xq, groups, gamma.double(), beta.double(), eps=1e-5))
    nbytes = int(nv.lib().iunet_gn_precise_slab_bytes(N, C, vox))
    assert nbytes == N * C * min(max(ceil(vox, 8192), 1), 512) * 2 * 8          # double [N][C][parts of 8192 voxels][2]

    def run(r):
        xo = split_in(hi, lo, TIGHT, 'x')
        yo = split_out(N, C, vox, r['y'], 'y', own_lo=r.get('lo', True))
        y8o = m8_out(N, C, vox, r['y8'], 'y8') if r['fn'] == 'x2m' else None
        go, bo, sat = vec(gamma, 'gamma'), vec(beta, 'beta'), sat_word()
        slab, sc, sh = scratch(nbytes, 'slab', U8), scratch(N * C, 'scale'), scratch(N * C, 'shift')
        tail = (nv.ptr(go.t), nv.ptr(bo.t), groups, 1e-5, A, nv.ptr(slab.t), nv.ptr(sc.t), nv.ptr(sh.t), C, N, vox, nv.ptr(sat.t), nv.stream())
        if r['fn'] == 'x2':
            nv.call('iunet_x2_gn_relu_fwd', nv.ptr(xo.t), xo.ss, xo.lo, nv.ptr(yo.t), yo.ss, yo.lo, *tail)
        else:
            nv.call('iunet_x2m_gn_relu_fwd', nv.ptr(xo.t), xo.ss, xo.lo, nv.ptr(yo.t), yo.ss, yo.lo, nv.ptr(y8o.t), y8o.ss, *tail)
        return reader(yo, y8o, sat), [xo, yo, go, bo, sat, slab, sc, sh] + ([y8o] if y8o is not None else [])

    got = m8 = over_rows(run, GN_ROWS)          # (the x2m rows are held to the fp16x2 form's hi and lo bits)
    sp = (vox,)
    val = (unblocked(got['hi'].float(), C, sp, 8).double() + unblocked(got['lo'].float(), C, sp, 8).double()) / A
    err, bar = float((val - want).abs().max()), 2e-6 * max(1.0, float(want.abs().max()))
    print(f'[GroupNorm N{N} C{C} g{groups} vox{vox}] max err {err:.2e} (bar {bar:.1e})')
    verify(err <= bar, f'GroupNorm: max err {err:.3e} over the bar {bar:.3e}')
    verify(cd.lo8_in_interval(unblocked(m8['m8'], C, sp, 16), unblocked(m8['lo'].float(), C, sp, 8)) == 0, 'lo8 bytes outside the interval of their lo words')
    assert 0.2 < float((want == 0).float().mean()) < 0.8


# ---------------------------------------------------------------------------------------------------------------- 11. the first stage in one launch
@pytest.mark.parametrize('N,grid,dt,pool', [pytest.param(2, (34, 66), 'u8', True, id='pool-u8-N2-34x66'), pytest.param(3, (17, 35), 'f16', False, id='nopool-f16-N3-17x35')])
def test_first_stage_is_first_conv_plus_conv_bit_for_bit(nv, N, grid, dt, pool):
    """iunet_x2m_first_stage_fwd against iunet_x2m_first_conv_fwd + iunet_x2m_conv_fwd / _conv_pool_fwd: every word, with the fused launch's
    outputs at the gap and skip placements and the image a strided view."""
    H, W = grid
    c, vox, pv = 32, H * W, (H // 2) * (W // 2)
    code, dtype = IN_DTYPES[dt]
    g = cd.gen(1100 + N)
    xin = torch.randint(0, 256, (N, 1, 1, H, W), generator=g, dtype=U8) if dt == 'u8' else torch.rand((N, 1, 1, H, W), generator=g).to(dtype)
    f = prep_x2(nv, 2, torch.randn((c, 1, 3, 3), generator=g) * (2.0 / 9) ** 0.5, bn=bn_vectors(g, c), act_out=A, first=True)
    op = prep_x2m(nv, 2, torch.randn((c, c, 3, 3), generator=g) * (2.0 / (c * 9)) ** 0.5, bn_vectors(g, c, -0.2))

    def run(fused):
        place, place8 = ('gap', 'skip') if fused else (TIGHT, TIGHT)
        xo = StridedInput(xin, device=DEVICE)
        yo, y8o = split_out(N, c, vox, place, 'y', own_lo=False), m8_out(N, c, vox, place8, 'y8')
        po, p8o = (split_out(N, c, pv, place8, 'py', own_lo=False), m8_out(N, c, pv, place, 'py8')) if pool else (None, None)
        sat = sat_word()
        pargs = (nv.ptr(po.t), po.ss, nv.ptr(p8o.t), p8o.ss) if pool else (None, 0, None, 0)
        wargs = (nv.ptr(op['w16'].t), nv.ptr(op['w8'].t), nv.ptr(op['osc'].t), nv.ptr(op['bias'].t))
        ops = [xo, yo, y8o, sat] + ([po, p8o] if pool else [])
        if fused:
            nv.call('iunet_x2m_first_stage_fwd', nv.ptr(xo.t), code, nv.ll_array(xo.strides), nv.ptr(f['wpk'].t), nv.ptr(f['osc'].t), nv.ptr(f['bias'].t), A,
                    nv.ptr(yo.t), yo.ss, -1, nv.ptr(y8o.t), y8o.ss, *pargs, *wargs, N, H, W, nv.ptr(sat.t), nv.stream())
        else:
            ao, a8o = split_out(N, c, vox, TIGHT, 'a', own_lo=False), m8_out(N, c, vox, TIGHT, 'a8')
            ops += [ao, a8o]
            nv.call('iunet_x2m_first_conv_fwd', 2, nv.ptr(xo.t), code, nv.ll_array(xo.strides), nv.ptr(ao.t), ao.ss, -1, nv.ptr(a8o.t), a8o.ss, nv.ptr(f['wpk'].t),
                    nv.ptr(f['osc'].t), nv.ptr(f['bias'].t), A, N, 1, H, W, 1, c, 1, nv.ptr(sat.t), nv.stream())
            if pool:
                nv.call('iunet_x2m_conv_pool_fwd', 2, nv.ptr(ao.t), ao.ss, nv.ptr(a8o.t), a8o.ss, nv.ptr(yo.t), yo.ss, -1, nv.ptr(y8o.t), y8o.ss, *pargs, *wargs,
                        N, 1, H, W, c, c, 2, nv.ptr(sat.t), nv.stream())
            else:
                nv.call('iunet_x2m_conv_fwd', 2, nv.ptr(ao.t), ao.ss, nv.ptr(a8o.t), a8o.ss, nv.ptr(yo.t), yo.ss, -1, nv.ptr(y8o.t), y8o.ss, *wargs,
                        N, 1, H, W, c, c, 2, nv.ptr(sat.t), nv.stream())

        def read():
            out = {'hi': yo.logical()[0], 'm8': y8o.logical(), 'sat': sat_of(sat)}
            if pool:
                out.update({'pooled hi': po.logical()[0], 'pooled m8': p8o.logical()})
            return out
        return read, ops + f['ops'] + op['ops']

    got = over_rows(run, [False, True])
    verify(float(got['hi'].float().abs().max()) > 0 and float((got['hi'].float() == 0).float().mean()) < 0.9, 'the stage output is all but zero')


# ---------------------------------------------------------------------------------------------------------------- 12. the range flag
def saturated(got, what):
    """Data saturation: finite words, a hi maximum of 65504 and sat == 0x7bff."""
    hi = got['hi'].float()
    verify(bool(torch.isfinite(hi).all()) and ('lo' not in got or bool(torch.isfinite(got['lo'].float()).all())), f'{what}: a stored word is not finite')
    verify(float(hi.abs().max()) == 65504.0 and got['sat'] == 0x7bff, f'{what}: hi maximum {float(hi.abs().max())}, range flag {got["sat"]:#x}')


def read_all(yo, y8o, sat):
    r = reader(yo, y8o, sat)

    def go(ops):
        sync()
        for o in ops:
            o.check()
        return r()
    return go


def test_range_flag_x2_conv(nv):
    nd, N, grid, ci, co = 3, 1, (4, 8, 16), 32, 32
    g = cd.gen(1200)
    w = torch.randn((co, ci, 3, 3, 3), generator=g).abs() * 0.05
    hi, lo, _ = canonical_split(torch.rand((N, ci) + grid, generator=g) * 600.0)          # sums far beyond 65504 / act_scale
    op = prep_x2(nv, nd, w, bias=torch.zeros(co), act_out=A)
    xo, yo, sat = split_in(hi, lo, 'up', 'x'), split_out(N, co, vol(grid), 'gap', 'y'), sat_word()
    x2_conv_call(nv, nd, xo, yo, op, N, grid, ci, co, 0, sat)
    saturated(read_all(yo, None, sat)([xo, yo, sat]), 'fp16x2 conv')


def test_range_flag_x2m_first_conv(nv):
    nd, N, grid, co = 2, 1, (17, 33), 32
    g = cd.gen(1210)
    op = prep_x2(nv, nd, torch.randn((co, 1, 3, 3), generator=g).abs() + 0.5, bias=torch.zeros(co), act_out=A, first=True)
    xo = StridedInput(torch.rand((N, 1, 1) + grid, generator=g) * 4000.0 + 500.0, device=DEVICE)
    yo, y8o, sat = split_out(N, co, vol(grid), 'skip', 'y'), m8_out(N, co, vol(grid), 'gap', 'y8'), sat_word()
    nv.call('iunet_x2m_first_conv_fwd', nd, nv.ptr(xo.t), 0, nv.ll_array(xo.strides), nv.ptr(yo.t), yo.ss, yo.lo, nv.ptr(y8o.t), y8o.ss, nv.ptr(op['wpk'].t),
            nv.ptr(op['osc'].t), nv.ptr(op['bias'].t), A, N, 1, *grid, 1, co, 1, nv.ptr(sat.t), nv.stream())
    saturated(read_all(yo, y8o, sat)([xo, yo, y8o, sat]), 'x2m first conv')


def test_range_flag_x2m_convT(nv):
    nd, N, grid, ci, co = 2, 1, (5, 18), 64, 32
    g = cd.gen(1220)
    op = prep_x2(nv, nd, torch.randn((ci, co, 2, 2), generator=g).abs() * 0.2, transposed=True, bias=torch.zeros(co), act_out=A)
    hi, lo, _ = canonical_split(torch.rand((N, ci) + grid, generator=g) * 600.0)
    xo, yo, y8o, sat = split_in(hi, lo, TIGHT, 'x'), split_out(N, co, 4 * vol(grid), 'up', 'y'), m8_out(N, co, 4 * vol(grid), 'up', 'y8'), sat_word()
    nv.call('iunet_x2m_convT_fwd', nd, nv.ptr(xo.t), xo.ss, xo.lo, nv.ptr(yo.t), yo.ss, yo.lo, nv.ptr(y8o.t), y8o.ss, nv.ptr(op['wpk'].t), nv.ptr(op['osc'].t),
            nv.ptr(op['bias'].t), N, 1, *grid, ci, co, nv.ptr(sat.t), nv.stream())
    saturated(read_all(yo, y8o, sat)([xo, yo, y8o, sat]), 'x2m transposed conv')


def test_range_flag_x2m_gn(nv):
    N, C, groups, vox = 1, 32, 8, 315
    g = cd.gen(1230)
    hi, lo, _ = canonical_split(torch.randn((N, C, vox), generator=g))
    go, bo = vec(torch.full((C,), 4000.0), 'gamma'), vec(torch.zeros(C), 'beta')          # 4000 x a unit-variance value x 64: beyond 65504
    xo, yo, y8o, sat = split_in(hi, lo, TIGHT, 'x'), split_out(N, C, vox, 'up', 'y'), m8_out(N, C, vox, 'up', 'y8'), sat_word()
    nbytes = int(nv.lib().iunet_gn_precise_slab_bytes(N, C, vox))
    slab, sc, sh = scratch(nbytes, 'slab', U8), scratch(N * C, 'scale'), scratch(N * C, 'shift')
    nv.call('iunet_x2m_gn_relu_fwd', nv.ptr(xo.t), xo.ss, xo.lo, nv.ptr(yo.t), yo.ss, yo.lo, nv.ptr(y8o.t), y8o.ss, nv.ptr(go.t), nv.ptr(bo.t), groups, 1e-5, A,
            nv.ptr(slab.t), nv.ptr(sc.t), nv.ptr(sh.t), C, N, vox, nv.ptr(sat.t), nv.stream())
    saturated(read_all(yo, y8o, sat)([xo, yo, y8o, sat, slab, sc, sh]), 'x2m GroupNorm')
