"""The decoders' gather-GEMM kernels (csrc/gather_gemm.h under the policies of linknet.hip, deeplab.hip and segformer.hip, and the small
kernels next to them) across launch geometry x dtype x nd x buffer placement, through the C ABI.

The grids are the smallest that leave the single-workgroup regime and are ragged everywhere: more than one workgroup along x with a wave
walking several column tiles, column tiles that straddle two samples, a last tile of one column, more than one row group with a short
last one, two weight-gradient splits (and the split count halved under the 8 Mi-float slab cap), K and channel tails.  Every operand is
allocated through tests/arena.py, and each case asserts the four points of tests/test_gpu_kernel_matrix.py:
  1. the tight result bit for bit against torch on the CPU.  All data are small integers (activations and gradients -2..2, operators
     -1..1, biases, skips and per-sample biases -3..3, prologue scales 1 or 2 with integer shifts, alpha and psb_scale powers of two;
     Segformer's resampling weights are dyadic), so every fp32 partial sum is exact in any order: fp32 outputs (dW, G, y of the fp32
     forms, statistics rows summed in float64) equal the reference, 16-bit outputs equal the reference rounded once to the storage
     type.  What makes this legitimate is asserted on the reference alone (check_* below; tests/test_decoder_matrix_cpu.py evaluates the
     same conditions for every case without a GPU): every partial sum is bounded by the conv of |x| with |w| < 2^24, the sum of squares
     of each statistics row's share of columns is below 2^24 units of the data's resolution, resampled operands survive the rounding;
  2. stride independence: two further placement rows give the bits of the tight run;
  3. no stray write and no modified input: Operand.check() on every operand, the operator, the parameter vectors and scratch of exactly
     the size the library reports included;
  4. no unwritten output: outputs, statistics and slabs start as the NaN sentinel.
Each case also asserts the launch geometry it is named after, restated here from the launcher, against what the library reports.
Batch size 3 except in the capped launch.  Needs an MI355X: run with -m gpu."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.arena import SENTINEL, Operand, bits, pointer_table, scratch, source_tables
from tests.test_gpu_kernel_matrix import DT, F32, TIGHT, dev32, dhw, gen, ints, nv, out, over_placements, planar, put  # noqa: F401 (nv: fixture)

pytestmark = pytest.mark.gpu

N3 = 3
CODE = {torch.float16: 0, torch.bfloat16: 1, torch.float32: 2}
EXACT32 = 2 ** 24          # integers up to here are exact in fp32


# ---------------------------------------------------------------------------------------------------------------- launch arithmetic
def gg_fwd_blocks(cols, ngroups):
    """gather_gemm.h: workgroups along x of the forward GEMM; ngroups = row groups x classes."""
    tiles = -(-cols // 16)
    return max(1, min(-(-tiles // 16), -(-2048 // ngroups), 1024))


def gg_fwd_share(cols, blocks):
    """Column tiles per workgroup (per_block) and the tile count of each workgroup."""
    tiles = -(-cols // 16)
    per = -(-tiles // blocks)
    return per, [max(0, min(tiles, (b + 1) * per) - b * per) for b in range(blocks)]


def gg_wgrad_splits(cols, per_split_floats):
    """gather_gemm.h: splits of the LDS-staged weight gradient (chunks of 32 columns, 16 chunks per split at least, 8 Mi floats of slab)."""
    s = max(1, min(64, -(-(-(-cols // 32)) // 16)))
    while s > 1 and s * per_split_floats > 8 << 20:
        s >>= 1
    return s


def lk_classes(nd, kind):
    return 2 ** nd if kind == 1 else 1


def lk_taps(nd, kind):
    return 1 if kind == 0 else 2 ** nd if kind == 1 else 4 ** nd


def lk_wgrad_splits(nd, kind, cols, cin, cout):
    """linknet.hip: 2048 columns per split at least, the same 8 Mi-float cap over classes x splits."""
    s = max(1, min(64, -(-cols // 2048)))
    while s > 1 and lk_classes(nd, kind) * s * cout * lk_taps(nd, kind) * cin > 8 << 20:
        s >>= 1
    return s


def dl_kept(nd, rate, sp):
    """deeplab.hip, dl_add_taps: the kernel indices (kd * 3 + kh) * 3 + kw (2-D: kh * 3 + kw) a dilated conv keeps on the grid sp."""
    if rate == 0:
        return [0]
    D, H, W = dhw(nd, sp)
    keep = []
    for kd in range(3 if nd == 3 else 1):
        for kh in range(3):
            for kw in range(3):
                od, oh, ow = ((kd - 1) * rate if nd == 3 else 0), (kh - 1) * rate, (kw - 1) * rate
                if abs(od) < D and abs(oh) < H and abs(ow) < W:
                    keep.append((kd * 3 + kh) * 3 + kw if nd == 3 else kh * 3 + kw)
    return keep


def sf_blocks(cols):
    return -(-cols // 64)          # SF_COLS = 64 voxels per workgroup, all rows


def vox(sp):
    return int(np.prod(sp))


def up2(sp):
    return tuple(2 * s for s in sp)


def bc(v, nd):
    return v.view(1, -1, *([1] * nd))


def prologue(g, C, top=5):
    """scale 1 or 2 and an integer shift: relu(scale x + shift) of x in -2..2 is an integer in 0..top (5: shift -1..1; 3: Segformer)."""
    scale = 2.0 ** torch.randint(0, 2, (C,), generator=g).float()
    shift = ints(g, -1, 1, (C,))
    if top == 3:
        shift = shift - 2 * (scale == 2).float()
    return scale, shift


def act_of(x, scale, shift):
    nd = x.dim() - 2
    return F.relu(bc(scale, nd).to(x.dtype) * x + bc(shift, nd).to(x.dtype))


# ---------------------------------------------------------------------------------------------------------------- assertions
def assert_rounded(got, ref, dtype, what):
    """A 16-bit output against the exact reference rounded once to the storage type; an unwritten element (a NaN) differs."""
    want = ref.to(dtype).float()
    bad = got != want
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} of {bad.numel()} elements differ, the first at {tuple(bad.nonzero()[0].tolist())}'


def assert_same32(got, ref, what):
    bad = got.double() != ref.double()
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} of {bad.numel()} elements differ, the first at {tuple(bad.nonzero()[0].tolist())}'


def assert_stats(st, parts, cout, ref, what):
    """[parts][Cout][2] rows, summed in float64, against the sums of the exact reference."""
    dims = [0] + list(range(2, ref.dim()))
    s = st.logical().reshape(parts, cout, 2).double().sum(0)
    assert torch.equal(s[:, 0], ref.double().sum(dims)), f'{what}: sums differ'
    assert torch.equal(s[:, 1], (ref.double() ** 2).sum(dims)), f'{what}: sums of squares differ'


def check_partial_sums(bound, what):
    """On the reference alone: every partial sum of the accumulation, in any order, is an integer (or a multiple of the data's
    resolution, `bound` given in those units) below 2^24."""
    assert float(bound) < EXACT32, f'{what}: partial sums reach {float(bound)}, not exact in fp32'


def check_row_squares(ref, blocks_cols, unit, what):
    """On the reference alone: the statistics are exact.  ref [N, C, *sp] in units of `unit`; a statistics row holds the sum over at most
    `blocks_cols` consecutive columns (n, voxel) of one channel; its sum of squares in units of unit^2 stays below 2^24 (non-negative
    terms: every partial sum is bounded by the total), and so does |sum|.  The rows are summed in float64."""
    N, C = ref.shape[:2]
    v = (ref.double() / unit).reshape(N, C, -1).permute(1, 0, 2).reshape(C, -1)
    sq = (v * v).cumsum(1)
    sq = torch.cat([torch.zeros(C, 1, dtype=sq.dtype), sq], 1)
    n = sq.shape[1] - 1
    lo = torch.arange(0, n, blocks_cols)
    hi = torch.clamp(lo + blocks_cols, max=n)
    worst = (sq[:, hi] - sq[:, lo]).max().item()
    assert worst < EXACT32, f'{what}: a statistics row sums squares to {worst} units, not exact in fp32'


# ================================================================================================================ LinkNet
# Column grids (N 3).  gg_fwd_blocks: tiles = ceil(cols / 16), blocks = min(ceil(tiles / 16), ceil(2048 / (row groups x classes)), 1024).
#   G2 = 13 x 23   299 voxels, 897 columns, 57 tiles (the last holds 1 column; 299 % 16 = 11: tiles straddle samples) -> 4 blocks, per_block 15:
#                  15, 15, 15, 12 tiles, a wave walks up to 4 tiles
#   G3 = 3 x 7 x 13  273 voxels, 819 columns, 52 tiles (the last holds 3 columns) -> 4 blocks of 13 tiles
# For kinds 1 and 2 the column grid is the coarse one (kind 1: the input grid, y on 2x; kind 2: the output grid, x on 2x).
# (Cin, Cout) of the launch: (16, 48) K below one 32-wide step at kind 0, one row group of ntile 3; (48, 80) a K tail inside the second
# step, two row groups, the second with ntile 1; (64, 128) two full row groups.
G2, G3 = (13, 23), (3, 7, 13)
GRID = {2: G2, 3: G3}
LK_CH = [(16, 48), (48, 80), (64, 128)]
LK_FWD = [(kind, nd, ci, co) for kind in (0, 1, 2) for nd in (2, 3) for ci, co in LK_CH]
LK_ROWS = [None, {'x': 'gap', 'y': 'upper', 'skip': 'gap'}, {'x': 'lower', 'y': 'gap', 'skip': 'upper'}]


def lk_grids(kind, sp):
    """(input grid, output grid) of a launch whose column grid is sp."""
    return (sp, sp) if kind == 0 else (sp, up2(sp)) if kind == 1 else (up2(sp), sp)


def lk_op(kind, nd, x, w):
    """kind 0: 1x1 conv (w [Cout][Cin]); 1: ConvTranspose k4 s2 p1 (w [Cin][Cout][4^d]); 2: its data gradient, the strided conv (w [Cout][Cin][4^d]
    of the launch's channels)."""
    conv, convT = (F.conv2d, F.conv_transpose2d) if nd == 2 else (F.conv3d, F.conv_transpose3d)
    if kind == 0:
        return conv(x, w.view(*w.shape[:2], *([1] * nd)))
    if kind == 1:
        return convT(x, w, stride=2, padding=1)
    return conv(x, w, stride=2, padding=1)


def lk_class_view(t, nd, cls):
    """The output voxels of parity class cls of a kind-1 launch, in the order of its columns."""
    pw, ph, pd = cls & 1, (cls >> 1) & 1, (cls >> 2) & 1
    return t[..., ph::2, pw::2] if nd == 2 else t[..., pd::2, ph::2, pw::2]


def lk_wshape(kind, nd, cin, cout):
    return (cout, cin) if kind == 0 else (cin, cout) + (4,) * nd if kind == 1 else (cout, cin) + (4,) * nd


@functools.lru_cache(maxsize=None)
def lk_data(kind, nd, N, sp, cin, cout, real=torch.float64):
    g = gen(2000 + 100 * kind + 10 * nd + cin)
    isp, osp = lk_grids(kind, sp)
    d = dict(x=ints(g, -2, 2, (N, cin) + isp), w=ints(g, -1, 1, lk_wshape(kind, nd, cin, cout)), bias=ints(g, -3, 3, (cout,)),
             skip=ints(g, -3, 3, (N, cout) + osp))
    d['scale'], d['shift'] = prologue(g, cin)
    d['act'] = act_of(d['x'], d['scale'], d['shift'])
    w = d['w'].to(real)
    d['raw'] = lk_op(kind, nd, d['x'].to(real), w)
    if kind != 2:
        d['raw_act'] = lk_op(kind, nd, d['act'].to(real), w)
        d['epi'] = F.relu(d['raw'] + bc(d['bias'], nd).to(real)) + d['skip'].to(real)
    d['bound'] = lk_op(kind, nd, d['act'].to(real), w.abs()).max().item() + 6          # |x| <= act's range; bias and skip on top
    return d


def lk_fwd_geometry(kind, nd, N, sp, cout):
    cols = N * vox(sp)
    groups = -(-cout // 64)
    blocks = gg_fwd_blocks(cols, groups * lk_classes(nd, kind))
    return cols, groups, blocks


def check_lk_fwd(kind, nd, N, sp, cin, cout, real=torch.float64):
    d = lk_data(kind, nd, N, sp, cin, cout, real)
    cols, groups, blocks = lk_fwd_geometry(kind, nd, N, sp, cout)
    per, _ = gg_fwd_share(cols, blocks)
    check_partial_sums(d['bound'], 'lk fwd')
    stats_of = d['raw'] if kind == 2 else d['raw_act']
    for cls in range(lk_classes(nd, kind)):          # a row of class c holds per * 16 columns of that class's output voxels
        check_row_squares(lk_class_view(stats_of, nd, cls) if kind == 1 else stats_of, per * 16, 1.0, 'lk fwd')
    return d


def lk_pack(nv, dtype, kind, nd, w, cin, cout):
    """The operator of a launch with (cin, cout) channels, packed by the library: pack kinds 0 (1x1), 2 (convT), 3 (convT data gradient of a
    transposed conv whose Cin is the launch's Cout)."""
    pk, pco, pci = ((0, cout, cin), (2, cout, cin), (3, cin, cout))[kind]
    wo = dev32(w, 'w')
    wpk = scratch(nv.lib().iunet_lk_pack_elems(nd, pk, pco, pci), dtype, name='wpk')
    nv.call('iunet_lk_pack', CODE[dtype], nd, pk, nv.ptr(wo.t), None, None, None, None, 0.0, nv.ptr(wpk.t), None, pco, pci, nv.stream())
    return wo, wpk


def lk_fwd_run(nv, dtype, kind, nd, N, sp, cin, cout, d, form, pl):
    """form 'raw_act': raw output + statistics rows through the input activation; 'raw': the same without it; 'epi': + bias, ReLU, + skip."""
    D, H, W = dhw(nd, sp)
    isp, osp = lk_grids(kind, sp)
    xo = put(d['x'], dtype, pl['x'], 'x')
    wo, wpk = lk_pack(nv, dtype, kind, nd, d['w'], cin, cout)
    yo = out(N, cout, vox(osp), dtype, pl['y'], 'y')
    ops, outs = [xo, wo, wpk, yo], {'y': yo}
    sc = sh = bo = so = st = None
    if form == 'raw_act':
        sc, sh = dev32(d['scale'], 'in_scale'), dev32(d['shift'], 'in_shift')
        ops += [sc, sh]
    if form == 'epi':
        bo, so = dev32(d['bias'], 'bias'), put(d['skip'], dtype, pl['skip'], 'skip')
        ops += [bo, so]
    else:
        st = scratch(nv.lib().iunet_lk_stats_parts(nd, kind, N, D, H, W, cout) * cout * 2, name='stats')          # every row is written
        ops.append(st)
        outs['stats'] = st
    P = lambda o: None if o is None else nv.ptr(o.t)
    nv.call('iunet_lk_conv_fwd', CODE[dtype], nd, kind, P(xo), xo.ss, P(yo), yo.ss, P(wpk), P(sc), P(sh), P(bo), P(so), 0 if so is None else so.ss,
            P(st), 1 if form == 'epi' else 0, N, D, H, W, cin, cout, nv.stream())
    return outs, ops


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('kind,nd,cin,cout', LK_FWD)
def test_lk_conv_fwd(nv, dt, kind, nd, cin, cout):
    """gg_fwd_kernel under LkGather<nd, kind>: 4 workgroups along x (per_block 15 / 13, the last short in 2-D), row groups with co0 > 0 and
    ntile 1 (Cout 80), the per-class operator rows cls * Cout + co0 (kind 1), statistics rows of every (class, block)."""
    dtype, N, sp = DT[dt], N3, GRID[nd]
    D, H, W = dhw(nd, sp)
    d = check_lk_fwd(kind, nd, N, sp, cin, cout)
    cols, groups, blocks = lk_fwd_geometry(kind, nd, N, sp, cout)
    parts = nv.lib().iunet_lk_stats_parts(nd, kind, N, D, H, W, cout)
    assert parts == blocks * lk_classes(nd, kind) and blocks == 4, (parts, blocks)
    per, share = gg_fwd_share(cols, blocks)
    assert share == ([15, 15, 15, 12] if nd == 2 else [13] * 4) and per > 8          # a wave walks more than two tiles
    assert groups == (1 if cout == 48 else 2) and (cout - 64 * (groups - 1)) // 16 == {48: 3, 80: 1, 128: 4}[cout]
    assert (vox(sp) % 16 != 0) and cols % 16 == (1 if nd == 2 else 3)
    osp = lk_grids(kind, sp)[1]
    forms = ['raw'] if kind == 2 else ['raw_act', 'epi']
    for form in forms:
        res = over_placements(nv, lambda pl: lk_fwd_run(nv, dtype, kind, nd, N, sp, cin, cout, d, form, pl), LK_ROWS)
        assert_rounded(planar(res['y'], cout, osp), d[form], dtype, f'lk y ({form})')
        if form != 'epi':
            assert_stats(res['stats'], parts, cout, d[form], f'lk statistics ({form})')


# The capped launch: kind 1, 2-D, N 1, 129 x 128, Cin 16, Cout 512: 16 512 columns, 1 032 tiles; 8 row groups x 4 classes = 32 cap the blocks
# at 2048 / 32 = 64 (65 uncapped), per_block = ceil(1032 / 64) = 17, so blocks 0..60 own the tiles and blocks 61..63 own none: they still
# write their zero statistics rows (iunet_lk_stats_parts = 256 rows).  ~34 M output elements: once, f16, tight.
CAP = dict(kind=1, nd=2, N=1, sp=(129, 128), cin=16, cout=512)


def test_lk_conv_fwd_capped(nv):
    dtype = torch.float16
    kind, nd, N, sp, cin, cout = (CAP[k] for k in ('kind', 'nd', 'N', 'sp', 'cin', 'cout'))
    D, H, W = dhw(nd, sp)
    d = check_lk_fwd(kind, nd, N, sp, cin, cout, torch.float32)
    cols, groups, blocks = lk_fwd_geometry(kind, nd, N, sp, cout)
    parts = nv.lib().iunet_lk_stats_parts(nd, kind, N, D, H, W, cout)
    per, share = gg_fwd_share(cols, blocks)
    assert (parts, blocks, groups, per) == (256, 64, 8, 17) and -(-(-(-cols // 16)) // 16) == 65, (parts, blocks, groups, per)
    assert share[60] == 12 and share[61:] == [0, 0, 0]
    res = over_placements(nv, lambda pl: lk_fwd_run(nv, dtype, kind, nd, N, sp, cin, cout, d, 'raw_act', pl), [{'x': TIGHT, 'y': TIGHT, 'skip': TIGHT}])
    assert_rounded(planar(res['y'], cout, up2(sp)), d['raw_act'], dtype, 'capped lk y')
    rows = res['stats'].logical().reshape(4, blocks, cout, 2)          # [class][block]
    assert torch.equal(bits(rows[:, 61:].contiguous()), torch.zeros_like(bits(rows[:, 61:].contiguous()))), 'a workgroup without tiles must write +0 rows'
    assert bool((rows[:, :61, :, 1] > 0).all())
    assert_stats(res['stats'], parts, cout, d['raw_act'], 'capped lk statistics')


# iunet_lk_wgrad (lk_wgrad_kernel + lk_wgrad_reduce_kernel): splits = min(ceil(cols / 2048), 64), halved while classes x splits x Cout x K > 8 Mi
#   L2 = 23 x 31   713 voxels, 2 139 columns -> 2 splits; 67 steps of 32 columns split 34 / 33, the last step holds 27 columns
#   L3 = 7 x 9 x 11  693 voxels, 2 079 columns -> 2 splits; 65 steps split 33 / 32, the last step holds 31 columns
#   the halving loop: kind 1, 2-D, 37 x 37, Cin = Cout = 512: 4 107 columns -> 3 splits, 4 x 3 x 512 x 2048 = 12 Mi > 8 Mi -> 1
L2, L3 = (23, 31), (7, 9, 11)
LK_WGRAD = [(kind, nd, ci, co) for kind in (0, 1) for nd in (2, 3) for ci, co in ((16, 48), (48, 16))]
LKW_ROWS = [None, {'x': 'gap', 'dy': 'upper'}, {'x': 'lower', 'dy': 'gap'}]
LK_HALVED = dict(kind=1, nd=2, N=3, sp=(37, 37), cin=512, cout=512)
ALPHA = 0.5


@functools.lru_cache(maxsize=None)
def lk_wgrad_data(kind, nd, N, sp, cin, cout):
    g = gen(2100 + 100 * kind + 10 * nd + cin)
    d = dict(x=ints(g, -2, 2, (N, cin) + sp), dy=ints(g, -2, 2, (N, cout) + lk_grids(kind, sp)[1]))
    d['scale'], d['shift'] = prologue(g, cin)
    d['act'] = act_of(d['x'], d['scale'], d['shift'])
    return d


@functools.lru_cache(maxsize=None)
def lk_wgrad_ref(kind, nd, N, sp, cin, cout, real=torch.float64):
    """alpha dW by autograd (fp32 for the large case: integer sums below 2^24 are exact in fp32 in any order too)."""
    d = lk_wgrad_data(kind, nd, N, sp, cin, cout)
    w = torch.zeros(lk_wshape(kind, nd, cin, cout), dtype=real, requires_grad=True)
    lk_op(kind, nd, d['act'].to(real), w).backward(d['dy'].to(real))
    return ALPHA * w.grad


def check_lk_wgrad(kind, nd, N, sp, cin, cout):
    d = lk_wgrad_data(kind, nd, N, sp, cin, cout)
    check_partial_sums(N * vox(lk_grids(kind, sp)[1]) * d['dy'].abs().max().item() * d['act'].max().item(), 'lk wgrad')          # sum |dy| |act| over every column
    return d


def lk_wgrad_run(nv, dtype, kind, nd, N, sp, cin, cout, d, pl):
    D, H, W = dhw(nd, sp)
    xo, dyo = put(d['x'], dtype, pl['x'], 'x'), put(d['dy'], dtype, pl['dy'], 'dy')
    sc, sh = dev32(d['scale'], 'x_scale'), dev32(d['shift'], 'x_shift')
    slab = scratch(nv.lib().iunet_lk_wgrad_slab_floats(nd, kind, N, D, H, W, cin, cout), name='slab')
    dW = scratch(int(np.prod(lk_wshape(kind, nd, cin, cout))), name='dW')
    nv.call('iunet_lk_wgrad', CODE[dtype], nd, kind, nv.ptr(xo.t), xo.ss, nv.ptr(dyo.t), dyo.ss, nv.ptr(sc.t), nv.ptr(sh.t), nv.ptr(slab.t), nv.ptr(dW.t),
            ALPHA, N, D, H, W, cin, cout, nv.stream())
    return {'dW': dW}, [xo, dyo, sc, sh, slab, dW]


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('kind,nd,cin,cout', LK_WGRAD)
def test_lk_wgrad(nv, dt, kind, nd, cin, cout):
    """Two splits: the slab's split stride (class x splits + split), the ordered reduce over both and its scatter into the parameter's layout."""
    dtype, N, sp = DT[dt], N3, (L2 if nd == 2 else L3)
    D, H, W = dhw(nd, sp)
    d = check_lk_wgrad(kind, nd, N, sp, cin, cout)
    cols, K = N * vox(sp), lk_taps(nd, kind) * cin
    splits = nv.lib().iunet_lk_wgrad_slab_floats(nd, kind, N, D, H, W, cin, cout) // (lk_classes(nd, kind) * cout * K)
    assert splits == lk_wgrad_splits(nd, kind, cols, cin, cout) == 2
    steps = -(-cols // 32)
    assert (steps, -(-steps // 2), cols % 32) == ((67, 34, 27) if nd == 2 else (65, 33, 31))
    res = over_placements(nv, lambda pl: lk_wgrad_run(nv, dtype, kind, nd, N, sp, cin, cout, d, pl), LKW_ROWS)
    ref = lk_wgrad_ref(kind, nd, N, sp, cin, cout)
    assert_same32(res['dW'].logical().reshape(ref.shape), ref, 'lk dW')


def test_lk_wgrad_splits_halved(nv):
    dtype = torch.float16
    kind, nd, N, sp, cin, cout = (LK_HALVED[k] for k in ('kind', 'nd', 'N', 'sp', 'cin', 'cout'))
    D, H, W = dhw(nd, sp)
    d = check_lk_wgrad(kind, nd, N, sp, cin, cout)
    cols, K = N * vox(sp), lk_taps(nd, kind) * cin
    splits = nv.lib().iunet_lk_wgrad_slab_floats(nd, kind, N, D, H, W, cin, cout) // (lk_classes(nd, kind) * cout * K)
    assert -(-cols // 2048) == 3 and 4 * 3 * cout * K > 8 << 20 and splits == lk_wgrad_splits(nd, kind, cols, cin, cout) == 1
    res = over_placements(nv, lambda pl: lk_wgrad_run(nv, dtype, kind, nd, N, sp, cin, cout, d, pl), [None, {'x': 'gap', 'dy': 'upper'}])
    ref = lk_wgrad_ref(kind, nd, N, sp, cin, cout, torch.float32)
    assert_same32(res['dW'].logical().reshape(ref.shape), ref, 'lk dW, splits halved')


# iunet_lk_f32_conv_fwd (gg_f32_kernel under LkGather): one column tile per wave, grid x = ceil(tiles / 4) = 15 (G2) / 13 (G3); (48, 80): K = 48
# (kind 0) is 12 steps of 4, two row groups, the second with ntile 1.  The pack leaves the BatchNorm fold out (gamma null): the bias is passed.
@pytest.mark.parametrize('kind,nd', [(0, 2), (0, 3), (1, 2), (1, 3)])
def test_lk_f32_conv_fwd(nv, kind, nd):
    N, sp, cin, cout = N3, GRID[nd], 48, 80
    D, H, W = dhw(nd, sp)
    d = check_lk_fwd(kind, nd, N, sp, cin, cout)
    assert -(-(-(-N * vox(sp) // 16)) // 4) == (15 if nd == 2 else 13) and -(-cout // 64) == 2
    isp, osp = lk_grids(kind, sp)
    ref = F.relu(d['raw'] + bc(d['bias'], nd).double()) + (d['skip'].double() if kind == 0 else 0)

    def run(pl):
        xo = Operand(N, cin * vox(isp), F32, pl['x'], d['x'].reshape(N, -1), name='x')
        wo, bo = dev32(d['w'], 'w'), dev32(d['bias'], 'bias')
        pk = 0 if kind == 0 else 2
        wpk = scratch(nv.lib().iunet_lk_pack_elems(nd, pk, cout, cin), F32, name='wpk')
        nv.call('iunet_lk_pack', 2, nd, pk, nv.ptr(wo.t), None, None, None, None, 0.0, nv.ptr(wpk.t), None, cout, cin, nv.stream())
        so = Operand(N, cout * vox(osp), F32, pl['skip'], d['skip'].reshape(N, -1), name='skip') if kind == 0 else None
        yo = Operand(N, cout * vox(osp), F32, pl['y'], None, name='y')
        nv.call('iunet_lk_f32_conv_fwd', nd, kind, nv.ptr(xo.t), xo.ss, nv.ptr(yo.t), yo.ss, nv.ptr(wpk.t), nv.ptr(bo.t), None if so is None else nv.ptr(so.t),
                0 if so is None else so.ss, N, D, H, W, cin, cout, nv.stream())
        return {'y': yo}, [xo, wo, bo, wpk, yo] + ([so] if so is not None else [])

    res = over_placements(nv, run, LK_ROWS)
    assert_same32(res['y'].logical().reshape(ref.shape), ref, 'lk f32 y')


# iunet_lk_bn_relu_add: one thread per voxel and 8-channel plane, 256 per block: vox 63 (one block), 299 and 600 (ragged second / third block)
@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('C', [8, 72])
@pytest.mark.parametrize('v', [63, 299, 600])
def test_lk_bn_relu_add(nv, dt, C, v):
    dtype, N = DT[dt], N3
    g = gen(2200 + C + v)
    y, skip = ints(g, -2, 2, (N, C, v)), ints(g, -3, 3, (N, C, v))
    scale, shift = prologue(g, C)
    ref = act_of(y, scale, shift) + skip

    def run(pl):
        yo, so, oo = put(y, dtype, pl['y'], 'y'), put(skip, dtype, pl['skip'], 'skip'), out(N, C, v, dtype, pl['out'], 'out')
        sc, sh = dev32(scale, 'scale'), dev32(shift, 'shift')
        nv.call('iunet_lk_bn_relu_add', CODE[dtype], nv.ptr(yo.t), yo.ss, nv.ptr(so.t), so.ss, nv.ptr(oo.t), oo.ss, nv.ptr(sc.t), nv.ptr(sh.t), C, N, v, nv.stream())
        return {'out': oo}, [yo, so, oo, sc, sh]

    res = over_placements(nv, run, [None, {'y': 'gap', 'skip': 'upper', 'out': 'lower'}, {'y': 'upper', 'skip': 'lower', 'out': 'gap'}])
    assert_rounded(planar(res['out'], C, (v,)), ref, dtype, 'bn_relu_add')


# ================================================================================================================ DeepLabV3
# iunet_dl_conv_fwd (gg_fwd_kernel under DlFwdGather) on G2 / G3: 4 workgroups along x as above, one or two row groups (Cout 16: ntile 1; 80: the
# second group ntile 1).  Cin 8 and 24: a tap changes inside one 32-wide k step (the operator is not padded: a K tail loads zeros on both sides).
# Rates and the taps they keep (|(k - 1) rate| < extent on every axis):
#   G2 13 x 23:     0 -> 1;  1 -> 9;  13 -> 3 (kh pruned);  23 -> 1
#   G3 3 x 7 x 13:  0 -> 1;  1 -> 27;  3 -> 9 (kd pruned);  7 -> 3 (kd, kh pruned);  13 -> 1
DL_RATES = {2: [(0, 1), (1, 9), (13, 3), (23, 1)], 3: [(0, 1), (1, 27), (3, 9), (7, 3), (13, 1)]}
DL_FWD = [(nd, rate, taps, ci, co) for nd in (2, 3) for rate, taps in DL_RATES[nd] for ci in (8, 24, 64) for co in (16, 80)]
DL_ROWS = [None, {'x': 'gap', 'y': 'upper'}, {'x': 'lower', 'y': 'gap'}]
PSB_SCALE = 0.5


def dl_conv(nd, x, w, rate):
    k, r = w.shape[-1], max(rate, 1)
    return (F.conv3d if nd == 3 else F.conv2d)(x, w, padding=r * (k // 2), dilation=r)


def dl_dgrad(nd, dy, w, rate):
    """The data gradient of dl_conv with w [Cout][Cin][k..]: dy [N, Cout] -> dx [N, Cin]."""
    k, r = w.shape[-1], max(rate, 1)
    return (F.conv_transpose3d if nd == 3 else F.conv_transpose2d)(dy, w, padding=r * (k // 2), dilation=r)


@functools.lru_cache(maxsize=None)
def dl_data(nd, N, sp, cin, cout, rate):
    """Forward launch cin -> cout with w [cout][cin]; the data-gradient launch has the same channels: w2 [cin][cout], dy with cin channels -> dx with cout."""
    g = gen(3000 + 100 * nd + cin + rate)
    kk = (1 if rate == 0 else 3,) * nd
    d = dict(x=ints(g, -2, 2, (N, cin) + sp), w=ints(g, -1, 1, (cout, cin) + kk), bias=ints(g, -3, 3, (cout,)), psb=ints(g, -3, 3, (N, cout)),
             w2=ints(g, -1, 1, (cin, cout) + kk))
    d['scale'], d['shift'] = prologue(g, cin)
    d['act'] = act_of(d['x'], d['scale'], d['shift'])
    w = d['w'].double()
    d['raw_psb'] = dl_conv(nd, d['x'].double(), w, rate) + PSB_SCALE * d['psb'].double().view(N, cout, *([1] * nd))
    d['raw_act'] = dl_conv(nd, d['act'].double(), w, rate)
    d['epi'] = F.relu(d['raw_psb'] - PSB_SCALE * d['psb'].double().view(N, cout, *([1] * nd)) + bc(d['bias'], nd).double())
    d['dgrad'] = dl_dgrad(nd, d['x'].double(), d['w2'].double(), rate)
    d['bound'] = max(dl_conv(nd, d['act'].double(), w.abs(), rate).max().item(), dl_dgrad(nd, d['x'].abs().double(), d['w2'].abs().double(), rate).max().item()) + 3
    return d


def check_dl_fwd(nd, N, sp, cin, cout, rate):
    d = dl_data(nd, N, sp, cin, cout, rate)
    check_partial_sums(2 * d['bound'], 'dl fwd')          # in units of psb_scale = 1/2
    per, _ = gg_fwd_share(N * vox(sp), gg_fwd_blocks(N * vox(sp), -(-cout // 64)))
    check_row_squares(d['raw_psb'], per * 16, PSB_SCALE, 'dl fwd + psb')
    check_row_squares(d['raw_act'], per * 16, 1.0, 'dl fwd, activation')
    return d


def dl_fwd_run(nv, dtype, nd, N, sp, cin, cout, rate, d, form, pl):
    """'raw_psb': raw + statistics + per-sample bias; 'raw_act': raw + statistics through the input activation; 'epi': + bias, ReLU;
    'dgrad': the mode-1 operator of w2 over x as the gradient."""
    D, H, W = dhw(nd, sp)
    ksz = 1 if rate == 0 else 3
    kv = ksz ** nd
    xo = put(d['x'], dtype, pl['x'], 'x')
    wo = dev32(d['w2'] if form == 'dgrad' else d['w'], 'w')
    Kw = kv * cin
    wpk = scratch(cout * Kw, dtype, name='wpk')
    if form == 'dgrad':          # dst[ci of w2 = the launch's Cout rows][kv * (Cout of w2 = the launch's Cin)]
        nv.call('iunet_dl_pack', CODE[dtype], nd, 1, ksz, nv.ptr(wo.t), None, None, None, None, 0.0, nv.ptr(wpk.t), None, cin, cout, cout, 0, 0, Kw, nv.stream())
    else:
        nv.call('iunet_dl_pack', CODE[dtype], nd, 0, ksz, nv.ptr(wo.t), None, None, None, None, 0.0, nv.ptr(wpk.t), None, cout, cin, cin, 0, 0, Kw, nv.stream())
    yo = out(N, cout, vox(sp), dtype, pl['y'], 'y')
    ops, outs = [xo, wo, wpk, yo], {'y': yo}
    sc = sh = bo = po = st = None
    if form == 'raw_act':
        sc, sh = dev32(d['scale'], 'in_scale'), dev32(d['shift'], 'in_shift')
        ops += [sc, sh]
    if form == 'raw_psb':
        po = dev32(d['psb'], 'psb')
        ops.append(po)
    if form == 'epi':
        bo = dev32(d['bias'], 'bias')
        ops.append(bo)
    if form in ('raw_psb', 'raw_act'):
        st = scratch(nv.lib().iunet_dl_stats_parts(N, D, H, W, cout) * cout * 2, name='stats')
        ops.append(st)
        outs['stats'] = st
    P = lambda o: None if o is None else nv.ptr(o.t)
    nv.call('iunet_dl_conv_fwd', CODE[dtype], nd, P(xo), xo.ss, P(yo), yo.ss, P(wpk), Kw, 1, nv.int_array([rate]), nv.int_array([0]), nv.int_array([0]),
            P(sc), P(sh), P(bo), P(po), PSB_SCALE, P(st), 1 if form == 'epi' else 0, N, D, H, W, cin, cout, nv.stream())
    return outs, ops


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('nd,rate,taps,cin,cout', DL_FWD)
def test_dl_conv_fwd(nv, dt, nd, rate, taps, cin, cout):
    dtype, N, sp = DT[dt], N3, GRID[nd]
    D, H, W = dhw(nd, sp)
    assert nv.lib().iunet_dl_num_taps(nd, rate, D, H, W) == len(dl_kept(nd, rate, sp)) == taps
    d = check_dl_fwd(nd, N, sp, cin, cout, rate)
    parts = nv.lib().iunet_dl_stats_parts(N, D, H, W, cout)
    assert parts == gg_fwd_blocks(N * vox(sp), -(-cout // 64)) == 4
    assert -(-cout // 64) == (2 if cout == 80 else 1) and (cout % 64) // 16 == 1          # the last (or only) row group has one row tile
    assert (cin % 32 != 0) == (cin in (8, 24))          # Cin 8, 24: a tap boundary inside a 32-wide k step (taps > 1), a K tail in the last one
    for form in ('raw_psb', 'raw_act', 'epi', 'dgrad'):
        res = over_placements(nv, lambda pl: dl_fwd_run(nv, dtype, nd, N, sp, cin, cout, rate, d, form, pl), DL_ROWS)
        assert_rounded(planar(res['y'], cout, sp), d[form], dtype, f'dl y ({form})')
        if 'stats' in res:
            assert_stats(res['stats'], parts, cout, d[form], f'dl statistics ({form})')


# The ASPP data gradient as ONE launch of four branches: dy is the four-slot branch-gradient buffer (cbase 0, C, 2C, 3C), the operators sit side
# by side (colbase 0, C, C + kv C, C + 2 kv C), dmean[n][c] * psb_scale is the pooling branch's adjoint (1 / vox as a power of two: 1 / 256).
# C = 32 (the launch's Cin), Cb = 80 (its Cout: two row groups).  Taps: G2 rates 0, 1, 13, 23: 1 + 9 + 3 + 1 = 14; G3 rates 0, 1, 3, 7: 1 + 27 + 9 + 3 = 40.
ASPP = {2: (0, 1, 13, 23), 3: (0, 1, 3, 7)}
ASPP_C, ASPP_CB, ASPP_SCALE = 32, 80, 1.0 / 256


@functools.lru_cache(maxsize=None)
def aspp_data(nd, N, sp):
    g = gen(3500 + nd)
    C, Cb = ASPP_C, ASPP_CB
    ws = [ints(g, -1, 1, (C, Cb) + ((1 if r == 0 else 3),) * nd) for r in ASPP[nd]]
    dys = [ints(g, -2, 2, (N, C) + sp) for _ in range(4)]
    dmean = ints(g, -3, 3, (N, Cb))
    ref = sum(dl_dgrad(nd, dy.double(), w.double(), r) for dy, w, r in zip(dys, ws, ASPP[nd])) + ASPP_SCALE * dmean.double().view(N, Cb, *([1] * nd))
    bound = sum(dl_dgrad(nd, dy.abs().double(), w.abs().double(), r) for dy, w, r in zip(dys, ws, ASPP[nd])).max().item() + 1
    return dict(ws=ws, dys=dys, dmean=dmean, ref=ref, bound=bound)


def check_aspp(nd, N, sp):
    d = aspp_data(nd, N, sp)
    check_partial_sums(d['bound'] / ASPP_SCALE, 'aspp dgrad')          # in units of 1 / 256
    return d


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('nd', [2, 3])
def test_dl_aspp_dgrad_one_launch(nv, dt, nd):
    dtype, N, sp = DT[dt], N3, GRID[nd]
    D, H, W = dhw(nd, sp)
    C, Cb, kv = ASPP_C, ASPP_CB, 3 ** nd
    d = check_aspp(nd, N, sp)
    rates = ASPP[nd]
    cbase, colbase = [0, C, 2 * C, 3 * C], [0, C, C + kv * C, C + 2 * kv * C]
    ntaps = [nv.lib().iunet_dl_num_taps(nd, r, D, H, W) for r in rates]
    assert ntaps == [len(dl_kept(nd, r, sp)) for r in rates] and sum(ntaps) == (14 if nd == 2 else 40) and len(set(cbase)) == 4
    ld = C * (1 + 3 * kv)

    def run(pl):
        dyo = put(torch.cat(d['dys'], 1), dtype, pl['dy'], 'dy')          # the four slots of one buffer
        wos = [dev32(w, f'w{k}') for k, w in enumerate(d['ws'])]
        op = scratch(Cb * ld, dtype, name='operators')
        for k, wo in enumerate(wos):
            nv.call('iunet_dl_pack', CODE[dtype], nd, 1, 1 if rates[k] == 0 else 3, nv.ptr(wo.t), None, None, None, None, 0.0, nv.ptr(op.t), None, C, Cb, Cb, 0,
                    colbase[k], ld, nv.stream())
        dm = dev32(d['dmean'], 'dmean')
        dxo = out(N, Cb, vox(sp), dtype, pl['dx'], 'dx')
        nv.call('iunet_dl_conv_fwd', CODE[dtype], nd, nv.ptr(dyo.t), dyo.ss, nv.ptr(dxo.t), dxo.ss, nv.ptr(op.t), ld, 4, nv.int_array(rates), nv.int_array(cbase),
                nv.int_array(colbase), None, None, None, nv.ptr(dm.t), ASPP_SCALE, None, 0, N, D, H, W, C, Cb, nv.stream())
        return {'dx': dxo}, [dyo, op, dm, dxo] + wos

    res = over_placements(nv, run, [None, {'dy': 'gap', 'dx': 'upper'}, {'dy': 'gap', 'dx': 'gap'}])
    assert_rounded(planar(res['dx'], Cb, sp), d['ref'], dtype, 'aspp dx')


# iunet_dl_wgrad (gg_wgrad_kernel under DlWgGather + dl_wgrad_reduce_kernel): chunks of 32 columns, splits = min(ceil(chunks / 16), 64)
#   G2: 897 columns, 29 chunks -> 2 splits of 15 and 14 chunks, the last chunk holds 1 column;  G3: 819 columns, 26 chunks -> 2 splits of 13, the last holds 19
# Cout 24 / 72: the co_ok path (3 of 8 row groups of 8; a second 64-row group of 8 rows); Cin 8 / 40: the k_ok path and K no multiple of 64.
# x holds Cin + 8 channels and is read from cbase = 8; dW is [Cout][Cin_tot = Cin + 16][kvol], written at ci_off = 8: the other entries keep the
# sentinel bits, a pruned tap's entries are +0.
DL_WGRAD = [(nd, rate, ci, co) for nd in (2, 3) for rate in ((0, 1, 13) if nd == 2 else (0, 1, 3)) for ci in (8, 40) for co in (24, 72)]
DL_HALVED = dict(nd=3, N=3, sp=(6, 10, 20), cin=256, cout=256, rate=1)


@functools.lru_cache(maxsize=None)
def dl_wgrad_data(nd, N, sp, cin, cout, rate, cbase, lo=-2):
    g = gen(3600 + 100 * nd + cin + rate)
    d = dict(x=ints(g, lo, -lo, (N, cin + cbase) + sp), dy=ints(g, -2, 2, (N, cout) + sp))
    d['scale'], d['shift'] = prologue(g, cin + cbase)
    d['act'] = act_of(d['x'], d['scale'], d['shift'])
    return d


@functools.lru_cache(maxsize=None)
def dl_wgrad_ref(nd, N, sp, cin, cout, rate, cbase, act, lo=-2, real=torch.float64):
    d = dl_wgrad_data(nd, N, sp, cin, cout, rate, cbase, lo)
    w = torch.zeros((cout, cin) + ((1 if rate == 0 else 3),) * nd, dtype=real, requires_grad=True)
    dl_conv(nd, (d['act'] if act else d['x'])[:, cbase:cbase + cin].to(real), w, rate).backward(d['dy'].to(real))
    return ALPHA * w.grad


def check_dl_wgrad(nd, N, sp, cin, cout, rate, cbase, lo=-2):
    d = dl_wgrad_data(nd, N, sp, cin, cout, rate, cbase, lo)
    check_partial_sums(N * vox(sp) * d['dy'].abs().max().item() * max(d['act'].max().item(), d['x'].abs().max().item()), 'dl wgrad')
    return d


def dl_wgrad_run(nv, dtype, nd, N, sp, cin, cout, rate, cbase, cin_tot, ci_off, act, d, pl):
    D, H, W = dhw(nd, sp)
    kvol = 1 if rate == 0 else 3 ** nd
    xo, dyo = put(d['x'], dtype, pl['x'], 'x'), put(d['dy'], dtype, pl['dy'], 'dy')
    slab = scratch(nv.lib().iunet_dl_wgrad_slab_floats(nd, rate, N, D, H, W, cin, cout), name='slab')
    dW = scratch(cout * cin_tot * kvol, name='dW')
    ops = [xo, dyo, slab, dW]
    sc = sh = None
    if act:
        sc, sh = dev32(d['scale'], 'x_scale'), dev32(d['shift'], 'x_shift')
        ops += [sc, sh]
    nv.call('iunet_dl_wgrad', CODE[dtype], nd, rate, nv.ptr(xo.t), xo.ss, cbase, nv.ptr(dyo.t), dyo.ss, None if sc is None else nv.ptr(sc.t),
            None if sh is None else nv.ptr(sh.t), nv.ptr(slab.t), nv.ptr(dW.t), cin_tot, ci_off, ALPHA, N, D, H, W, cin, cout, nv.stream())
    return {'dW': dW}, ops


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('nd,rate,cin,cout', DL_WGRAD)
def test_dl_wgrad(nv, dt, nd, rate, cin, cout):
    dtype, N, sp = DT[dt], N3, GRID[nd]
    D, H, W = dhw(nd, sp)
    cbase, ci_off, cin_tot = 8, 8, cin + 16
    d = check_dl_wgrad(nd, N, sp, cin, cout, rate, cbase)
    kept = dl_kept(nd, rate, sp)
    kvol = 1 if rate == 0 else 3 ** nd
    K = len(kept) * cin
    assert nv.lib().iunet_dl_num_taps(nd, rate, D, H, W) == len(kept) and (len(kept) < kvol) == (rate > 1)
    cols = N * vox(sp)
    splits = nv.lib().iunet_dl_wgrad_slab_floats(nd, rate, N, D, H, W, cin, cout) // (cout * K)
    chunks = -(-cols // 32)
    assert splits == gg_wgrad_splits(cols, cout * K) == 2 and (chunks, -(-chunks // 2), cols % 32) == ((29, 15, 1) if nd == 2 else (26, 13, 19))
    assert cout % 16 != 0 and K % 64 != 0          # rows of the last row tile and columns of the last k group unused
    pruned = torch.tensor([k not in kept for k in range(kvol)])
    for act in (False, True):
        res = over_placements(nv, lambda pl: dl_wgrad_run(nv, dtype, nd, N, sp, cin, cout, rate, cbase, cin_tot, ci_off, act, d, pl),
                              [None, {'x': 'gap', 'dy': 'upper'}, {'x': 'upper', 'dy': 'gap'}])
        got = res['dW'].logical().reshape(cout, cin_tot, kvol)
        ref = dl_wgrad_ref(nd, N, sp, cin, cout, rate, cbase, act).reshape(cout, cin, kvol)
        assert_same32(got[:, ci_off:ci_off + cin], ref, f'dl dW (act {act})')
        outside = torch.cat([got[:, :ci_off], got[:, ci_off + cin:]], 1)
        assert bool((bits(outside) == SENTINEL[F32]).all()), 'dW outside the channel slice must keep the sentinel bits'
        assert bool((bits(got[:, ci_off:ci_off + cin][:, :, pruned]) == 0).all()), "a pruned tap's gradient must be +0"


def test_dl_wgrad_splits_halved(nv):
    """3-D, 6 x 10 x 20, Cin = Cout = 256, rate 1: 3 600 columns, 113 chunks -> 8 splits, 8 x 256 x 6912 = 13.5 Mi > 8 Mi -> 4 splits of 29 chunks."""
    dtype = torch.float16
    nd, N, sp, cin, cout, rate = (DL_HALVED[k] for k in ('nd', 'N', 'sp', 'cin', 'cout', 'rate'))
    D, H, W = dhw(nd, sp)
    d = check_dl_wgrad(nd, N, sp, cin, cout, rate, 0, -1)
    cols, K = N * vox(sp), 27 * cin
    splits = nv.lib().iunet_dl_wgrad_slab_floats(nd, rate, N, D, H, W, cin, cout) // (cout * K)
    assert -(-(-(-cols // 32)) // 16) == 8 and 8 * cout * K > 8 << 20 and splits == gg_wgrad_splits(cols, cout * K) == 4
    res = over_placements(nv, lambda pl: dl_wgrad_run(nv, dtype, nd, N, sp, cin, cout, rate, 0, cin, 0, True, d, pl), [None, {'x': 'gap', 'dy': 'upper'}])
    ref = dl_wgrad_ref(nd, N, sp, cin, cout, rate, 0, True, -1, torch.float32)
    assert_same32(res['dW'].logical().reshape(ref.shape), ref, 'dl dW, splits halved')


# iunet_dl_f32_conv_fwd (gg_f32_kernel under DlFwdGather): Cin 24 (a tap changes inside the incremental k walk of 4), Cout 80, psb at scale 1
@pytest.mark.parametrize('nd,rate', [(2, 1), (2, 13), (3, 1), (3, 3)])
def test_dl_f32_conv_fwd(nv, nd, rate):
    N, sp, cin, cout = N3, GRID[nd], 24, 80
    D, H, W = dhw(nd, sp)
    d = check_dl_fwd(nd, N, sp, cin, cout, rate)
    kv = 3 ** nd
    assert nv.lib().iunet_dl_num_taps(nd, rate, D, H, W) == len(dl_kept(nd, rate, sp)) == dict(DL_RATES[nd])[rate]
    ref = F.relu(dl_conv(nd, d['x'].double(), d['w'].double(), rate) + d['psb'].double().view(N, cout, *([1] * nd)) + bc(d['bias'], nd).double())

    def run(pl):
        xo = Operand(N, cin * vox(sp), F32, pl['x'], d['x'].reshape(N, -1), name='x')
        wo, bo, po = dev32(d['w'], 'w'), dev32(d['bias'], 'bias'), dev32(d['psb'], 'psb')
        wpk = scratch(cout * kv * cin, F32, name='wpk')
        nv.call('iunet_dl_pack', 2, nd, 0, 3, nv.ptr(wo.t), None, None, None, None, 0.0, nv.ptr(wpk.t), None, cout, cin, cin, 0, 0, kv * cin, nv.stream())
        yo = Operand(N, cout * vox(sp), F32, pl['y'], None, name='y')
        nv.call('iunet_dl_f32_conv_fwd', nd, rate, nv.ptr(xo.t), xo.ss, nv.ptr(yo.t), yo.ss, nv.ptr(wpk.t), kv * cin, nv.ptr(bo.t), nv.ptr(po.t), N, D, H, W, cin,
                cout, nv.stream())
        return {'y': yo}, [xo, wo, bo, po, wpk, yo]

    res = over_placements(nv, run, DL_ROWS)
    assert_same32(res['y'].logical().reshape(ref.shape), ref, 'dl f32 y')


# iunet_dl_chansum: one workgroup per (plane, n) (16-bit) / (channel, n) (planar fp32), 256 threads striding the voxels: 299 (one ragged pass
# and a bit) and 2 431 (ten passes, ragged)
@pytest.mark.parametrize('dt', ['f16', 'bf16', 'f32'])
@pytest.mark.parametrize('C', [8, 72])
@pytest.mark.parametrize('v', [299, 2431])
def test_dl_chansum(nv, dt, C, v):
    dtype, N = {**DT, 'f32': F32}[dt], N3
    x = ints(gen(3700 + C + v), -2, 2, (N, C, v))
    ref = 0.25 * x.double().sum(2)
    check_partial_sums(2 * v, 'chansum')

    def run(pl):
        xo = put(x, dtype, pl['x'], 'x') if dtype != F32 else Operand(N, C * v, F32, pl['x'], x.reshape(N, -1), name='x')
        so = scratch(N * C, name='sums')
        nv.call('iunet_dl_chansum', CODE[dtype], nv.ptr(xo.t), xo.ss, nv.ptr(so.t), 0.25, C, N, v, nv.stream())
        return {'sums': so}, [xo, so]

    res = over_placements(nv, run, [None, {'x': 'gap'}, {'x': 'upper'}])
    assert_same32(res['sums'].logical().reshape(N, C), ref, 'chansum')


# ================================================================================================================ Segformer
# Target grids and sources at the ratios 1/2, 1 and 2 (align_corners=False: weights {1/2, 1/2}, {1}, {1/4, 3/4} with the border clamp: dyadic):
#   T2 = 14 x 22     308 voxels, 924 columns: 15 workgroups of 64 columns, the last holds 28; workgroups straddle samples; sources 28 x 44, 14 x 22, 7 x 11
#   T3 = 4 x 6 x 14  336 voxels, 1 008 columns: 16 workgroups, the last holds 48; sources 8 x 12 x 28, 4 x 6 x 14, 2 x 3 x 7
# Source channels (32, 64, 32): K = 128.  A resampled value is a multiple of SF_UNIT = 1/16 of magnitude <= 4 (the prologue keeps
# relu(scale x + shift) in 0..3): it fits bf16's 8 significant bits, so B survives the rounding to the storage type, and the GEMM, its
# statistics, the weight gradient and the adjoint are exact in fp32.  A statistics row holds 64 columns; its sum of squares is exact where it
# stays below 2^24 units of SF_UNIT^2.  Integers in -2..2 at ratio 2 in 3-D would leave multiples of 1/64, and a row of 64 columns of a K = 128
# product then sums squares to ~5 x 2^24 units: the coarsest 3-D source holds -4, 0, 4 (and relu(scale x + shift) in {0, 4}) instead, so
# that its weights, multiples of 1/64, leave multiples of 1/16 as in 2-D.
T2, T3 = (14, 22), (4, 6, 14)
SF_T = {2: T2, 3: T3}
SF_SRC = {2: [(28, 44), (14, 22), (7, 11)], 3: [(8, 12, 28), (4, 6, 14), (2, 3, 7)]}
SF_CH = (32, 64, 32)
SF_K = sum(SF_CH)
SF_UNIT = {2: 1.0 / 16, 3: 1.0 / 16}
SF_GEMM = ([(nd, dt, co) for nd in (2, 3) for dt in ('f16', 'bf16', 'f32') for co in (48, 272)] + [(nd, 'f32', 512) for nd in (2, 3)])
SF_ROWS = [None, {'x0': 'gap', 'x1': 'upper', 'x2': 'lower', 'y': 'upper', 'dz': 'gap'}, {'x0': 'upper', 'x1': 'gap', 'x2': 'gap', 'y': 'gap', 'dz': 'upper'}]


def sf_mode(nd):
    return 'trilinear' if nd == 3 else 'bilinear'


@functools.lru_cache(maxsize=None)
def sf_sources(nd, N):
    g = gen(4000 + nd)
    xs = [ints(g, -2, 2, (N, c) + sp) for c, sp in zip(SF_CH, SF_SRC[nd])]
    pro = [prologue(g, c, top=3) for c in SF_CH]
    if nd == 3:          # multiples of 4 under weights that are multiples of 1/64
        xs[2] = 4 * ints(g, -1, 1, xs[2].shape)
        pro[2] = (pro[2][0], -4 * (pro[2][0] == 2).float())
    return xs, pro


@functools.lru_cache(maxsize=None)
def sf_B(nd, N, act):
    """The resampled, concatenated operand [N, K, *T] in float64."""
    xs, pro = sf_sources(nd, N)
    srcs = [act_of(x, *p) if act else x for x, p in zip(xs, pro)]
    return torch.cat([F.interpolate(s.double(), size=list(SF_T[nd]), mode=sf_mode(nd), align_corners=False) for s in srcs], 1)


@functools.lru_cache(maxsize=None)
def sf_operator(nd, cout):
    g = gen(4100 + nd + cout)
    return ints(g, -1, 1, (cout, SF_K)), ints(g, -3, 3, (cout,))


@functools.lru_cache(maxsize=None)
def sf_gemm_ref(nd, N, cout, act):
    M, bias = sf_operator(nd, cout)
    return torch.einsum('ok,nk...->no...', M.double(), sf_B(nd, N, act)) + bc(bias, nd).double()


def check_sf_B(nd, N, act):
    B = sf_B(nd, N, act)
    for dtype in (torch.float16, torch.bfloat16):
        assert torch.equal(B.to(dtype).double(), B), f'the resampled operand does not survive the rounding to {dtype}'
    assert torch.equal((B / SF_UNIT[nd]).round() * SF_UNIT[nd], B) and B.abs().max().item() <= 4
    return B


def check_sf_gemm(nd, N, cout, act):
    B = check_sf_B(nd, N, act)
    M, _ = sf_operator(nd, cout)
    check_partial_sums((torch.einsum('ok,nk...->no...', M.abs().double(), B.abs()).max().item() + 3) / SF_UNIT[nd], 'sf gemm')
    ref = sf_gemm_ref(nd, N, cout, act)
    check_row_squares(ref, 64, SF_UNIT[nd], 'sf gemm')
    return ref


def sf_put_sources(nd, N, dtype, pl):
    xs, _ = sf_sources(nd, N)
    if dtype == F32:
        return [Operand(N, x[0].numel(), F32, pl[f'x{i}'], x.reshape(N, -1), name=f'x{i}') for i, x in enumerate(xs)]
    return [put(x, dtype, pl[f'x{i}'], f'x{i}') for i, x in enumerate(xs)]


def sf_prologue_tables(nd, N, act):
    if not act:
        return None, None, []
    _, pro = sf_sources(nd, N)
    scs, shs = [dev32(p[0], f'sc{i}') for i, p in enumerate(pro)], [dev32(p[1], f'sh{i}') for i, p in enumerate(pro)]
    return pointer_table(scs), pointer_table(shs), scs + shs


def sf_dims(nd):
    return [e for sp in SF_SRC[nd] for e in dhw(nd, sp)]


@pytest.mark.parametrize('act', [False, True])
@pytest.mark.parametrize('nd,dt,cout', SF_GEMM)
def test_sf_gemm(nv, nd, dt, cout, act):
    """sf_gemm_kernel: 15 / 16 workgroups; Cout 272 = 17 row tiles, wave 0 takes five (wave + 4 i up to i = 4); fp32 Cout 512: 32 row tiles and
    (64 + 512) x 36 x 4 = 82 944 bytes of dynamic LDS, above the 64 KiB default."""
    dtype, N, tsp = {**DT, 'f32': F32}[dt], N3, SF_T[nd]
    D, H, W = dhw(nd, tsp)
    vt = vox(tsp)
    ref = check_sf_gemm(nd, N, cout, act)
    parts = nv.lib().iunet_sf_stats_parts(N, D, H, W)
    assert parts == sf_blocks(N * vt) == (15 if nd == 2 else 16) and N * vt - 64 * (parts - 1) == (28 if nd == 2 else 48) and vt % 64 != 0
    assert cout // 16 == {48: 3, 272: 17, 512: 32}[cout] and -(-(cout // 16) // 4) == {48: 1, 272: 5, 512: 8}[cout]
    assert ((64 + cout) * 36 * 4 > 65536) == (cout == 512)
    M, bias = sf_operator(nd, cout)

    for epi in (0, 1):
        def run(pl):
            xos = sf_put_sources(nd, N, dtype, pl)
            xp, xss = source_tables(xos)
            scp, shp, pro_ops = sf_prologue_tables(nd, N, act)
            wo, bo = Operand(1, cout * SF_K, dtype, TIGHT, M, name='operator'), dev32(bias, 'bias')
            yo = Operand(N, cout * vt, dtype, pl['y'], None, name='y')
            st = scratch(parts * cout * 2, name='stats') if epi == 0 else None
            nv.call('iunet_sf_gemm', CODE[dtype], nd, 3, xp, xss, nv.int_array(SF_CH), nv.int_array(sf_dims(nd)), scp, shp, nv.ptr(wo.t), nv.ptr(bo.t), nv.ptr(yo.t),
                    yo.ss, None if st is None else nv.ptr(st.t), epi, N, D, H, W, cout, nv.stream())
            return ({'y': yo, 'stats': st} if st is not None else {'y': yo}), xos + pro_ops + [wo, bo, yo] + ([st] if st is not None else [])

        res = over_placements(nv, run, SF_ROWS)
        want = ref if epi == 0 else F.relu(ref)
        if dtype == F32:
            assert_same32(res['y'].logical().reshape(want.shape), want, f'sf y (epi {epi})')
        else:
            assert_rounded(planar(res['y'], cout, tsp), want, dtype, f'sf y (epi {epi})')
        if epi == 0:
            assert_stats(res['stats'], parts, cout, ref, 'sf statistics')


# iunet_sf_wgrad (gg_wgrad_kernel under SfResample): G [Cout][K = 128] (two k groups of 64); 924 columns: 29 chunks -> 2 splits of 15 and 14;
# 1 008 columns: 32 chunks -> 2 splits of 16.  Cout 24 / 72: the co_ok path as in iunet_dl_wgrad.
@pytest.mark.parametrize('act', [False, True])
@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('nd,cout', [(nd, co) for nd in (2, 3) for co in (24, 72)])
def test_sf_wgrad(nv, nd, cout, dt, act):
    dtype, N, tsp = DT[dt], N3, SF_T[nd]
    D, H, W = dhw(nd, tsp)
    vt = vox(tsp)
    B = check_sf_B(nd, N, act)
    dz = ints(gen(4200 + nd + cout), -2, 2, (N, cout) + tsp)
    check_partial_sums(N * vt * 2 * 4 / SF_UNIT[nd], 'sf wgrad')
    ref = torch.einsum('nc...,nk...->ck', dz.double(), B)
    floats = nv.lib().iunet_sf_wgrad_slab_floats(N, D, H, W, SF_K, cout)
    chunks = -(-N * vt // 32)
    assert floats // (cout * SF_K) == gg_wgrad_splits(N * vt, cout * SF_K) == 2 and chunks == (29 if nd == 2 else 32) and cout % 16 != 0 and SF_K // 64 == 2

    def run(pl):
        xos = sf_put_sources(nd, N, dtype, pl)
        xp, xss = source_tables(xos)
        scp, shp, pro_ops = sf_prologue_tables(nd, N, act)
        dzo = put(dz, dtype, pl['dz'], 'dz')
        slab, G = scratch(floats, name='slab'), scratch(cout * SF_K, name='G')
        nv.call('iunet_sf_wgrad', CODE[dtype], nd, 3, xp, xss, nv.int_array(SF_CH), nv.int_array(sf_dims(nd)), scp, shp, nv.ptr(dzo.t), dzo.ss, nv.ptr(slab.t),
                nv.ptr(G.t), N, D, H, W, cout, nv.stream())
        return {'G': G}, xos + pro_ops + [dzo, slab, G]

    res = over_placements(nv, run, SF_ROWS)
    assert_same32(res['G'].logical().reshape(cout, SF_K), ref, 'sf G')


# iunet_sf_adjoint: the resize's adjoint from T to each source grid (ratios 1/2, 1, 2), one thread per (source voxel, 8 channels); integer u and
# dyadic weights: the fp32 sum is exact, one rounding.  The reference is the autograd of F.interpolate in float64.
@functools.lru_cache(maxsize=None)
def sf_adjoint_data(nd, N, C, src):
    tsp, ssp = SF_T[nd], SF_SRC[nd][src]
    u = ints(gen(4300 + nd + C + src), -2, 2, (N, C) + tsp)
    x = torch.zeros((N, C) + ssp, dtype=torch.float64, requires_grad=True)
    r = F.interpolate(x, size=list(tsp), mode=sf_mode(nd), align_corners=False)
    ref = torch.autograd.grad((r * u.double()).sum(), x, retain_graph=True)[0]
    bound = torch.autograd.grad((r * u.abs().double()).sum(), x)[0]          # the adjoint of |u|: every partial sum's bound
    return u, ref, bound.max().item()


def check_sf_adjoint(nd, N, C, src):
    u, ref, bound = sf_adjoint_data(nd, N, C, src)
    unit = 4.0 ** -nd          # integer u under per-axis weights that are multiples of 1/4
    assert torch.equal((ref / unit).round() * unit, ref)
    check_partial_sums(bound / unit, 'sf adjoint')
    return u, ref


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('C', [8, 24])
@pytest.mark.parametrize('nd,src', [(nd, s) for nd in (2, 3) for s in range(3)])
def test_sf_adjoint(nv, nd, src, C, dt):
    dtype, N, tsp, ssp = DT[dt], N3, SF_T[nd], SF_SRC[nd][src]
    u, ref = check_sf_adjoint(nd, N, C, src)
    Dt, Ht, Wt = dhw(nd, tsp)
    Ds, Hs, Ws = dhw(nd, ssp)

    def run(pl):
        uo, dxo = put(u, dtype, pl['u'], 'u'), out(N, C, vox(ssp), dtype, pl['dx'], 'dx')
        nv.call('iunet_sf_adjoint', CODE[dtype], nd, nv.ptr(uo.t), uo.ss, Dt, Ht, Wt, nv.ptr(dxo.t), dxo.ss, Ds, Hs, Ws, C, N, nv.stream())
        return {'dx': dxo}, [uo, dxo]

    res = over_placements(nv, run, [None, {'u': 'gap', 'dx': 'upper'}, {'u': 'lower', 'dx': 'gap'}])
    assert_rounded(planar(res['dx'], C, ssp), ref, dtype, 'sf adjoint dx')
