"""The 16-bit core kernels across dtype x nd x host dispatch branch x buffer placement, through the C ABI.

Every operand is allocated through tests/arena.py: it sits `lead` elements into a sentinel-filled allocation with its samples
`ss` apart, the way net.hip / train_net.hip hand the kernels halves of concat buffers and slots of gradient buffers.  Each case runs
its entry point once with every operand tight and once per further placement row and asserts
  1. the tight result against a reference that owes nothing to the library: torch on the CPU, bit for bit on small-integer data for
     the linear kernels (fp32 outputs exact throughout, 16-bit outputs where |ref| <= 2048 (f16) / 256 (bf16), at most 2 % of the
     reference outside that), float64 on inputs already rounded to the storage type for the non-linear ones (16-bit elements within
     one unit in the last place of the storage type at |ref| plus 1e-5 x the tensor's maximum);
  2. stride independence: every other placement gives the bits of the tight one (no launch geometry here depends on a stride);
  3. no stray write: the sentinel outside the samples' extents is intact, inputs are unchanged bit for bit, scratch bands included;
  4. no unwritten output: outputs start as the sentinel, a NaN.
Batch sizes are 1 and 3 (with 3 a stride applied to the wrong operand cannot cancel).  Needs an MI355X: run with -m gpu."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.arena import Operand, StridedInput, bits, scratch
from tests.test_gpu_kernels import blocked, unblocked

pytestmark = pytest.mark.gpu

DT = {'f16': torch.float16, 'bf16': torch.bfloat16}
EXACT = {torch.float16: 2048, torch.bfloat16: 256}          # integers up to here are exact in the storage type
ULP = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}  # one unit in the last place, relative (twice a correct rounding)
TINY = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133}  # ... and of a subnormal number: the spacing of the type at the bottom of its range
F32 = torch.float32
TIGHT = 'tight'


@pytest.fixture(scope='module')
def nv():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from interactive_unet import _native
    _native.lib()
    return _native


# ---------------------------------------------------------------------------------------------------------------- helpers
def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def dhw(nd, shape):
    return tuple(shape) if nd == 3 else (1,) + tuple(shape)


def put(x, dtype, place, name):
    """An input activation tensor [N, C, *sp] (CPU, values exact in dtype) in blocked layout at a placement."""
    return Operand(x.shape[0], x[0].numel(), dtype, place, blocked(x.float(), dtype), name=name)


def out(N, C, vox, dtype, place, name):
    return Operand(N, C * vox, dtype, place, None, name=name)


def dev32(t, name):
    """A small fp32 parameter vector (an input) with bands around it."""
    t = t.reshape(-1).float()
    return Operand(1, t.numel(), F32, TIGHT, t, name=name)


def planar(op, C, sp):
    """Logical contents of a blocked 16-bit operand as fp32 [N, C, *sp]."""
    return unblocked(op.logical().float().reshape(-1), op.N, C, tuple(sp))


def over_placements(nv, run, rows):
    """run(places) -> (outputs: {name: Operand}, every operand of the call).  rows[0] is the all-tight placement.  Returns the tight
    outputs (the Operands, read back); asserts 2. and 3. of the module docstring for every row."""
    base = None
    for r, places in enumerate(rows):
        pl = {k: TIGHT for k in rows[-1]} if r == 0 else places
        outs, ops = run(pl)
        torch.cuda.synchronize()
        for o in ops:
            o.check()
        got = {k: o.logical() for k, o in outs.items()}
        if base is None:
            base, base_ops = got, outs
        else:
            for k in got:
                assert torch.equal(bits(base[k]), bits(got[k])), f'{k}: placement {pl} changes the result ({int((bits(base[k]) != bits(got[k])).sum())} elements)'
    return base_ops


def assert_exact16(got, ref, dtype, what):
    """16-bit output of a linear kernel on integer data against the exact reference."""
    ok = ref.abs() <= EXACT[dtype]
    assert (~ok).float().mean().item() <= 0.02, f'{what}: the reference leaves the exactly representable range too often'      # on the reference alone
    bad = (got != ref.float()) & ok          # a NaN (an unwritten element) differs
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} elements differ, max |diff| {(got - ref.float())[ok].abs().max().item()}'


def assert_ulp16(got, ref, dtype, what, sel=None):
    """16-bit output of a non-linear kernel against its float64 reference: one unit in the last place of the storage type at |ref| (2^-10 |ref| in
    f16, 2^-7 |ref| in bf16; the subnormal spacing where |ref| is subnormal: a gradient of 1e-5 is one in f16) + 1e-5 x max |ref|."""
    ref = ref.double()
    tol = torch.clamp(ULP[dtype] * ref.abs(), min=TINY[dtype]) + 1e-5 * ref.abs().max()
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)                      # a NaN fails
    if sel is not None:
        assert bool(torch.isfinite(got[~sel]).all()), f'{what}: non-finite output next to the ReLU kink'
        bad = bad & sel
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} elements off, worst err/tol {(err / tol)[bad].max().item():.2f}'


def roundT(t, dtype):
    return t.to(dtype).double()


# ---------------------------------------------------------------------------------------------------------------- transposed conv
@functools.lru_cache(maxsize=None)
def convT_data(nd, N, shape, cin, cout):
    g = gen(600 + nd)
    x = ints(g, -2, 2, (N, cin) + shape)
    w = ints(g, -1, 1, (cin, cout) + (2,) * nd)
    b = ints(g, -3, 3, (cout,))
    dy = ints(g, -1, 1, (N, cout) + tuple(2 * s for s in shape))
    return x, w, b, dy


@functools.lru_cache(maxsize=None)
def convT_fwd_ref(nd, N, shape, cin, cout):
    x, w, b, _ = convT_data(nd, N, shape, cin, cout)
    return (F.conv_transpose2d if nd == 2 else F.conv_transpose3d)(x, w, bias=b, stride=2)


@functools.lru_cache(maxsize=None)
def convT_dgrad_ref(nd, N, shape, cin, cout):
    _, w, _, dy = convT_data(nd, N, shape, cin, cout)
    return (F.conv2d if nd == 2 else F.conv3d)(dy, w, stride=2)          # the adjoint of the k2 s2 transposed conv


@functools.lru_cache(maxsize=None)
def convT_wgrad_ref(nd, N, shape, cin, cout):
    x, _, _, dy = convT_data(nd, N, shape, cin, cout)
    if nd == 2:
        H, W = shape
        dW = torch.einsum('nihw,nohawb->ioab', x, dy.reshape(N, cout, H, 2, W, 2))
    else:
        D, H, W = shape
        dW = torch.einsum('nidhw,nodehawb->ioeab', x, dy.reshape(N, cout, D, 2, H, 2, W, 2))
    return dW.contiguous(), dy.sum([0] + list(range(2, 2 + nd)))          # integer sums below 2^24: exact in fp32 in any order


def convT_waves(N, nd, shape):
    D, H, W = dhw(nd, shape)
    return N * D * H * ((W + 15) // 16)


# iunet_convT_fwd (pointwise.hip, iunet_convT_launch): waves = N D H ceil(W / 16), nk = Cin / 32
#   resident weights   nk <= 4 and waves >= 256                    2-D N 1 86 x 40: 258;   3-D N 3 3 x 16 x 24: 288   (W ragged in both)
#   resident Cin 256   nk == 8, 3-D, waves >= 2048                 N 1 16 x 16 x 120: 2048
#   chunked weights    nk in {4, 8, 16} and 64 <= waves < 256      2-D N 3 8 x 40: 72;     3-D N 1 3 x 8 x 40: 72
#   plain kernel       waves < 64, or nk == 3 with waves < 256     2-D N 1 5 x 24: 10;     3-D N 3 2 x 3 x 24: 36;   Cin 96 on the 72-wave grids
RES2, RES3 = (1, (86, 40)), (3, (3, 16, 24))
CHK2, CHK3 = (3, (8, 40)), (1, (3, 8, 40))
CONVT_FWD = ([('resident', 2) + RES2 + (c, 64 if c % 64 == 0 else 32) for c in (32, 64, 96, 128)] +
             [('resident', 3) + RES3 + (c, 64 if c % 64 == 0 else 32) for c in (32, 64, 96, 128)] +
             [('resident256', 3, 1, (16, 16, 120), 256, 32)] +
             [('chunked', 2) + CHK2 + (c, 32) for c in (128, 256, 512)] + [('chunked', 3) + CHK3 + (c, 32) for c in (128, 256, 512)] +
             [('plain', 2, 1, (5, 24), 64, 32), ('plain', 3, 3, (2, 3, 24), 128, 64), ('plain', 2) + CHK2 + (96, 32), ('plain', 3) + CHK3 + (96, 64)])


def convT_fwd_branch(nd, N, shape, cin):
    waves, nk = convT_waves(N, nd, shape), cin // 32
    if (nk <= 4 or (nk == 8 and nd == 3 and waves >= 2048)) and waves >= 256:
        return 'resident256' if nk == 8 else 'resident'
    if nk >= 4 and nk % 4 == 0 and waves >= 64:
        return 'chunked'
    return 'plain'


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('branch,nd,N,shape,cin,cout', CONVT_FWD)
def test_convT_fwd(nv, dt, branch, nd, N, shape, cin, cout):
    """y in the upper half of a concat buffer (and the lower one), the other half untouched; x with gaps between the samples."""
    dtype = DT[dt]
    assert convT_fwd_branch(nd, N, shape, cin) == branch          # the launcher's condition, restated above
    x, w, b, _ = convT_data(nd, N, shape, cin, cout)
    ref = convT_fwd_ref(nd, N, shape, cin, cout)
    D, H, W = dhw(nd, shape)
    osp = tuple(2 * s for s in shape)
    vout = int(np.prod(osp))
    code = nv.DTYPE_CODE[dtype]

    def run(pl):
        xo, wo, bo = put(x, dtype, pl['x'], 'x'), dev32(w, 'w'), dev32(b, 'bias')
        wpk = scratch(w.numel(), dtype, name='wpk')
        yo = out(N, cout, vout, dtype, pl['y'], 'y')
        nv.call('iunet_pack_convT', code, nv.ptr(wo.t), nv.ptr(wpk.t), cin, cout, 2 ** nd, nv.stream())
        nv.call('iunet_convT_fwd', code, nd, nv.ptr(xo.t), xo.ss, nv.ptr(yo.t), yo.ss, nv.ptr(wpk.t), nv.ptr(bo.t), N, D, H, W, cin, cout, nv.stream())
        return {'y': yo}, [xo, wo, bo, wpk, yo]

    res = over_placements(nv, run, [None, {'x': 'gap', 'y': 'upper'}, {'x': 'gap', 'y': 'lower'}])
    assert_exact16(planar(res['y'], cout, osp), ref, dtype, 'convT y')


# iunet_convT_dgrad (train_misc.hip): waves as above, nk = Cout / 32
#   LDS kernel <NK = nk, NCI>   nk <= 4 and waves >= 256; NCI = 2 iff nk <= 2 and Cin / 32 even (NCI 1, 2, 1, 2 for Cin 32, 64, 96, 128 at
#                               Cout <= 64; NCI 1 at Cout 96, 128) -- the resident grids above, W ragged
#   plain kernel                waves < 256 (the 72-wave grids), and Cout = 256 (nk = 8) at any size
CONVT_DGRAD = ([('lds', 2) + RES2 + (ci, co) for co in (32, 64, 96, 128) for ci in (32, 64, 96, 128)] +
               [('lds', 3) + RES3 + (ci, co) for co in (32, 64, 96, 128) for ci in (32, 64, 96, 128)] +
               [('plain', 2) + CHK2 + (64, 32), ('plain', 3) + CHK3 + (64, 32), ('plain', 2) + RES2 + (32, 256), ('plain', 3) + RES3 + (64, 256)])


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('branch,nd,N,shape,cin,cout', CONVT_DGRAD)
def test_convT_dgrad(nv, dt, branch, nd, N, shape, cin, cout):
    """dy in the upper half of a two-slot gradient buffer (train_net.hip's dcat_ss), dx with gaps."""
    dtype = DT[dt]
    assert ('lds' if cout // 32 <= 4 and convT_waves(N, nd, shape) >= 256 else 'plain') == branch
    _, w, _, dy = convT_data(nd, N, shape, cin, cout)
    ref = convT_dgrad_ref(nd, N, shape, cin, cout)
    D, H, W = dhw(nd, shape)
    vin = int(np.prod(shape))
    code = nv.DTYPE_CODE[dtype]

    def run(pl):
        dyo, wo = put(dy, dtype, pl['dy'], 'dy'), dev32(w, 'w')
        wpk = scratch(w.numel(), dtype, name='wpk')
        dxo = out(N, cin, vin, dtype, pl['dx'], 'dx')
        nv.call('iunet_pack_convT_dgrad', code, nv.ptr(wo.t), nv.ptr(wpk.t), cin, cout, 2 ** nd, nv.stream())
        nv.call('iunet_convT_dgrad', code, nd, nv.ptr(dyo.t), dyo.ss, nv.ptr(dxo.t), dxo.ss, nv.ptr(wpk.t), N, D, H, W, cin, cout, nv.stream())
        return {'dx': dxo}, [dyo, wo, wpk, dxo]

    res = over_placements(nv, run, [None, {'dy': 'upper', 'dx': 'gap'}, {'dy': 'lower', 'dx': 'upper'}])
    assert_exact16(planar(res['dx'], cin, shape), ref, dtype, 'convT dx')


# iunet_convT_wgrad (train_misc.hip): tiles of 1 x 8 x 16 (2-D) / 2 x 4 x 16 (3-D); NCI = 2 iff Cin / 32 even; pairs = (Cin / 32 / NCI) (Cout / 32);
# blocks = min(ceil(512 / pairs), tiles) = iunet_convT_wgrad_blocks.  Caps for Cin 32 / 64 / 96: Cout 32: 512 512 171, 64: 256 256 86, 256: 64 64 22.
#   'tiles'  the tile count caps the blocks: 2-D N 3 13 x 40 = 18 tiles, 3-D N 3 3 x 5 x 12 = 12 tiles (ragged on every axis), every channel pair
#   'cap'    more tiles than the cap: 2-D N 3 45 x 72 = 90 tiles, 3-D N 3 5 x 18 x 40 = 135 tiles, the pairs whose cap is below that
CONVT_WGRAD = ([('tiles', nd, 3, sh, ci, co) for nd, sh in ((2, (13, 40)), (3, (3, 5, 12))) for ci in (32, 64, 96) for co in (32, 64, 256)] +
               [('cap', nd, 3, sh, ci, co) for nd, sh in ((2, (45, 72)), (3, (5, 18, 40))) for ci, co in ((32, 256), (64, 256), (96, 256), (96, 64))])


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('branch,nd,N,shape,cin,cout', CONVT_WGRAD)
def test_convT_wgrad(nv, dt, branch, nd, N, shape, cin, cout):
    dtype = DT[dt]
    D, H, W = dhw(nd, shape)
    tz, ty = (2, 4) if nd == 3 else (1, 8)
    tiles = N * -(-D // tz) * -(-H // ty) * -(-W // 16)
    nci = 2 if (cin // 32) % 2 == 0 else 1
    cap = -(-512 // ((cin // 32 // nci) * (cout // 32)))
    nb = nv.lib().iunet_convT_wgrad_blocks(nd, N, D, H, W, cin, cout)
    assert nb == (tiles if branch == 'tiles' else cap) and (tiles < cap) == (branch == 'tiles'), (nb, tiles, cap)
    x, _, _, dy = convT_data(nd, N, shape, cin, cout)
    dW_ref, db_ref = convT_wgrad_ref(nd, N, shape, cin, cout)
    npos = 2 ** nd
    code = nv.DTYPE_CODE[dtype]

    def run(pl):
        xo, dyo = put(x, dtype, pl['x'], 'x'), put(dy, dtype, pl['dy'], 'dy')
        wslab, bslab = scratch(nb * cin * cout * npos, name='wslab'), scratch(nb * cout, name='bslab')      # every row is written: NaN-filled
        dW, db = scratch(cin * cout * npos, name='dW'), scratch(cout, name='db')
        nv.call('iunet_convT_wgrad', code, nd, nv.ptr(xo.t), xo.ss, nv.ptr(dyo.t), dyo.ss, nv.ptr(wslab.t), nv.ptr(bslab.t), nv.ptr(dW.t), nv.ptr(db.t),
                N, D, H, W, cin, cout, nv.stream())
        return {'dW': dW, 'db': db}, [xo, dyo, wslab, bslab, dW, db]

    res = over_placements(nv, run, [None, {'x': 'gap', 'dy': 'upper'}, {'x': 'upper', 'dy': 'gap'}])
    assert torch.equal(res['dW'].logical().reshape(dW_ref.shape), dW_ref)
    assert torch.equal(res['db'].logical().reshape(-1), db_ref)


# ---------------------------------------------------------------------------------------------------------------- max-pool
def windows(t, nd):
    """[N, C, *pooled, 2^nd] windows of a tensor on the 2x grid, in the order the kernels scan them (z, y, x; x fastest)."""
    N, C = t.shape[:2]
    if nd == 2:
        H, W = t.shape[2:]
        return t.reshape(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)
    D, H, W = t.shape[2:]
    return t.reshape(N, C, D // 2, 2, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(N, C, D // 2, H // 2, W // 2, 8)


def unwindows(wn, nd):
    N, C = wn.shape[:2]
    if nd == 2:
        Ho, Wo = wn.shape[2:4]
        return wn.reshape(N, C, Ho, Wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, 2 * Ho, 2 * Wo)
    Do, Ho, Wo = wn.shape[2:5]
    return wn.reshape(N, C, Do, Ho, Wo, 2, 2, 2).permute(0, 1, 2, 5, 3, 6, 4, 7).reshape(N, C, 2 * Do, 2 * Ho, 2 * Wo)


def route_first_max(z, dpool, nd):
    """The max-pool backward: dpool goes to the FIRST maximum of each 2^nd window of z."""
    wn = windows(z, nd)
    is_max = wn == wn.max(-1, keepdim=True).values
    first = is_max & (is_max.cumsum(-1) == 1)
    return unwindows(first.to(dpool.dtype) * dpool.unsqueeze(-1), nd)


# iunet_maxpool_fwd / _bwd: one thread per pooled voxel and 8-channel plane, 256 per block: pooled voxels x planes on both sides of 256 and no
# multiple of it -- 2-D 5 x 7 = 35 (C 8: 35, C 32: 140) and 9 x 15 = 135 (C 32: 540); 3-D 3 x 5 x 7 = 105 (C 8: 105, C 32: 420)
MAXPOOL = [(2, 3, (5, 7), 8), (2, 1, (5, 7), 32), (2, 3, (9, 15), 32), (3, 1, (3, 5, 7), 8), (3, 3, (3, 5, 7), 32)]


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('nd,N,osp,C', MAXPOOL)
def test_maxpool_fwd_bwd(nv, dt, nd, N, osp, C):
    """Tie-heavy integer data (values 0..3): the first maximum wins; add_skip 0 (dz starts as the sentinel and must be written everywhere) and 1."""
    dtype = DT[dt]
    g = gen(700 + nd)
    sp = tuple(2 * s for s in osp)
    z = ints(g, 0, 3, (N, C) + sp)
    dp = ints(g, -2, 2, (N, C) + osp)
    dskip = ints(g, -4, 4, (N, C) + sp)
    pooled_ref = windows(z, nd).max(-1).values
    routed = route_first_max(z, dp, nd)
    Do, Ho, Wo = dhw(nd, osp)
    vin, vo = int(np.prod(sp)), int(np.prod(osp))
    code = nv.DTYPE_CODE[dtype]

    def run_fwd(pl):
        zo, po = put(z, dtype, pl['z'], 'z'), out(N, C, vo, dtype, pl['pooled'], 'pooled')
        nv.call('iunet_maxpool_fwd', code, nd, nv.ptr(zo.t), zo.ss, nv.ptr(po.t), po.ss, C, N, Do, Ho, Wo, nv.stream())
        return {'pooled': po}, [zo, po]

    res = over_placements(nv, run_fwd, [None, {'z': 'upper', 'pooled': 'gap'}, {'z': 'gap', 'pooled': 'lower'}])
    assert torch.equal(planar(res['pooled'], C, osp), pooled_ref)

    for add_skip in (0, 1):
        def run_bwd(pl):
            zo, dpo = put(z, dtype, pl['z'], 'z'), put(dp, dtype, pl['dpool'], 'dpool')
            dzo = put(dskip, dtype, pl['dz'], 'dz') if add_skip else out(N, C, vin, dtype, pl['dz'], 'dz')
            dzo.is_input = False          # written in place: only its surroundings must stay
            nv.call('iunet_maxpool_bwd', code, nd, nv.ptr(zo.t), zo.ss, nv.ptr(dpo.t), dpo.ss, nv.ptr(dzo.t), dzo.ss, add_skip, C, N, Do, Ho, Wo, nv.stream())
            return {'dz': dzo}, [zo, dpo, dzo]

        res = over_placements(nv, run_bwd, [None, {'z': 'upper', 'dpool': 'gap', 'dz': 'upper'}, {'z': 'gap', 'dpool': 'lower', 'dz': 'gap'}])
        assert torch.equal(planar(res['dz'], C, sp), routed + dskip if add_skip else routed), add_skip


# ---------------------------------------------------------------------------------------------------------------- first conv
def first_conv_input(g, N, cin, sp3, in_dtype, dtype):
    """The caller's tensor and the values the kernels see: u8 is x / 255 in fp32, then rounded to the storage type (predict.py:30)."""
    if in_dtype == torch.uint8:
        xi = torch.randint(0, 256, (N, cin) + sp3, generator=g, dtype=torch.uint8)
        return xi, (xi.float() / 255.0).to(dtype).double()
    xi = ints(g, -2, 2, (N, cin) + sp3)
    return xi, xi.double()


# iunet_first_conv_fwd / _wgrad / _wgrad_bn: first_conv_kernel<T, ND, CIN> and first_wgrad_kernel<T, ND, CIN> for CIN 1..4; tiles 16 x 32 (2-D) /
# 4 x 8 x 16 (3-D) forward and weight gradient: odd extents that cut the tiles on every axis, more than one tile per axis in x.
# The input is the caller's tensor read through strides: a view of a larger tensor (sample, channel, plane and row pitch larger than the extents).
FIRST = [(nd, cin, ind) for nd in (2, 3) for cin in (1, 2, 3, 4) for ind in ('u8', 'f32')]


def first_conv_shapes(nd):
    return (3, (19, 37)) if nd == 2 else (3, (5, 9, 19))


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('nd,cin,ind', FIRST)
def test_first_conv_fwd(nv, dt, nd, cin, ind):
    """fp32 input holding small integers: bias + ReLU output and both statistics sums bit for bit.  u8 input: x / 255 rounded to the storage type
    is a multiple of 2^-18 (f16) / 2^-15 (bf16) and the weights are -1..1, so where sum |w| x stays below 2^6 / 2^9 every partial sum is exact in
    fp32 in any order and the output is one rounding of the exact value: bit for bit against float64 (asserted on the reference; otherwise one unit
    in the last place); the statistics of u8 data are not exact: the tolerance of test_first_conv."""
    dtype, in_dtype = DT[dt], {'u8': torch.uint8, 'f32': torch.float32}[ind]
    N, shape = first_conv_shapes(nd)
    cout = 32
    g = gen(800 + 10 * nd + cin)
    D, H, W = dhw(nd, shape)
    xi, xv = first_conv_input(g, N, cin, (D, H, W), in_dtype, dtype)
    w = ints(g, -1, 1, (cout, cin) + (3,) * nd)
    bias = ints(g, -3, 3, (cout,))
    conv = F.conv2d if nd == 2 else F.conv3d
    raw = conv(xv.reshape((N, cin) + shape), w.double(), padding=1)
    ref = F.relu(raw + bias.double().view(1, -1, *([1] * nd)))
    taps, vox = 3 ** nd, D * H * W
    code = nv.DTYPE_CODE[dtype]
    nt = nv.lib().iunet_conv3_num_tiles(nd, N, D, H, W)

    def run(pl):
        xs, wo, bo = StridedInput(xi), dev32(w, 'w'), dev32(bias, 'bias')
        wp = scratch(nv.lib().iunet_pack_first_conv_elems(cout, cin, taps), dtype, name='wpk')
        yo = out(N, cout, vox, dtype, pl['y'], 'y')
        st = scratch(nt * cout * 2, name='stats')          # one row per tile, every row written
        nv.call('iunet_pack_first_conv', code, nv.ptr(wo.t), None, nv.ptr(wp.t), cout, cin, taps, nv.stream())
        nv.call('iunet_first_conv_fwd', code, nd, nv.ptr(xs.t), nv.IN_DTYPE_CODE[in_dtype], nv.ll_array(xs.strides), nv.ptr(yo.t), yo.ss, nv.ptr(wp.t),
                nv.ptr(bo.t), nv.ptr(st.t), N, D, H, W, cin, cout, 1, nv.stream())
        return {'y': yo, 'stats': st}, [xs, wo, bo, wp, yo, st]

    res = over_placements(nv, run, [None, {'y': 'upper'}, {'y': 'gap'}])
    got = planar(res['y'], cout, shape)
    bound = conv(xv.abs().reshape((N, cin) + shape), w.abs().double(), padding=1).max().item() + 3          # every partial sum, bias included
    if ind == 'f32' or bound < (2 ** 6 if dtype == torch.float16 else 2 ** 9):
        want = ref.to(dtype).float()         # one correct rounding of the exact value (the integers are far below the exact range)
        assert torch.equal(got, want), (got - want).abs().max()
    else:
        assert_ulp16(got, ref, dtype, 'first conv y')
    s = res['stats'].logical().reshape(nt, cout, 2).double().sum(0)
    dims = [0] + list(range(2, 2 + nd))
    if ind == 'f32':
        assert torch.equal(s[:, 0], raw.sum(dims)) and torch.equal(s[:, 1], (raw * raw).sum(dims))
    else:
        assert torch.allclose(s[:, 0], raw.sum(dims), rtol=1e-4, atol=1e-2)
        assert torch.allclose(s[:, 1], (raw * raw).sum(dims), rtol=1e-4, atol=1e-2)


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('nd,cin,ind', FIRST)
def test_first_conv_wgrad(nv, dt, nd, cin, ind):
    """dW = sum dy (x) shifted x with dy in -1..1.  fp32 input holding small integers: bit for bit.  u8 input (x / 255, not integers: sums over
    thousands of voxels are not exact in fp32): float64 reference at the tolerance of test_gpu_train.test_first_conv_wgrad (rtol 1e-4, atol 1e-3).
    iunet_first_conv_wgrad_blocks rows of slab."""
    dtype, in_dtype = DT[dt], {'u8': torch.uint8, 'f32': torch.float32}[ind]
    N, shape = first_conv_shapes(nd)
    cout = 32
    g = gen(900 + 10 * nd + cin)
    D, H, W = dhw(nd, shape)
    xi, xv = first_conv_input(g, N, cin, (D, H, W), in_dtype, dtype)
    dy = ints(g, -1, 1, (N, cout) + shape)
    ref = first_wgrad_ref(xv.reshape((N, cin) + shape), dy.double(), nd)
    taps = 3 ** nd
    code = nv.DTYPE_CODE[dtype]
    nb = nv.lib().iunet_first_conv_wgrad_blocks(nd, N, D, H, W)

    def run(pl):
        xs, dyo = StridedInput(xi), put(dy, dtype, pl['dy'], 'dy')
        slab, dW = scratch(nb * cout * 112, name='slab'), scratch(cout * cin * taps, name='dW')
        nv.call('iunet_first_conv_wgrad', code, nd, nv.ptr(xs.t), nv.IN_DTYPE_CODE[in_dtype], nv.ll_array(xs.strides), nv.ptr(dyo.t), dyo.ss,
                nv.ptr(slab.t), nv.ptr(dW.t), N, D, H, W, cin, cout, nv.stream())
        return {'dW': dW}, [xs, dyo, slab, dW]

    res = over_placements(nv, run, [None, {'dy': 'gap'}, {'dy': 'upper'}])
    got = res['dW'].logical().reshape(ref.shape).double()
    if ind == 'f32':
        assert torch.equal(got, ref), (got - ref).abs().max()
    else:
        assert torch.allclose(got, ref, rtol=1e-4, atol=1e-3), (got - ref).abs().max()


def first_wgrad_ref(x, dy, nd):
    """dW [Cout][Cin][3^nd] of a 3^nd pad-1 conv in float64, by autograd."""
    w = torch.zeros((dy.shape[1], x.shape[1]) + (3,) * nd, dtype=torch.float64, requires_grad=True)
    ((F.conv2d if nd == 2 else F.conv3d)(x, w, padding=1) * dy).sum().backward()
    return w.grad


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('nd,cin,ind', [(nd, cin, ind) for nd in (2, 3) for cin, ind in ((1, 'u8'), (2, 'f32'), (3, 'u8'), (4, 'f32'))])
def test_first_conv_wgrad_bn(nv, dt, nd, cin, ind):
    """iunet_first_conv_wgrad_bn against the composition it replaces, in float64: dy = a (dz' - c1 - xhat c2) with dz' = dz where
    round_T(relu(scale y + shift)) > 0, rounded to the storage type as iunet_bn_relu_bwd stores it, then the plain weight gradient of dy.
    Tolerance: test_first_conv_wgrad's rtol 1e-4, but its atol 1e-3 does not cover this composition in either dtype: fp32 and float64 arithmetic
    round a few elements of dy to different neighbours, each moving a dW entry by ulp(dy) |x|.  Measured on these inputs, an fp32 torch CPU
    evaluation of the same composition against the float64 one: max |error| 1.97e-3 (f16, 3-D, Cin 2; 9.8e-4 in bf16); four times that: atol 8e-3."""
    dtype, in_dtype = DT[dt], {'u8': torch.uint8, 'f32': torch.float32}[ind]
    N, shape = first_conv_shapes(nd)
    cout = 32
    g = gen(950 + 10 * nd + cin)
    D, H, W = dhw(nd, shape)
    xi, xv = first_conv_input(g, N, cin, (D, H, W), in_dtype, dtype)
    bn = bn_inputs(g, N, cout, shape, dtype)
    dz = roundT(torch.randn((N, cout) + shape, generator=g), dtype)
    d = dz * (bn['z'] > 0)
    cnt = N * D * H * W
    dims = [0] + list(range(2, 2 + nd))
    bc = lambda v: v.double().view(1, -1, *([1] * nd))
    xhat = (bn['y'] - bc(bn['mean'])) * bc(bn['invstd'])
    s1, s2 = d.sum(dims), (d * xhat).sum(dims)
    coef = torch.stack([bn['gamma'].double() * bn['invstd'].double(), s1 / cnt, s2 / cnt], 1).float()      # [C][3]: a, c1, c2, as iunet_bn_relu_bwd leaves them
    cf = coef.double()
    dy = roundT(bc(cf[:, 0]) * (d - bc(cf[:, 1]) - xhat * bc(cf[:, 2])), dtype)
    ref = first_wgrad_ref(xv.reshape((N, cin) + shape), dy, nd)
    taps = 3 ** nd
    code = nv.DTYPE_CODE[dtype]
    nb = nv.lib().iunet_first_conv_wgrad_blocks(nd, N, D, H, W)

    def run(pl):
        xs, dzo, yo = StridedInput(xi), put(dz, dtype, pl['dz'], 'dz'), put(bn['y'], dtype, pl['y'], 'y')
        par = {k: dev32(bn[k], k) for k in ('mean', 'invstd', 'scale', 'shift')}
        co = dev32(coef, 'coef')
        slab, dW = scratch(nb * cout * 112, name='slab'), scratch(cout * cin * taps, name='dW')
        nv.call('iunet_first_conv_wgrad_bn', code, nd, nv.ptr(xs.t), nv.IN_DTYPE_CODE[in_dtype], nv.ll_array(xs.strides), nv.ptr(dzo.t), dzo.ss,
                nv.ptr(yo.t), yo.ss, nv.ptr(par['mean'].t), nv.ptr(par['invstd'].t), nv.ptr(co.t), nv.ptr(par['scale'].t), nv.ptr(par['shift'].t),
                nv.ptr(slab.t), nv.ptr(dW.t), N, D, H, W, cin, cout, nv.stream())
        return {'dW': dW}, [xs, dzo, yo, co, slab, dW] + list(par.values())

    res = over_placements(nv, run, [None, {'dz': 'gap', 'y': 'upper'}, {'dz': 'upper', 'y': 'gap'}])
    got = res['dW'].logical().reshape(ref.shape).double()
    assert torch.allclose(got, ref, rtol=1e-4, atol=8e-3), (got - ref).abs().max()


# ---------------------------------------------------------------------------------------------------------------- 3^d stage conv
def conv3_run(nv, dtype, nd, x, w, layout, mode, pl, bias=None, epi=0, stats=False):
    """iunet_conv3_fwd on x [N, C, *sp]; w [Cout, Cin, 3..]; mode 1: the data-gradient operator (launch channels swapped)."""
    N = x.shape[0]
    sp = tuple(x.shape[2:])
    D, H, W = dhw(nd, sp)
    taps, vox = 3 ** nd, D * H * W
    co_l, ci_l = (w.shape[0], w.shape[1]) if mode == 0 else (w.shape[1], w.shape[0])
    assert x.shape[1] == ci_l
    pmode = mode | (6 if layout == 3 else 2)
    code = nv.DTYPE_CODE[dtype]
    xo, wo = put(x, dtype, pl['x'], 'x'), dev32(w, 'w')
    wpk = scratch(nv.pack_conv3_elems(w.shape[0], w.shape[1], taps, pmode), dtype, name='wpk')
    yo = out(N, co_l, vox, dtype, pl['y'], 'y')
    ops = [xo, wo, wpk, yo]
    bo = st = None
    if bias is not None:
        bo = dev32(bias, 'bias')
        ops.append(bo)
    outs = {'y': yo}
    if stats:
        rows = nv.lib().iunet_conv3_stats_parts(nd, N, D, H, W, co_l, layout)
        st = scratch(rows * co_l * 2, name='stats')          # one row per workgroup, every row written
        ops.append(st)
        outs['stats'] = st
    nv.call('iunet_pack_conv3', code, nv.ptr(wo.t), None, nv.ptr(wpk.t), w.shape[0], w.shape[1], taps, pmode, nv.stream())
    nv.call('iunet_conv3_fwd', code, nd, nv.ptr(xo.t), xo.ss, nv.ptr(yo.t), yo.ss, nv.ptr(wpk.t), None if bo is None else nv.ptr(bo.t),
            None if st is None else nv.ptr(st.t), N, D, H, W, ci_l, co_l, epi, layout, nv.stream())
    return outs, ops


@functools.lru_cache(maxsize=None)
def conv3_data(nd, N, shape, cin, cout):
    g = gen(1000 + nd)
    x = ints(g, -2, 2, (N, cin) + shape)
    w = ints(g, -1, 1, (cout, cin) + (3,) * nd)
    bias = ints(g, -3, 3, (cout,))
    dy = ints(g, -2, 2, (N, cout) + shape)
    conv = F.conv2d if nd == 2 else F.conv3d
    ref = conv(x, w, padding=1)
    dgrad = (F.conv_transpose2d if nd == 2 else F.conv_transpose3d)(dy, w, padding=1)
    return x, w, bias, dy, ref, dgrad


# iunet_conv3_fwd, layouts 2 (padded K16 operator) and 3 (compact; iunet_conv3_compact_ok: 2-D every channel count, 3-D Cin > 32): one ragged grid
# per (nd, layout), N 3, Cin = 2c = 64 as the decoder's first conv reads a concat buffer whole, y into the upper half of the next one.  The data
# gradient (mode 1) runs the same kernel with 64 launch input channels too (w [64][32]).
@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('nd,shape,layout', [(2, (20, 70), 2), (2, (20, 70), 3), (3, (9, 7, 17), 2), (3, (9, 7, 17), 3)])
def test_conv3_fwd_placements(nv, dt, nd, shape, layout):
    dtype = DT[dt]
    N, cin, cout = 3, 64, 32
    D, H, W = dhw(nd, shape)
    if layout == 3:
        assert nv.lib().iunet_conv3_compact_ok(nd, N, D, H, W, cin, cout, 0, 0) == 1
    # 3-D: 3 x 3 x 1 x 2 tiles of 4 x 8 x 16 on one Cout block = 18 < 128: the half-size tile, tiles walked singly (the paired walk of the big grids has
    # test_conv3_tile_pairs_exact_integers)
    assert nv.lib().iunet_conv3_tile_pairs(nd, N, D, H, W, cin, cout) == 0
    x, w, bias, _, ref, _ = conv3_data(nd, N, shape, cin, cout)
    rows = [None, {'x': 'gap', 'y': 'upper'}, {'x': 'lower', 'y': 'gap'}]
    dims = [0] + list(range(2, 2 + nd))
    # raw output with statistics rows
    res = over_placements(nv, lambda pl: conv3_run(nv, dtype, nd, x, w, layout, 0, pl, stats=True), rows)
    assert_exact16(planar(res['y'], cout, shape), ref, dtype, 'conv3 y')
    st = res['stats'].logical().reshape(-1, cout, 2).double().sum(0)
    assert (ref * ref).sum(dims).max().item() < 2 ** 24          # non-negative integer terms: every partial sum exact in fp32, in any order
    assert torch.equal(st[:, 0], ref.double().sum(dims)) and torch.equal(st[:, 1], (ref.double() ** 2).sum(dims))
    # bias + ReLU epilogue
    res = over_placements(nv, lambda pl: conv3_run(nv, dtype, nd, x, w, layout, 0, pl, bias=bias, epi=2), rows)
    assert_exact16(planar(res['y'], cout, shape), F.relu(ref + bias.view(1, -1, *([1] * nd))), dtype, 'conv3 bias relu')
    # the data gradient: w2 [64 out][32 in], dy with 64 channels -> dx with 32
    _, w2, _, dy2, _, dgrad2 = conv3_data(nd, N, shape, cout, cin)          # the launch has the same 64 -> 32 channels: the same answer of compact_ok
    res = over_placements(nv, lambda pl: conv3_run(nv, dtype, nd, dy2, w2, layout, 1, pl), rows)
    assert_exact16(planar(res['y'], cout, shape), dgrad2, dtype, 'conv3 dgrad')


# iunet_conv3_wgrad / _wgrad_act (conv3_wgrad.hip, wgrad_impl): nblk = (Cout / 32)(Cin / 32), nb = iunet_conv3_wgrad_blocks;
#   'block'  nblk >= 128 and nb <= 4: the LDS-transposing reduce, one workgroup per filter block -- Cin 256 x Cout 512 (nblk 128; nb = 2 in 3-D, 4 rows in 2-D)
#   'plain'  everything else -- Cin 64 x Cout 32
# ragged grids, N 3; x a concat buffer read whole (tight) / with gaps, dy with gaps / in a slot
CONV3_WGRAD = [('plain', 2, (20, 70), 64, 32), ('plain', 3, (5, 9, 17), 64, 32), ('block', 2, (9, 37), 256, 512), ('block', 3, (3, 5, 17), 256, 512)]


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('branch,nd,shape,cin,cout', CONV3_WGRAD)
def test_conv3_wgrad_placements(nv, dt, branch, nd, shape, cin, cout):
    """The plain form on x, and the _act form on (x, scale, shift) with powers of two for scale and integers for shift, so that
    relu(scale x + shift) of integer data is exact: both bit for bit against autograd on the materialised activation."""
    dtype = DT[dt]
    N = 3
    D, H, W = dhw(nd, shape)
    nb = nv.lib().iunet_conv3_wgrad_blocks(nd, N, D, H, W, cin, cout)
    assert ((cout // 32) * (cin // 32) >= 128 and nb <= 4) == (branch == 'block'), nb
    g = gen(1100 + nd)
    x = ints(g, -2, 2, (N, cin) + shape)
    dy = ints(g, -1, 1, (N, cout) + shape)
    scale = 2.0 ** torch.randint(0, 2, (cin,), generator=g).float()          # 1 or 2
    shift = ints(g, -1, 1, (cin,))
    bc = lambda v: v.view(1, -1, *([1] * nd))
    act = F.relu(bc(scale) * x + bc(shift))                                   # integers 0..5
    taps = 3 ** nd
    code = nv.DTYPE_CODE[dtype]
    nfl = nv.lib().iunet_conv3_wgrad_slab_floats(nd, N, D, H, W, cin, cout)
    rows = [None, {'x': 'gap', 'dy': 'gap'}, {'x': 'lower', 'dy': 'upper'}]
    for fused, src in ((False, x), (False, act), (True, x)):
        ref = first_wgrad_ref(act.double() if fused else src.double(), dy.double(), nd).float()

        def run(pl):
            xo, dyo = put(src, dtype, pl['x'], 'x'), put(dy, dtype, pl['dy'], 'dy')
            slab, dW = scratch(nfl, name='slab'), scratch(cout * cin * taps, name='dW')
            ops = [xo, dyo, slab, dW]
            if fused:
                so, ho = dev32(scale, 'x_scale'), dev32(shift, 'x_shift')
                ops += [so, ho]
                nv.call('iunet_conv3_wgrad_act', code, nd, nv.ptr(xo.t), xo.ss, nv.ptr(dyo.t), dyo.ss, nv.ptr(slab.t), nv.ptr(dW.t), 1.0, nv.ptr(so.t),
                        nv.ptr(ho.t), N, D, H, W, cin, cout, nv.stream())
            else:
                nv.call('iunet_conv3_wgrad', code, nd, nv.ptr(xo.t), xo.ss, nv.ptr(dyo.t), dyo.ss, nv.ptr(slab.t), nv.ptr(dW.t), 1.0, N, D, H, W, cin,
                        cout, nv.stream())
            return {'dW': dW}, ops

        res = over_placements(nv, run, rows)
        assert torch.equal(res['dW'].logical().reshape(ref.shape), ref), (fused, (res['dW'].logical().reshape(ref.shape) - ref).abs().max())


# ---------------------------------------------------------------------------------------------------------------- BatchNorm + ReLU
def bcast(v, nd):
    return v.double().view(1, -1, *([1] * nd))


def bn_inputs(g, N, C, shape, dtype):
    """Inputs of the BatchNorm + ReLU kernels, every tensor already rounded to the type it is stored in (y: dtype; parameters: fp32), and the float64
    evaluation of the forward on them.  t = scale y + shift stays clear of the ReLU kink: an element within 2^-10 of it is moved away (fp32-versus-float64
    arithmetic could otherwise flip its mask, which enters the sums), and `clear` = |t| >= 2^-6 marks the elements compared one by one."""
    nd = len(shape)
    dims = [0] + list(range(2, 2 + nd))
    y = roundT(torch.randn((N, C) + tuple(shape), generator=g) * 3 + 0.3, dtype)
    gamma = (2 + torch.rand(C, generator=g)).float()
    beta = (0.2 * torch.randn(C, generator=g)).float()
    mean = y.mean(dims).float()
    invstd = (1 / torch.sqrt(y.var(dims, unbiased=False) + 1e-5)).float()
    scale = gamma * invstd
    shift = beta - mean * scale
    t = bcast(scale, nd) * y + bcast(shift, nd)
    y = torch.where(t.abs() < 2.0 ** -10, roundT(y + 0.25, dtype), y)
    t = bcast(scale, nd) * y + bcast(shift, nd)
    assert t.abs().min().item() >= 2.0 ** -10
    clear = t.abs() >= 2.0 ** -6
    assert (~clear).float().mean().item() <= 0.01          # on the reference alone
    return dict(y=y, gamma=gamma, beta=beta, mean=mean, invstd=invstd, scale=scale, shift=shift, t=t, z=roundT(F.relu(t), dtype), clear=clear)


def bn_bwd_ref(bn, dz, nd, rows=None):
    """dy, dgamma, dbeta, coef [C][3] of z = relu(bn(y)) in float64; the ReLU mask is that of the STORED z.  rows: [parts][C][2] fp32 partial sums to
    take (s1, s2) from (iunet_bn_relu_bwd_apply), else they are summed here."""
    dims = [0] + list(range(2, 2 + nd))
    cnt = bn['y'].numel() / bn['y'].shape[1]
    d = dz * (bn['z'] > 0)
    xhat = (bn['y'] - bcast(bn['mean'], nd)) * bcast(bn['invstd'], nd)
    if rows is None:
        s1, s2 = d.sum(dims), (d * xhat).sum(dims)
    else:
        s1, s2 = rows.double().sum(0)[:, 0], rows.double().sum(0)[:, 1]
    a = bn['gamma'].double() * bn['invstd'].double()
    dy = bcast(a, nd) * (d - bcast(s1 / cnt, nd) - xhat * bcast(s2 / cnt, nd))
    return dy, s2, s1, torch.stack([a, s1 / cnt, s2 / cnt], 1)


def assert_bn_sums(res, dgamma, dbeta, coef, cnt, what):
    """fp32 reductions at the tolerances of test_bn_relu_fwd_bwd (rtol 2e-3, atol 2e-2; the coefficients c1, c2 are the sums over the count)."""
    assert torch.allclose(res['dgamma'].logical().reshape(-1).double(), dgamma, rtol=2e-3, atol=2e-2), what
    assert torch.allclose(res['dbeta'].logical().reshape(-1).double(), dbeta, rtol=2e-3, atol=2e-2), what
    c = res['coef'].logical().reshape(-1, 3).double()
    assert torch.allclose(c[:, 0], coef[:, 0], rtol=1e-6, atol=0), what          # gamma * invstd: one fp32 product
    assert torch.allclose(c[:, 1:], coef[:, 1:], rtol=2e-3, atol=2e-2 / cnt), what


def bn_params(bn):
    return {k: dev32(bn[k], k) for k in ('mean', 'invstd', 'gamma', 'scale', 'shift')}


# iunet_bn_relu_fwd / _bwd / _bwd_apply: pass 1 takes BN_BWD_PER_BLOCK = 2048 voxels per workgroup (= a row of the slab, iunet_bn_bwd_num_parts),
# the forward and pass 2 take 512 per workgroup: vox 455 (below both), 1001 (between), 2431 (above both), multiples of neither; C / 8 = 1, 4, 9 planes
BN_ROWS = [None, {'y': 'upper', 'z': 'gap', 'dz': 'gap', 'dy': 'upper'}, {'y': 'gap', 'z': 'lower', 'dz': 'upper', 'dy': 'gap'}]


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('N,vox', [(3, 455), (1, 1001), (3, 2431)])
@pytest.mark.parametrize('C', [8, 32, 72])
def test_bn_relu_fwd_bwd(nv, dt, C, N, vox):
    dtype = DT[dt]
    code = nv.DTYPE_CODE[dtype]
    g = gen(1200 + C + vox)
    sp = (vox,)
    bn = bn_inputs(g, N, C, sp, dtype)
    dz = roundT(torch.randn((N, C) + sp, generator=g), dtype)
    nparts = nv.lib().iunet_bn_bwd_num_parts(N, vox)
    assert nparts == N * -(-vox // 2048)

    def run_fwd(pl):
        yo, zo, par = put(bn['y'], dtype, pl['y'], 'y'), out(N, C, vox, dtype, pl['z'], 'z'), bn_params(bn)
        nv.call('iunet_bn_relu_fwd', code, nv.ptr(yo.t), yo.ss, nv.ptr(zo.t), zo.ss, nv.ptr(par['scale'].t), nv.ptr(par['shift'].t), C, N, vox, nv.stream())
        return {'z': zo}, [yo, zo] + list(par.values())

    res = over_placements(nv, run_fwd, BN_ROWS)
    assert_ulp16(planar(res['z'], C, sp), bn['z'], dtype, 'z')

    dy_ref, dgamma, dbeta, coef = bn_bwd_ref(bn, dz, 1)
    for variant in ('z', 'no z', 'dy NULL'):
        def run_bwd(pl):
            yo, dzo, par = put(bn['y'], dtype, pl['y'], 'y'), put(dz, dtype, pl['dz'], 'dz'), bn_params(bn)
            zo = put(bn['z'], dtype, pl['z'], 'z') if variant == 'z' else None
            dyo = None if variant == 'dy NULL' else out(N, C, vox, dtype, pl['dy'], 'dy')
            slab, co, dg, db = scratch(nparts * C * 2, name='slab'), scratch(3 * C, name='coef'), scratch(C, name='dgamma'), scratch(C, name='dbeta')
            nv.call('iunet_bn_relu_bwd', code, nv.ptr(dzo.t), dzo.ss, None if zo is None else nv.ptr(zo.t), 0 if zo is None else zo.ss, nv.ptr(yo.t), yo.ss,
                    None if dyo is None else nv.ptr(dyo.t), 0 if dyo is None else dyo.ss, nv.ptr(par['mean'].t), nv.ptr(par['invstd'].t),
                    nv.ptr(par['gamma'].t), nv.ptr(par['scale'].t), nv.ptr(par['shift'].t), nv.ptr(dg.t), nv.ptr(db.t), nv.ptr(slab.t), nv.ptr(co.t),
                    C, N, vox, nv.stream())
            outs = {'dgamma': dg, 'dbeta': db, 'coef': co}
            if dyo is not None:
                outs['dy'] = dyo
            return outs, [o for o in (yo, dzo, zo, dyo, slab, co, dg, db) if o is not None] + list(par.values())

        res = over_placements(nv, run_bwd, BN_ROWS)
        assert_bn_sums(res, dgamma, dbeta, coef, N * vox, variant)
        if 'dy' in res:
            assert_ulp16(planar(res['dy'], C, sp), dy_ref, dtype, f'dy ({variant})', bn['clear'])

    # iunet_bn_relu_bwd_apply on rows of (s1, s2) computed here in float64 and rounded to fp32: on its own, not through the dgrad that writes them
    d = dz * (bn['z'] > 0)
    xhat = (bn['y'] - bcast(bn['mean'], 1)) * bcast(bn['invstd'], 1)
    cuts = [0, vox // 3, vox // 2, vox]
    rows = torch.stack([torch.stack([d[:, :, a:b].sum((0, 2)), (d * xhat)[:, :, a:b].sum((0, 2))], 1) for a, b in zip(cuts, cuts[1:])]).float()
    dy_ref, dgamma, dbeta, coef = bn_bwd_ref(bn, dz, 1, rows)

    def run_apply(pl):
        yo, dzo, par = put(bn['y'], dtype, pl['y'], 'y'), put(dz, dtype, pl['dz'], 'dz'), bn_params(bn)
        dyo = out(N, C, vox, dtype, pl['dy'], 'dy')
        slab, co, dg, db = dev32(rows, 'slab rows'), scratch(3 * C, name='coef'), scratch(C, name='dgamma'), scratch(C, name='dbeta')
        nv.call('iunet_bn_relu_bwd_apply', code, nv.ptr(dzo.t), dzo.ss, nv.ptr(yo.t), yo.ss, nv.ptr(dyo.t), dyo.ss, nv.ptr(par['mean'].t),
                nv.ptr(par['invstd'].t), nv.ptr(par['gamma'].t), nv.ptr(par['scale'].t), nv.ptr(par['shift'].t), nv.ptr(dg.t), nv.ptr(db.t), nv.ptr(slab.t),
                rows.shape[0], nv.ptr(co.t), C, N, vox, nv.stream())
        return {'dgamma': dg, 'dbeta': db, 'coef': co, 'dy': dyo}, [yo, dzo, dyo, slab, co, dg, db] + list(par.values())

    res = over_placements(nv, run_apply, BN_ROWS)
    assert_bn_sums(res, dgamma, dbeta, coef, N * vox, 'apply')
    assert_ulp16(planar(res['dy'], C, sp), dy_ref, dtype, 'dy (apply)', bn['clear'])


def sixteenths(g, shape):
    """Gradients in multiples of 1/16 up to 4: the sum of two is exact in f16 and in bf16 (at most 8 significant bits)."""
    return torch.randint(-64, 65, shape, generator=g).double() / 16


# iunet_bn_relu_pool_fwd / _pool_bwd: one thread per POOLED voxel and plane; the forward and pass 2 take 256 pooled voxels per workgroup, pass 1
# BN_POOL_PER_BLOCK = 8192 input voxels = 2048 pooled (2-D) / 1024 pooled (3-D) per workgroup and slab row (the pooled chunk rule, norm_pool_chunks):
# pooled 9 x 15 = 135 and 3 x 5 x 7 = 105 (below 256), 33 x 65 = 2145 (above 2048) and 7 x 11 x 15 = 1155 (above 1024), multiples of none
POOL_ROWS = [None, {'y': 'upper', 'z': 'upper', 'pooled': 'gap', 'dskip': 'upper', 'dpool': 'gap', 'dy': 'gap'},
             {'y': 'gap', 'z': 'gap', 'pooled': 'lower', 'dskip': 'gap', 'dpool': 'upper', 'dy': 'upper'}]


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('nd,N,osp', [(2, 3, (9, 15)), (2, 1, (33, 65)), (3, 3, (3, 5, 7)), (3, 1, (7, 11, 15))])
@pytest.mark.parametrize('C', [8, 32, 72])
def test_bn_relu_pool_fwd_bwd(nv, dt, C, nd, N, osp):
    dtype = DT[dt]
    code = nv.DTYPE_CODE[dtype]
    g = gen(1300 + C + nd)
    sp = tuple(2 * s for s in osp)
    vox, ovox = int(np.prod(sp)), int(np.prod(osp))
    Do, Ho, Wo = dhw(nd, osp)
    bn = bn_inputs(g, N, C, sp, dtype)
    dskip, dpool = sixteenths(g, (N, C) + sp), sixteenths(g, (N, C) + osp)

    def run_fwd(pl):
        yo, zo, po, par = put(bn['y'], dtype, pl['y'], 'y'), out(N, C, vox, dtype, pl['z'], 'z'), out(N, C, ovox, dtype, pl['pooled'], 'pooled'), bn_params(bn)
        nv.call('iunet_bn_relu_pool_fwd', code, nd, nv.ptr(yo.t), yo.ss, nv.ptr(zo.t), zo.ss, nv.ptr(po.t), po.ss, nv.ptr(par['scale'].t),
                nv.ptr(par['shift'].t), C, N, Do, Ho, Wo, nv.stream())
        return {'z': zo, 'pooled': po}, [yo, zo, po] + list(par.values())

    res = over_placements(nv, run_fwd, POOL_ROWS)
    assert_ulp16(planar(res['z'], C, sp), bn['z'], dtype, 'z')
    assert_ulp16(planar(res['pooled'], C, osp), windows(bn['z'], nd).max(-1).values, dtype, 'pooled')

    dz = dskip + route_first_max(bn['z'], dpool, nd)
    assert torch.equal(roundT(dz, dtype), dz)          # exact in the storage type: the rounding of the fused sum is no source of error
    dy_ref, dgamma, dbeta, coef = bn_bwd_ref(bn, dz, nd)
    nparts = nv.lib().iunet_bn_bwd_num_parts(N, vox)

    def run_bwd(pl):
        yo, dso, dpo, par = put(bn['y'], dtype, pl['y'], 'y'), put(dskip, dtype, pl['dskip'], 'dskip'), put(dpool, dtype, pl['dpool'], 'dpool'), bn_params(bn)
        dyo = out(N, C, vox, dtype, pl['dy'], 'dy')
        slab, co, dg, db = scratch(nparts * C * 2, name='slab'), scratch(3 * C, name='coef'), scratch(C, name='dgamma'), scratch(C, name='dbeta')
        nv.call('iunet_bn_relu_pool_bwd', code, nd, nv.ptr(dso.t), dso.ss, nv.ptr(dpo.t), dpo.ss, nv.ptr(yo.t), yo.ss, nv.ptr(dyo.t), dyo.ss,
                nv.ptr(par['mean'].t), nv.ptr(par['invstd'].t), nv.ptr(par['gamma'].t), nv.ptr(par['scale'].t), nv.ptr(par['shift'].t), nv.ptr(dg.t),
                nv.ptr(db.t), nv.ptr(slab.t), nv.ptr(co.t), C, N, Do, Ho, Wo, nv.stream())
        return {'dgamma': dg, 'dbeta': db, 'coef': co, 'dy': dyo}, [yo, dso, dpo, dyo, slab, co, dg, db] + list(par.values())

    res = over_placements(nv, run_bwd, POOL_ROWS)
    assert_bn_sums(res, dgamma, dbeta, coef, N * vox, 'pool bwd')
    assert_ulp16(planar(res['dy'], C, sp), dy_ref, dtype, 'dy (pool)', bn['clear'])


# ---------------------------------------------------------------------------------------------------------------- GroupNorm + ReLU
def gn_ref(y, gamma, beta, groups, dtype, eps=1e-5):
    """float64 GroupNorm + ReLU forward on y [N, C, *sp]: per-(sample, group) statistics broadcast to the channels, xhat, t, stored z."""
    N, C = y.shape[:2]
    nd = y.dim() - 2
    yg = y.reshape(N, groups, -1)
    mean = yg.mean(-1).repeat_interleave(C // groups, 1)
    invstd = (1 / torch.sqrt(yg.var(-1, unbiased=False) + eps)).repeat_interleave(C // groups, 1)
    ex = lambda v: v.reshape(N, C, *([1] * nd))
    xhat = (y - ex(mean)) * ex(invstd)
    t = xhat * bcast(gamma, nd) + bcast(beta, nd)
    return dict(mean=mean, invstd=invstd, xhat=xhat, t=t, z=roundT(F.relu(t), dtype), clear=t.abs() >= 2.0 ** -6)


def gn_bwd_ref(r, dz, gamma, groups):
    N, C = dz.shape[:2]
    nd = dz.dim() - 2
    dims = [0] + list(range(2, 2 + nd))
    d = dz * (r['z'] > 0)
    gd = d * bcast(gamma, nd)
    grp = lambda v: v.reshape(N, groups, -1).mean(-1).repeat_interleave(C // groups, 1).reshape(N, C, *([1] * nd))
    dy = r['invstd'].reshape(N, C, *([1] * nd)) * (gd - grp(gd) - r['xhat'] * grp(gd * r['xhat']))
    return dy, (d * r['xhat']).sum(dims), d.sum(dims)


def gn_data(g, N, C, sp, dtype):
    y = roundT(torch.randn((N, C) + tuple(sp), generator=g) * 3 + 0.3, dtype)
    gamma = (2 + torch.rand(C, generator=g)).float()          # |t| < 2^-6 on about 0.5 % of the elements
    beta = (0.3 * torch.randn(C, generator=g)).float()
    return y, gamma, beta


def assert_gn_outputs(res, r, dgamma, dbeta, what):
    """statistics and parameter gradients at the tolerances of test_gn_relu_fwd_bwd_vs_torch"""
    N, C = r['mean'].shape
    if 'mean' in res:
        assert torch.allclose(res['mean'].logical().reshape(N, C).double(), r['mean'], rtol=1e-5, atol=1e-5), what
        assert torch.allclose(res['invstd'].logical().reshape(N, C).double(), r['invstd'], rtol=1e-5, atol=1e-6), what
    if 'dgamma' in res:
        assert (res['dgamma'].logical().reshape(-1).double() - dgamma).abs().max() <= 2e-2 * max(1.0, dgamma.abs().max().item()), what
        assert (res['dbeta'].logical().reshape(-1).double() - dbeta).abs().max() <= 2e-2 * max(1.0, dbeta.abs().max().item()), what


# iunet_gn_relu_fwd / _bwd / _pool_fwd / _pool_bwd: the two smallest entries of test_gn_relu_fwd_bwd_vs_torch's shape list, which runs both dtypes
# already; new here: the placements, the bands, the float64 reference.  The pooled forms take the entries as the pooled grid.
GN_SHAPES = [(1, 256, 8, (4, 4, 4)), (2, 32, 8, (5, 7, 9))]
GN_ROWS = [None, {'y': 'gap', 'z': 'upper', 'dz': 'upper', 'dy': 'gap', 'pooled': 'gap', 'dskip': 'gap', 'dpool': 'upper'},
           {'y': 'upper', 'z': 'gap', 'dz': 'gap', 'dy': 'upper', 'pooled': 'upper', 'dskip': 'upper', 'dpool': 'gap'}]


def gn_stat_outs(N, C):
    return {k: scratch(N * C, name=k) for k in ('scale', 'shift', 'mean', 'invstd')}


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('N,C,groups,sp', GN_SHAPES)
def test_gn_relu_fwd_bwd(nv, dt, N, C, groups, sp):
    dtype = DT[dt]
    code = nv.DTYPE_CODE[dtype]
    g = gen(1400 + C)
    y, gamma, beta = gn_data(g, N, C, sp, dtype)
    dz = roundT(torch.randn((N, C) + sp, generator=g), dtype)
    r = gn_ref(y, gamma, beta, groups, dtype)
    assert (~r['clear']).float().mean().item() <= 0.01
    dy_ref, dgamma, dbeta = gn_bwd_ref(r, dz, gamma, groups)
    vox = int(np.prod(sp))
    parts = nv.lib().iunet_gn_num_parts(N, vox)

    def run(pl):
        yo, dzo, go, bo = put(y, dtype, pl['y'], 'y'), put(dz, dtype, pl['dz'], 'dz'), dev32(gamma, 'gamma'), dev32(beta, 'beta')
        zo, dyo = out(N, C, vox, dtype, pl['z'], 'z'), out(N, C, vox, dtype, pl['dy'], 'dy')
        st = gn_stat_outs(N, C)
        slab, co, dg, db = scratch(parts * C * 2, name='slab'), scratch(N * C * 3, name='coef'), scratch(C, name='dgamma'), scratch(C, name='dbeta')
        nv.call('iunet_gn_relu_fwd', code, nv.ptr(yo.t), yo.ss, nv.ptr(zo.t), zo.ss, nv.ptr(go.t), nv.ptr(bo.t), groups, 1e-5, nv.ptr(slab.t),
                nv.ptr(st['scale'].t), nv.ptr(st['shift'].t), nv.ptr(st['mean'].t), nv.ptr(st['invstd'].t), C, N, vox, nv.stream())
        nv.call('iunet_gn_relu_bwd', code, nv.ptr(dzo.t), dzo.ss, nv.ptr(yo.t), yo.ss, nv.ptr(dyo.t), dyo.ss, nv.ptr(go.t), groups, nv.ptr(st['scale'].t),
                nv.ptr(st['shift'].t), nv.ptr(st['mean'].t), nv.ptr(st['invstd'].t), nv.ptr(dg.t), nv.ptr(db.t), nv.ptr(slab.t), nv.ptr(co.t), C, N, vox,
                nv.stream())
        return dict(z=zo, dy=dyo, dgamma=dg, dbeta=db, **st), [yo, dzo, go, bo, zo, dyo, slab, co, dg, db] + list(st.values())

    res = over_placements(nv, run, GN_ROWS)
    assert_gn_outputs(res, r, dgamma, dbeta, 'gn')
    assert_ulp16(planar(res['z'], C, sp), r['z'], dtype, 'z')
    assert_ulp16(planar(res['dy'], C, sp), dy_ref, dtype, 'dy', r['clear'])


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('N,C,groups,osp', GN_SHAPES)
def test_gn_relu_pool_fwd_bwd(nv, dt, N, C, groups, osp):
    dtype = DT[dt]
    code = nv.DTYPE_CODE[dtype]
    nd = 3
    g = gen(1500 + C)
    sp = tuple(2 * s for s in osp)
    y, gamma, beta = gn_data(g, N, C, sp, dtype)
    dskip, dpool = sixteenths(g, (N, C) + sp), sixteenths(g, (N, C) + osp)
    r = gn_ref(y, gamma, beta, groups, dtype)
    assert (~r['clear']).float().mean().item() <= 0.01
    dz = dskip + route_first_max(r['z'], dpool, nd)
    assert torch.equal(roundT(dz, dtype), dz)
    dy_ref, dgamma, dbeta = gn_bwd_ref(r, dz, gamma, groups)
    vox, ovox = int(np.prod(sp)), int(np.prod(osp))
    Do, Ho, Wo = osp
    parts = nv.lib().iunet_gn_num_parts(N, vox)

    def run(pl):
        yo, dso, dpo = put(y, dtype, pl['y'], 'y'), put(dskip, dtype, pl['dskip'], 'dskip'), put(dpool, dtype, pl['dpool'], 'dpool')
        go, bo = dev32(gamma, 'gamma'), dev32(beta, 'beta')
        zo, po, dyo = out(N, C, vox, dtype, pl['z'], 'z'), out(N, C, ovox, dtype, pl['pooled'], 'pooled'), out(N, C, vox, dtype, pl['dy'], 'dy')
        st = gn_stat_outs(N, C)
        slab, co, dg, db = scratch(parts * C * 2, name='slab'), scratch(N * C * 3, name='coef'), scratch(C, name='dgamma'), scratch(C, name='dbeta')
        nv.call('iunet_gn_relu_pool_fwd', code, nd, nv.ptr(yo.t), yo.ss, nv.ptr(zo.t), zo.ss, nv.ptr(po.t), po.ss, nv.ptr(go.t), nv.ptr(bo.t), groups, 1e-5,
                nv.ptr(slab.t), nv.ptr(st['scale'].t), nv.ptr(st['shift'].t), nv.ptr(st['mean'].t), nv.ptr(st['invstd'].t), C, N, Do, Ho, Wo, nv.stream())
        nv.call('iunet_gn_relu_pool_bwd', code, nd, nv.ptr(dso.t), dso.ss, nv.ptr(dpo.t), dpo.ss, nv.ptr(yo.t), yo.ss, nv.ptr(dyo.t), dyo.ss, nv.ptr(go.t),
                groups, nv.ptr(st['scale'].t), nv.ptr(st['shift'].t), nv.ptr(st['mean'].t), nv.ptr(st['invstd'].t), nv.ptr(dg.t), nv.ptr(db.t),
                nv.ptr(slab.t), nv.ptr(co.t), C, N, Do, Ho, Wo, nv.stream())
        return dict(z=zo, pooled=po, dy=dyo, dgamma=dg, dbeta=db, **st), [yo, dso, dpo, go, bo, zo, po, dyo, slab, co, dg, db] + list(st.values())

    res = over_placements(nv, run, GN_ROWS)
    assert_gn_outputs(res, r, dgamma, dbeta, 'gn pool')
    assert_ulp16(planar(res['z'], C, sp), r['z'], dtype, 'z')
    assert_ulp16(planar(res['pooled'], C, osp), windows(r['z'], nd).max(-1).values, dtype, 'pooled')
    assert_ulp16(planar(res['dy'], C, sp), dy_ref, dtype, 'dy', r['clear'])


# ---------------------------------------------------------------------------------------------------------------- head
@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('ncls,C0', [(2, 32), (3, 64), (10, 32)])
def test_head_fwd(nv, dt, ncls, C0):
    """iunet_head_fwd with x at a placement; logits / probs / class map in banded allocations; 3 x 10 x 13 = 390 voxels end inside a 256-voxel chunk.
    float64 reference at the tolerances of test_head_softmax_argmax (1e-5 on logits, 1e-6 on probabilities); the class map is exactly the argmax of
    the probabilities returned."""
    dtype = DT[dt]
    g = gen(1600 + ncls)
    N, shape = 3, (3, 10, 13)
    D, H, W = shape
    vox = D * H * W
    x = roundT(torch.randn((N, C0) + shape, generator=g), dtype)
    w = (torch.randn(ncls, C0, generator=g) * 0.3).float()
    b = (torch.randn(ncls, generator=g) * 0.1).float()
    ref_l = torch.einsum('kc,ncdhw->nkdhw', w.double(), x) + bcast(b, 3)
    ref_p = torch.softmax(ref_l, 1)

    def run(pl):
        xo, wo, bo = put(x, dtype, pl['x'], 'x'), dev32(w, 'w'), dev32(b, 'bias')
        lo, po = Operand(N, ncls * vox, F32, TIGHT, name='logits'), Operand(N, ncls * vox, F32, TIGHT, name='probs')
        co = Operand(N, vox, torch.uint8, TIGHT, name='cls')
        nv.call('iunet_head_fwd', nv.DTYPE_CODE[dtype], nv.ptr(xo.t), xo.ss, C0, nv.ptr(wo.t), nv.ptr(bo.t), ncls, nv.ptr(lo.t), nv.ptr(po.t), nv.ptr(co.t),
                nv.ll_array((ncls * vox, vox, H * W, W, 1)), 1.0, 0, N, D, H, W, nv.stream())
        return {'logits': lo, 'probs': po, 'cls': co}, [xo, wo, bo, lo, po, co]

    res = over_placements(nv, run, [None, {'x': 'gap'}, {'x': 'upper'}])
    logits, probs = res['logits'].logical().reshape(ref_l.shape).double(), res['probs'].logical().reshape(ref_p.shape).double()
    assert (logits - ref_l).abs().max() < 1e-5 and (probs - ref_p).abs().max() < 1e-6
    assert np.array_equal(res['cls'].logical().numpy(), np.argmax(res['probs'].logical().reshape(N, ncls, vox).numpy(), axis=1))


# iunet_head_loss_fwd / _bwd and the _act forms (test_gpu_train._head_loss_case, extended by dtype, batch, placement and the fused activation):
# the backward is the register kernel for (C0 / 8) ncls <= 16 (C0 32 x ncls 4 = 16; iunet_head_loss_bwd_num_parts rows of 2048 voxels) and the LDS
# kernel above (C0 64 x ncls 3 = 24); 20 x 37 = 740 and 40 x 59 = 2360 voxels end inside a 256-voxel chunk, the second past one 2048-voxel row
HEAD_ROWS = [None, {'x': 'gap', 'dx': 'gap'}, {'x': 'upper', 'dx': 'lower'}]


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('act', [False, True])
@pytest.mark.parametrize('C0,ncls,N,shape', [(32, 4, 3, (20, 37)), (64, 3, 1, (40, 59)), (64, 3, 3, (20, 37)), (32, 4, 1, (40, 59))])
def test_head_loss_fwd_bwd(nv, dt, act, C0, ncls, N, shape):
    from tests.test_gpu_train import _head_loss_case
    dtype = DT[dt]
    vox = shape[0] * shape[1]
    wide = (C0 // 8) * ncls > 16
    assert wide == (C0 == 64) and nv.lib().iunet_head_loss_bwd_num_parts(N, vox, ncls, C0) == N * -(-vox // 2048)          # both kernels: 8 x 256 voxels per row
    _head_loss_case(nv, 'dice_ce', True, C0, ncls, shape, dtype=dtype, N=N, places=HEAD_ROWS, act=act,
                    dx_check=lambda got, ref: assert_ulp16(got, ref, dtype, 'head dx'))
