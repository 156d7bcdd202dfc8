"""The fp32 parity-form kernels (csrc/precise_f32.hip, csrc/train_f32.hip and the helpers they lean on) one entry point at a time,
across dispatch branch x input dtype x nd x buffer placement, through the C ABI.

The layout and the rules are those of tests/test_gpu_kernel_matrix.py.  Every operand, parameter vectors included, sits in a NaN-sentinel
arena (tests/arena.py); each case runs with every operand tight first and then once per further placement row, and asserts
  1. the tight result against a reference that owes nothing to the library;
  2. the same bits at every other placement;
  3. intact sentinels around outputs and around exactly sized scratch, inputs unchanged bit for bit;
  4. no unwritten output: outputs and scratch start as the sentinel, a NaN.
Most rows are EXACT.  v_mfma_f32_16x16x4_f32 is a k-ordered fmaf chain and the kernels round every operation on its own, so on small
integers (activations in [-2, 2], weights in [-1, 1], bias in [-3, 3]; every |reference value| asserted below 2^24) the result does
not depend on the order of the sums and fp32 torch on the CPU has the same value.  Integer rows compare by value with NaN refused (a
zero's sign is the only thing that leaves open); rows on real data whose operation order the kernel states (the BatchNorm fold,
bn_relu_fwd, the divisions) compare bit for bit; the remaining rows go against float64 at the bars this project already holds its
fp32 kernels to (tests/test_gpu_train_f32.py), quoted where they are used.

Geometry the shapes are chosen for ("fp32 form: tiles and splits"): the conv and the weight gradient tile 4 x 4 x 16 voxels
in 3-D and 16 x 16 in 2-D, take 32 output channels per workgroup and 8 input channels per chunk (16 in the weight gradient).  The
default grids (5, 6, 18) and (18, 20) give two tiles along every tiled axis with every second tile ragged; pointwise kernels use
vox = 285 = 3 x 5 x 19 (two blocks of 256, the second ragged) and vox = 7.  Batch sizes are 1 and 3.

Every assertion on what the DEVICE produced goes through verify(); assertions on the reference alone and on the launch arithmetic are
plain asserts.  tests/test_f32_matrix_cpu.py runs every body of this file once against a stub binding (DEVICE = 'cpu', verify muted),
where only the plain asserts and the binding's own argument checks can fail.  Needs an MI355X: run with -m gpu."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import metrics_ref
from tests.arena import SENTINEL, Operand, StridedInput, StridedOutput, bits, fold_ref, scratch as _scratch, sqrt_rn

pytestmark = pytest.mark.gpu

F32 = torch.float32
TIGHT = 'tight'
DEVICE = 'cuda'
IN_DTYPES = {'f32': (0, torch.float32), 'f16': (1, torch.float16), 'u8': (2, torch.uint8), 'bf16': (3, torch.bfloat16)}
GRID = {3: (5, 6, 18), 2: (18, 20)}          # two tiles along every tiled axis, every second one ragged
VOXES = {285: (3, 5, 19), 7: (1, 1, 7)}
EXACT_BOUND = float(1 << 24)


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


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


def dhw(nd, shape):
    return tuple(shape) if nd == 3 else (1,) + tuple(shape)


def vol(shape):
    return int(np.prod(shape))


def fin(x, place, name, dtype=F32):
    """An input [N, ...] (CPU) as N samples at a placement."""
    return Operand(x.shape[0], x[0].numel(), dtype, place, x.reshape(x.shape[0], -1), device=DEVICE, name=name)


def fio(x, place, name):
    """A buffer the kernel reads AND writes (accumulate, in place): preset contents, watched like an output."""
    o = fin(x, place, name)
    o.is_input = False
    return o


def fout(N, per, place, name, dtype=F32):
    return Operand(N, per, dtype, place, None, device=DEVICE, name=name)


def vec(t, name, dtype=None):
    """A parameter vector (an input) with bands around it."""
    t = t.reshape(1, -1)
    return Operand(1, t.numel(), dtype or t.dtype, TIGHT, t, device=DEVICE, name=name)


def scratch(n, name, dtype=F32):
    return _scratch(n, dtype, DEVICE, name)


def unwritten(o):
    return int((bits(o.logical()) == SENTINEL[o.dtype]).sum())


def over_placements(run, rows):
    """run(places) -> (outputs {name: operand}, every operand of the call).  rows[0] stands for the all-tight row.  Returns the tight
    outputs' logical contents; asserts 2., 3. and 4. of the module docstring for every row."""
    base = None
    for r, places in enumerate(rows):
        pl = {k: TIGHT for k in rows[-1]} if r == 0 else places
        outs, ops = run(pl)
        sync()
        for o in ops:
            o.check()
            if isinstance(o, Operand) and not o.is_input and not getattr(o, 'partial', False):
                verify(unwritten(o) == 0, f'{o.name} [{pl}]: {unwritten(o)} elements never written')
        got = {k: o.logical() for k, o in outs.items()}
        if base is None:
            base = got
        else:
            for k in got:
                assert torch.equal(bits(base[k]), bits(got[k])), f'{k}: placement {pl} changes the result ({int((bits(base[k]) != bits(got[k])).sum())} elements)'
    return base


def bounded(ref, what):
    assert float(ref.abs().max()) < EXACT_BOUND, f'{what}: the reference leaves the exact range of fp32 integers'
    return ref


def same_value(got, ref, what):
    """Integer rows: the exact value everywhere, no NaN (an unwritten element)."""
    got, ref = got.reshape(-1).float(), ref.reshape(-1).float()
    verify(got.numel() == ref.numel() and not bool(torch.isnan(got).any()) and torch.equal(got, ref),
           f'{what}: {int((got != ref).sum()) if got.numel() == ref.numel() else "size"} of {ref.numel()} elements differ')


def same_bits(got, ref, what):
    got, ref = got.reshape(-1), ref.reshape(-1).to(got.dtype)
    verify(got.numel() == ref.numel() and torch.equal(bits(got), bits(ref)),
           f'{what}: {int((bits(got) != bits(ref)).sum()) if got.numel() == ref.numel() else "size"} of {ref.numel()} elements differ in their bits')


def close(got, ref, rel, what):
    """|got - ref| <= rel x max(1, max |ref|), NaN refused."""
    got, ref = got.reshape(-1).double(), ref.reshape(-1).double()
    err = (got - ref).abs().max().item() if got.numel() else 0.0
    bar = rel * max(1.0, ref.abs().max().item())
    verify(err <= bar, f'{what}: max err {err:.3e} over the bar {bar:.3e}')          # a NaN fails


def planar_strides(ss, C, D, H, W):
    return [ss, D * H * W, H * W, W, 1]


def tiles(nd, grid):
    D, H, W = dhw(nd, grid)
    tz, ty = (4, 4) if nd == 3 else (1, 16)
    return -(-D // tz), -(-H // ty), -(-W // 16)


def assert_ragged_two_tiles(nd, grid):
    D, H, W = dhw(nd, grid)
    tz, ty = (4, 4) if nd == 3 else (1, 16)
    assert tiles(nd, grid) == ((2, 2, 2) if nd == 3 else (1, 2, 2)) and H % ty and W % 16 and (nd == 2 or D % tz), (nd, grid)


# ---------------------------------------------------------------------------------------------------------------- operator packing
def pack_elems(cout, cin, taps):
    """iunet_f32_pack_conv_elems restated: [npos or 1][Cout / 32][chunks of 8 Cin][taps or 1][256]."""
    return (cout // 32) * (-(-cin // 8)) * taps * 256


def packed(nv, w, cout, cin, taps, transposed, bn=None, eps=1e-5):
    """Pack plain weights (conv [Cout][Cin][taps]; transposed [Cin][Cout][taps]) with iunet_f32_pack_conv into exactly sized scratch.
    bn = (gamma, beta, mean, var): the eval-mode fold, bias_out written too.  -> (wpk, bias_out or None, operands)."""
    n = nv.lib().iunet_f32_pack_conv_elems(cout, cin, taps)
    assert n == pack_elems(cout, cin, taps) and w.numel() == cout * cin * taps
    wo, wpk = vec(w, 'w'), scratch(n, 'wpk')
    ops, bo, bnp = [wo, wpk], None, [None] * 4
    if bn is not None:
        bnv = [vec(t, k) for t, k in zip(bn, ('gamma', 'beta', 'mean', 'var'))]
        bo = scratch(cout, 'bias_out')
        ops += bnv + [bo]
        bnp = [nv.ptr(o.t) for o in bnv]
    nv.call('iunet_f32_pack_conv', nv.ptr(wo.t), nv.ptr(wpk.t), None if bo is None else nv.ptr(bo.t), *bnp, float(eps), cout, cin, taps,
            int(transposed), nv.stream())
    return wpk, bo, ops


def conv_call(nv, nd, x_t, strides, code, yo, wpk, bias_t, N, grid, cin, cout, relu, mode):
    D, H, W = dhw(nd, grid)
    nv.call('iunet_f32_conv_fwd', nd, nv.ptr(x_t), code, nv.ll_array(strides), nv.ptr(yo.t), yo.ss, nv.ptr(wpk.t),
            None if bias_t is None else nv.ptr(bias_t), N, D, H, W, cin, cout, int(relu), mode, nv.stream())


# ---------------------------------------------------------------------------------------------------------------- conv, mode 0
SETTINGS = {'nobias_lin': (False, 0), 'bias_relu': (True, 1), 'bias_lin': (True, 0), 'nobias_relu': (False, 1)}
CIN = {1: (1, 1), 3: (1, 3), 8: (1, 0), 12: (2, 4), 40: (5, 0)}          # Cin -> (chunks of 8, channels in the ragged last chunk; 0 = full)


def chunk_name(cin):
    n, tail = CIN[cin]
    return f'cin{cin}_{n}chunk' + (f'_tail{tail}' if tail else '')


@functools.lru_cache(maxsize=None)
def conv_data(nd, N, cin, cout):
    g = gen(100 * nd + cin + cout)
    x = ints(g, -2, 2, (N, cin) + GRID[nd])
    w = ints(g, -1, 1, (cout, cin) + (3,) * nd)
    b = ints(g, -3, 3, (cout,))
    return x, w, b


def conv_nd(nd):
    return F.conv2d if nd == 2 else F.conv3d


@functools.lru_cache(maxsize=None)
def conv_ref(nd, N, cin, cout):
    x, w, _ = conv_data(nd, N, cin, cout)
    return bounded(conv_nd(nd)(x, w, padding=1), 'conv')


def finish(ref, b, bias, relu):
    if bias:
        ref = ref + b.view(1, -1, *([1] * (ref.dim() - 2)))
    return F.relu(ref) if relu else ref


CONV0 = [pytest.param(nd, cin, cout, s, 3, id=f'{nd}d_ragged-{chunk_name(cin)}-cout{cout}_{cout // 32}cob-{s}-N3')
         for nd in (2, 3) for cin in (1, 8, 12, 40) for cout in (32, 64) for s in SETTINGS]
CONV0 += [pytest.param(nd, 12, 64, 'bias_relu', 1, id=f'{nd}d_ragged-{chunk_name(12)}-cout64_2cob-bias_relu-N1') for nd in (2, 3)]
CONV_ROWS = [None, {'x': 'gap', 'y': 'upper'}, {'x': 'upper', 'y': 'lower'}, {'x': 'lower', 'y': 'gap'}]


@pytest.mark.parametrize('nd,cin,cout,setting,N', CONV0)
def test_conv(nv, nd, cin, cout, setting, N):
    """3^d conv from a planar fp32 input at a placement into both halves of a concat buffer; the operator packed from plain weights."""
    assert_ragged_two_tiles(nd, GRID[nd])
    assert (-(-cin // 8), cin % 8) == CIN[cin] and cout // 32 == (2 if cout == 64 else 1)
    bias, relu = SETTINGS[setting]
    x, w, b = conv_data(nd, N, cin, cout)
    ref = bounded(finish(conv_ref(nd, N, cin, cout), b, bias, relu), 'conv')
    D, H, W = dhw(nd, GRID[nd])

    def run(pl):
        xo, yo = fin(x, pl['x'], 'x'), fout(N, cout * D * H * W, pl['y'], 'y')
        wpk, _, ops = packed(nv, w, cout, cin, 3 ** nd, 0)
        bo = vec(b, 'bias') if bias else None
        conv_call(nv, nd, xo.t, planar_strides(xo.ss, cin, D, H, W), 0, yo, wpk, bo.t if bias else None, N, GRID[nd], cin, cout, relu, 0)
        return {'y': yo}, ops + [xo, yo] + ([bo] if bias else [])

    same_value(over_placements(run, CONV_ROWS)['y'], ref, 'conv y')


@functools.lru_cache(maxsize=None)
def typed_input(nd, cin, dt):
    """[N = 3, Cin, D, H, W] in the input dtype: small integers (exact in f16 / bf16), bytes 0 and 255 for u8 (x / 255 is 0 or 1)."""
    g = gen(7 * nd + cin)
    shape = (3, cin) + dhw(nd, GRID[nd])
    if dt == 'u8':
        return (torch.randint(0, 2, shape, generator=g) * 255).to(torch.uint8)
    return ints(g, -2, 2, shape).to(IN_DTYPES[dt][1])


def as_f32(x):
    return x.float() / 255 if x.dtype == torch.uint8 else x.float()


@pytest.mark.parametrize('dt', [pytest.param(k, id=f'{k}_code{v[0]}') for k, v in IN_DTYPES.items()])
@pytest.mark.parametrize('cin', [pytest.param(c, id=chunk_name(c)) for c in (1, 3)])
@pytest.mark.parametrize('nd', [pytest.param(2, id='2d_ragged_padded_pitches'), pytest.param(3, id='3d_ragged_padded_pitches')])
def test_conv_input_dtype_and_pitches(nv, nd, cin, dt):
    """The first conv's loader: dtype codes 0 .. 3 through a view whose row, plane, channel and sample pitch are all padded."""
    code, dtype = IN_DTYPES[dt]
    assert nv.IN_DTYPE_CODE[dtype] == code and (-(-cin // 8), cin % 8) == CIN[cin]
    cout, N = 32, 3
    x = typed_input(nd, cin, dt)
    _, w, b = conv_data(nd, N, cin, cout)
    ref = bounded(finish(conv_nd(nd)(as_f32(x).reshape((N, cin) + GRID[nd]), w, padding=1), b, True, 1), 'conv')
    D, H, W = dhw(nd, GRID[nd])

    def run(pl):
        xs, yo, bo = StridedInput(x, device=DEVICE), fout(N, cout * D * H * W, pl['y'], 'y'), vec(b, 'bias')
        assert all(s > e for s, e in zip(xs.strides[:4], (cin * D * H * W, D * H * W, H * W, W))) and xs.strides[4] == 1
        wpk, _, ops = packed(nv, w, cout, cin, 3 ** nd, 0)
        conv_call(nv, nd, xs.t, xs.strides, code, yo, wpk, bo.t, N, GRID[nd], cin, cout, 1, 0)
        return {'y': yo}, ops + [xs, yo, bo]

    same_value(over_placements(run, [None, {'y': 'gap'}, {'y': 'upper'}])['y'], ref, f'conv y from {dt}')


@pytest.mark.parametrize('view', ['x_slices_of_a_volume_sW_is_X', 'channels_last_u8_sC_is_1'])
def test_conv_views_with_an_x_stride(nv, view):
    """sW != 1.  (a) the 2.5-D view of a [Z, Y, X] volume sliced along x: sample n is the plane x = n, read with sN = 1, sH = Y X, sW = X;
    (b) a channels-last uint8 image [N][H][W][C]."""
    nd, cout = 2, 32
    H, W = GRID[2]
    g = gen(31)
    if view.startswith('x_slices'):
        N, cin, code = 3, 1, 0
        v = ints(g, -2, 2, (H, W, N))          # [Z][Y][X]: Z plays H, Y plays W, X the batch
        x = v.permute(2, 0, 1).reshape(N, 1, H, W)
        raw, strides = v.reshape(1, -1), lambda o: [1, H * W * N, 0, W * N, N]
        assert strides(None)[4] == N != 1
    else:
        N, cin, code = 3, 3, 2
        v = (torch.randint(0, 2, (N, H, W, cin), generator=g) * 255).to(torch.uint8)
        x = as_f32(v).permute(0, 3, 1, 2)
        raw, strides = v.reshape(N, -1), lambda o: [o.ss, 1, 0, W * cin, cin]
    _, w, b = conv_data(nd, N, cin, cout)
    ref = bounded(finish(F.conv2d(x, w, padding=1), b, True, 0), 'conv')

    def run(pl):
        xo, yo, bo = fin(raw, pl['x'], 'x', raw.dtype), fout(N, cout * H * W, pl['y'], 'y'), vec(b, 'bias')
        wpk, _, ops = packed(nv, w, cout, cin, 9, 0)
        conv_call(nv, nd, xo.t, strides(xo), code, yo, wpk, bo.t, N, GRID[2], cin, cout, 0, 0)
        return {'y': yo}, ops + [xo, yo, bo]

    same_value(over_placements(run, [None, {'x': 'gap', 'y': 'upper'}, {'x': 'upper', 'y': 'gap'}])['y'], ref, view)


@functools.lru_cache(maxsize=None)
def all_bytes_image():
    """[3, 3, 18, 20] uint8 in which every channel of every sample holds all 256 byte values."""
    g = gen(255)
    n = vol(GRID[2])
    return torch.stack([torch.cat([torch.randperm(256, generator=g), torch.randint(0, 256, (n - 256,), generator=g)])[torch.randperm(n, generator=g)]
                        for _ in range(9)]).reshape((3, 3) + GRID[2]).to(torch.uint8)


def test_conv_u8_division_is_correctly_rounded(nv):
    """The u8 loader's x / 255 on its own: under the centre-tap identity operator (w[co][ci] = 1 for ci == co % Cin) the output is the
    loaded value, which must have the bits of x.float() / 255 for all 256 bytes."""
    N, cin, cout = 3, 3, 32
    H, W = GRID[2]
    x = all_bytes_image()
    assert all(len(torch.unique(x[n, c])) == 256 for n in range(N) for c in range(cin))
    w = torch.zeros(cout, cin, 3, 3)
    for co in range(cout):
        w[co, co % cin, 1, 1] = 1.0
    ref = (x.float() / 255)[:, [co % cin for co in range(cout)]]

    def run(pl):
        xs, yo = StridedInput(x.reshape(N, cin, 1, H, W), device=DEVICE), fout(N, cout * H * W, pl['y'], 'y')
        wpk, _, ops = packed(nv, w, cout, cin, 9, 0)
        conv_call(nv, 2, xs.t, xs.strides, 2, yo, wpk, None, N, GRID[2], cin, cout, 0, 0)
        return {'y': yo}, ops + [xs, yo]

    same_bits(over_placements(run, [None, {'y': 'gap'}])['y'], ref, 'u8 / 255')


# ---------------------------------------------------------------------------------------------------------------- conv, modes 1 and 2
TGRID = {3: (3, 5, 18), 2: (5, 18)}          # input grids of the transposed conv: ragged tiles, two along x


@functools.lru_cache(maxsize=None)
def convT_data(nd, N, cin, cout):
    g = gen(200 * nd + cin + cout)
    return ints(g, -2, 2, (N, cin) + TGRID[nd]), ints(g, -1, 1, (cin, cout) + (2,) * nd), ints(g, -3, 3, (cout,))


CONVT = [pytest.param(nd, cin, cout, bias, 3, id=f'{nd}d_{2 ** nd}pos-cin{cin}_{-(-cin // 8)}chunk{"_tail4" if cin % 8 else ""}-cout{cout}_{cout // 32}cob-{"bias" if bias else "nobias"}-N3')
         for nd in (2, 3) for cin, cout in ((64, 32), (12, 64)) for bias in (True, False)]
CONVT += [pytest.param(3, 12, 64, True, 1, id='3d_8pos-cin12_2chunk_tail4-cout64_2cob-bias-N1')]


@pytest.mark.parametrize('nd,cin,cout,bias,N', CONVT)
def test_conv_transposed(nv, nd, cin, cout, bias, N):
    """ConvTranspose k2 s2 into the upper half of a concat buffer (the engines' use); Cout 64 puts the operator offset (pos * 2 + cob) * chunks to work."""
    tz, ty, tx = tiles(nd, TGRID[nd])
    assert tx == 2 and TGRID[nd][-1] % 16 and TGRID[nd][-2] % (4 if nd == 3 else 16)
    x, w, b = convT_data(nd, N, cin, cout)
    ref = bounded((F.conv_transpose2d if nd == 2 else F.conv_transpose3d)(x, w, bias=b if bias else None, stride=2), 'convT')
    D, H, W = dhw(nd, TGRID[nd])
    ovox = vol(TGRID[nd]) * 2 ** nd

    def run(pl):
        xo, yo = fin(x, pl['x'], 'x'), fout(N, cout * ovox, pl['y'], 'y')
        wpk, _, ops = packed(nv, w, cout, cin, 2 ** nd, 1)
        bo = vec(b, 'bias') if bias else None
        conv_call(nv, nd, xo.t, planar_strides(xo.ss, cin, D, H, W), 0, yo, wpk, bo.t if bias else None, N, TGRID[nd], cin, cout, 0, 1)
        return {'y': yo}, ops + [xo, yo] + ([bo] if bias else [])

    same_value(over_placements(run, [None, {'x': 'gap', 'y': 'upper'}, {'x': 'lower', 'y': 'lower'}])['y'], ref, 'convT y')


@pytest.mark.parametrize('nd,cin', [pytest.param(2, 24, id='2d-cin24_3chunk'), pytest.param(3, 24, id='3d-cin24_3chunk'),
                                    pytest.param(2, 96, id='2d-cin96_12chunk_s2d_of_cout12'), pytest.param(3, 96, id='3d-cin96_12chunk_s2d_of_cout12')])
def test_conv_pointwise(nv, nd, cin):
    """transposed == 2 on its own: the 1 x 1 conv, operator packed with taps = 1 (8 x 12 = the space-to-depth width of a 3-D
    transposed conv's data gradient at Cout 12)."""
    N, cout = 3, 32
    assert cin in (24, 8 * 12) and cin % 8 == 0
    g = gen(300 + cin + nd)
    x, w, b = ints(g, -2, 2, (N, cin) + GRID[nd]), ints(g, -1, 1, (cout, cin)), ints(g, -3, 3, (cout,))
    ref = bounded(torch.einsum('oc,nc...->no...', w, x) + b.view(1, -1, *([1] * nd)), 'pointwise conv')
    D, H, W = dhw(nd, GRID[nd])

    def run(pl):
        xo, yo, bo = fin(x, pl['x'], 'x'), fout(N, cout * D * H * W, pl['y'], 'y'), vec(b, 'bias')
        wpk, _, ops = packed(nv, w, cout, cin, 1, 0)
        conv_call(nv, nd, xo.t, planar_strides(xo.ss, cin, D, H, W), 0, yo, wpk, bo.t, N, GRID[nd], cin, cout, 0, 2)
        return {'y': yo}, ops + [xo, yo, bo]

    same_value(over_placements(run, [None, {'x': 'upper', 'y': 'gap'}, {'x': 'gap', 'y': 'upper'}])['y'], ref, '1x1 conv y')


# ---------------------------------------------------------------------------------------------------------------- packing, read back
DELTA_AT = {3: (1, 2, 5), 2: (3, 5)}          # interior to the first tile: the whole 3^d window stays inside it


def bn_vectors(g, C):
    return torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g), torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.25


def delta_input(nd, grid):
    """[3, 3, *grid]: sample ci holds a single 1.0, in channel ci."""
    x = torch.zeros((3, 3) + grid)
    for ci in range(3):
        x[(ci, ci) + DELTA_AT[nd]] = 1.0
    return x


def delta_conv_expected(nd, wf):
    """What the 3^d conv of delta_input returns for the operator wf [Cout][3][3^d]: y[ci][co][p + 1 - t] = wf[co][ci][t], zero elsewhere."""
    y = torch.zeros((3, wf.shape[0]) + GRID[nd])
    win = tuple(slice(p - 1, p + 2) for p in DELTA_AT[nd])
    for ci in range(3):
        y[(ci, slice(None)) + win] = wf[:, ci].flip(list(range(1, 1 + nd)))
    return y


def delta_convT_expected(nd, wf):
    """... and the transposed conv for wf [3][Cout][2^d]: y[ci][co][2 p + pos] = wf[ci][co][pos]."""
    y = torch.zeros((3, wf.shape[1]) + tuple(2 * s for s in TGRID[nd]))
    win = tuple(slice(2 * p, 2 * p + 2) for p in DELTA_AT[nd])
    for ci in range(3):
        y[(ci, slice(None)) + win] = wf[ci]
    return y


@pytest.mark.parametrize('nd,transposed', [pytest.param(2, 0, id='2d_conv_9taps'), pytest.param(3, 0, id='3d_conv_27taps'),
                                           pytest.param(2, 1, id='2d_transposed_4pos'), pytest.param(3, 1, id='3d_transposed_8pos')])
def test_pack_fold_read_back(nv, nd, transposed):
    """f32_pack_conv_kernel's eval-mode BatchNorm fold on its own: the conv of a delta input returns the folded operator element by
    element (one product by 1.0 and zeros: no rounding), which must have the bits of the fold in separately rounded fp32 operations."""
    N = cin = 3
    cout, eps = 32, 1e-5
    g = gen(400 + nd + transposed)
    grid = TGRID[nd] if transposed else GRID[nd]
    assert all(0 < p < e - 1 for p, e in zip(DELTA_AT[nd], grid)) and all(p + 1 < t for p, t in zip(DELTA_AT[nd], (4, 4, 16) if nd == 3 else (16, 16)))
    w = torch.randn(((cin, cout) + (2,) * nd) if transposed else ((cout, cin) + (3,) * nd), generator=g)
    bn = bn_vectors(g, cout)
    wf, bias_ref = fold_ref(w, bn, eps, transposed)
    ref = (delta_convT_expected if transposed else delta_conv_expected)(nd, wf)
    x = delta_input(nd, grid)
    D, H, W = dhw(nd, grid)
    taps = 2 ** nd if transposed else 3 ** nd

    def run(pl):
        xo, yo = fin(x, pl['x'], 'x'), fout(N, ref[0].numel(), pl['y'], 'y')
        wpk, bo, ops = packed(nv, w, cout, cin, taps, transposed, bn, eps)
        conv_call(nv, nd, xo.t, planar_strides(xo.ss, cin, D, H, W), 0, yo, wpk, None, N, grid, cin, cout, 0, transposed)
        return {'y': yo, 'bias_out': bo}, ops + [xo, yo]

    res = over_placements(run, [None, {'x': 'gap', 'y': 'upper'}])
    same_bits(res['y'], ref, 'folded operator read back')
    same_bits(res['bias_out'], bias_ref, 'folded bias')


@pytest.mark.parametrize('nd', [pytest.param(2, id='2d_ragged-cin12_2chunk_tail4'), pytest.param(3, id='3d_ragged-cin12_2chunk_tail4')])
def test_conv_with_a_power_of_two_fold(nv, nd):
    """A whole ragged conv with the fold on, kept exact: a = gamma / sqrt(var + 0) is a power of two."""
    N, cin, cout = 3, 12, 32
    g = gen(500 + nd)
    x, w, _ = conv_data(nd, N, cin, cout)
    pick = lambda vals: torch.tensor(vals)[torch.randint(0, len(vals), (cout,), generator=g)]
    bn = (pick([0.5, -0.5, 1.0, 2.0]), ints(g, -3, 3, (cout,)), ints(g, -2, 2, (cout,)), pick([0.25, 1.0, 4.0]))
    wf, bias = fold_ref(w, bn, 0.0, 0)
    a = wf.abs().reshape(cout, -1).max(1).values
    assert set(a.tolist()) <= {0.25, 0.5, 1.0, 2.0, 4.0} and len(set(a.tolist())) > 2
    ref = F.relu(conv_nd(nd)(x, wf, bias=bias, padding=1))
    assert float(ref.abs().max()) * 4 < EXACT_BOUND and torch.equal(ref.double(), F.relu(conv_nd(nd)(x.double(), wf.double(), bias=bias.double(), padding=1)))
    D, H, W = dhw(nd, GRID[nd])

    def run(pl):
        xo, yo = fin(x, pl['x'], 'x'), fout(N, cout * D * H * W, pl['y'], 'y')
        wpk, bo, ops = packed(nv, w, cout, cin, 3 ** nd, 0, bn, 0.0)
        conv_call(nv, nd, xo.t, planar_strides(xo.ss, cin, D, H, W), 0, yo, wpk, bo.t, N, GRID[nd], cin, cout, 1, 0)
        return {'y': yo}, ops + [xo, yo]

    same_value(over_placements(run, [None, {'x': 'gap', 'y': 'upper'}])['y'], ref, 'folded conv y')


# ---------------------------------------------------------------------------------------------------------------- max-pool
POOLED = {3: (1, 3, 5), 2: (3, 5)}


def pool_nd(nd):
    return F.max_pool2d if nd == 2 else F.max_pool3d


@functools.lru_cache(maxsize=None)
def pool_data(nd, N, values):
    g = gen(600 + nd + N)
    shape = (N, 3) + tuple(2 * s for s in POOLED[nd])
    if values == 'signed':          # channel 0: negative values only
        z = ints(g, -3, 3, shape)
        z[:, 0] = ints(g, -5, -1, shape[:1] + shape[2:])
    else:                           # {0, 1, 2}: most windows tie
        z = ints(g, 0, 2, shape)
    return z, ints(g, -3, 3, (N, 3) + POOLED[nd]), ints(g, -2, 2, shape)


def tie_share(nd, z):
    """Share of the pooling windows in which the maximum occurs more than once."""
    up = pool_nd(nd)(z, 2)
    for d in range(2, 2 + nd):
        up = up.repeat_interleave(2, d)
    at_max = (F.avg_pool2d if nd == 2 else F.avg_pool3d)((z == up).float(), 2) * 2 ** nd          # occurrences of the maximum per window
    return float((at_max > 1.5).float().mean())


BATCH = [pytest.param(1, id='N1'), pytest.param(3, id='N3')]
POOL_ND = [pytest.param(2, id='2d_pooled3x5'), pytest.param(3, id='3d_pooled1x3x5')]


@pytest.mark.parametrize('N', BATCH)
@pytest.mark.parametrize('nd', POOL_ND)
def test_maxpool_fwd(nv, nd, N):
    """x in each half of a two-slot buffer (the engines pool from `cat`), y at a gap; windows of negative values only in channel 0."""
    z, _, _ = pool_data(nd, N, 'signed')
    assert float(z[:, 0].max()) < 0
    ref = pool_nd(nd)(z, 2)
    Do, Ho, Wo = dhw(nd, POOLED[nd])

    def run(pl):
        xo, yo = fin(z, pl['x'], 'x'), fout(N, ref[0].numel(), pl['y'], 'y')
        nv.call('iunet_f32_maxpool_fwd', nd, nv.ptr(xo.t), xo.ss, nv.ptr(yo.t), yo.ss, 3, N, Do, Ho, Wo, nv.stream())
        return {'y': yo}, [xo, yo]

    same_value(over_placements(run, [None, {'x': 'upper', 'y': 'gap'}, {'x': 'lower', 'y': 'gap'}])['y'], ref, 'max-pool y')


@functools.lru_cache(maxsize=None)
def pool_bwd_ref(nd, N):
    z, dp, _ = pool_data(nd, N, 'ties')
    zr = z.clone().requires_grad_(True)
    pool_nd(nd)(zr, 2).backward(dp)
    return zr.grad


@pytest.mark.parametrize('accumulate', [pytest.param(0, id='overwrite'), pytest.param(1, id='accumulate')])
@pytest.mark.parametrize('N', BATCH)
@pytest.mark.parametrize('nd', POOL_ND)
def test_maxpool_bwd(nv, nd, N, accumulate):
    """The gradient goes to the FIRST maximum of a window in scan order (CPU autograd's choice) under heavy ties; accumulate = 1 adds to
    what dz holds.  z and dz in halves of two-slot buffers."""
    z, dp, dz0 = pool_data(nd, N, 'ties')
    assert tie_share(nd, z) >= 0.5
    ref = pool_bwd_ref(nd, N) + (dz0 if accumulate else 0)
    Do, Ho, Wo = dhw(nd, POOLED[nd])

    def run(pl):
        zo, dpo = fin(z, pl['z'], 'z'), fin(dp, pl['dp'], 'dpool')
        dzo = fio(dz0, pl['dz'], 'dz') if accumulate else fout(N, z[0].numel(), pl['dz'], 'dz')
        nv.call('iunet_f32_maxpool_bwd', nd, nv.ptr(zo.t), zo.ss, nv.ptr(dpo.t), dpo.ss, nv.ptr(dzo.t), dzo.ss, 3, N, Do, Ho, Wo, accumulate, nv.stream())
        return {'dz': dzo}, [zo, dpo, dzo]

    rows = [None, {'z': 'upper', 'dp': 'gap', 'dz': 'lower'}, {'z': 'lower', 'dp': 'tight', 'dz': 'upper'}]
    same_value(over_placements(run, rows)['dz'], ref, 'max-pool dz')


# ---------------------------------------------------------------------------------------------------------------- weight gradient
def wgrad_tiles(nd, N, grid):
    tz, ty, tx = tiles(nd, grid)
    return N * tz * ty * tx


def wgrad_blocks(cin, cout):
    return -(-cin // 16) * -(-cout // 32)


def wgrad_splits(nd, N, grid, cin, cout):
    """iunet_f32_wgrad_splits restated: as many slab rows as 1024 workgroups allow, at most one per voxel tile, at most 256."""
    return min(max(1024 // wgrad_blocks(cin, cout), 1), wgrad_tiles(nd, N, grid), 256)


def wgrad_regime(nd, N, grid, cin, cout):
    t, b = wgrad_tiles(nd, N, grid), 1024 // wgrad_blocks(cin, cout)
    return 'splits_eq_tiles' if t <= min(b, 256) and t < 256 else 'splits_eq_1024_per_blocks' if b < min(t, 256) else 'splits_eq_cap256'


@functools.lru_cache(maxsize=None)
def wgrad_data(nd, N, grid, cin, cout):
    g = gen(700 + nd + cin + cout + N)
    return ints(g, -2, 2, (N, cin) + grid), ints(g, -1, 1, (N, cout) + grid)


@functools.lru_cache(maxsize=None)
def wgrad_ref(nd, N, grid, cin, cout, taps):
    x, dy = wgrad_data(nd, N, grid, cin, cout)
    if taps == 1:
        ref = torch.einsum('no...,nc...->oc', dy.double(), x.double())
    else:
        w = torch.zeros((cout, cin) + (3,) * nd, dtype=torch.float64, requires_grad=True)
        ref = torch.autograd.grad(conv_nd(nd)(x.double(), w, padding=1), w, dy.double())[0]
    return bounded(ref.reshape(cout, cin, taps), 'weight gradient')


CHANNELS = ((1, 32), (12, 40), (40, 3), (64, 64))
WGRAD = [pytest.param(nd, 3, GRID[nd], ci, co, taps, 'splits_eq_tiles', id=f'{nd}d_ragged-taps{taps}-cin{ci}_cout{co}_{wgrad_blocks(ci, co)}blocks-splits_eq_tiles-N3')
         for nd, taps in ((3, 27), (2, 9), (3, 1), (2, 1)) for ci, co in CHANNELS]
WGRAD += [pytest.param(2, 1, GRID[2], 12, 40, 9, 'splits_eq_tiles', id='2d_ragged-taps9-cin12_cout40_2blocks-splits_eq_tiles-N1'),
          # 32 blocks allow 32 rows for 36 tiles: the first four workgroups walk two tiles, the second in another sample
          pytest.param(2, 3, (40, 60), 256, 64, 9, 'splits_eq_1024_per_blocks', id='2d_ragged-taps9-cin256_cout64_32blocks-splits_eq_1024_per_blocks-N3'),
          pytest.param(2, 3, (256, 256), 16, 32, 9, 'splits_eq_cap256', id='2d-taps9-cin16_cout32_1block-splits_eq_cap256_of_768_tiles-N3'),
          pytest.param(3, 4, (16, 16, 64), 16, 32, 27, 'splits_eq_cap256', id='3d-taps27-cin16_cout32_1block-splits_eq_cap256_of_256_tiles-N4')]


@pytest.mark.parametrize('nd,N,grid,cin,cout,taps,regime', WGRAD)
def test_wgrad_and_reduce(nv, nd, N, grid, cin, cout, taps, regime):
    """iunet_f32_wgrad into exactly sized slab scratch, then iunet_reduce_slab; x in the upper half of a concat buffer, dy at a gap."""
    D, H, W = dhw(nd, grid)
    splits = nv.lib().iunet_f32_wgrad_splits(nd, N, D, H, W, cin, cout)
    assert splits == wgrad_splits(nd, N, grid, cin, cout) and wgrad_regime(nd, N, grid, cin, cout) == regime, (splits, regime)
    if regime == 'splits_eq_tiles':
        assert_ragged_two_tiles(nd, grid)
        assert splits == wgrad_tiles(nd, N, grid) < 256
    elif regime == 'splits_eq_1024_per_blocks':
        per = wgrad_tiles(nd, 1, grid)
        assert splits == 1024 // wgrad_blocks(cin, cout) < wgrad_tiles(nd, N, grid) and (0 // per) != ((0 + splits) // per)          # split 0: tiles 0 and `splits`
    else:
        assert splits == 256 <= wgrad_tiles(nd, N, grid)
    x, dy = wgrad_data(nd, N, grid, cin, cout)
    ref = wgrad_ref(nd, N, grid, cin, cout, taps)
    n = cout * cin * taps

    def run(pl):
        xo, dyo, slab, dw = fin(x, pl['x'], 'x'), fin(dy, pl['dy'], 'dy'), scratch(splits * n, 'slab'), scratch(n, 'dW')
        nv.call('iunet_f32_wgrad', nd, nv.ptr(xo.t), xo.ss, nv.ptr(dyo.t), dyo.ss, nv.ptr(slab.t), N, D, H, W, cin, cout, taps, nv.stream())
        nv.call('iunet_reduce_slab', nv.ptr(slab.t), splits, n, nv.ptr(dw.t), 1.0, 0, nv.stream())
        return {'dW': dw}, [xo, dyo, slab, dw]

    rows = [None, {'x': 'upper', 'dy': 'gap'}] + ([{'x': 'gap', 'dy': 'lower'}] if regime == 'splits_eq_tiles' else [])
    same_value(over_placements(run, rows)['dW'], ref, 'dW')


# ---------------------------------------------------------------------------------------------------------------- reduce_slab on its own
def reduce_branch(nparts, n):
    """iunet_reduce_slab's host dispatch restated."""
    return 'tree' if n <= 16384 and nparts > 16 else 'fold' if nparts > 128 else 'plain'


REDUCE = ([('plain', 1, 285), ('plain', 16, 285), ('plain', 40, 16385)] + [('tree', p, n) for n in (3, 4097) for p in (17, 37, 300)] +
          [('fold', p, 16385) for p in (129, 131, 200)])


@pytest.mark.parametrize('alpha,accumulate', [pytest.param(a, c, id=f'alpha{a}-{"accumulate" if c else "overwrite"}') for a, c in ((1.0, 0), (0.5, 0), (1.0, 1), (0.5, 1))])
@pytest.mark.parametrize('branch,nparts,n', [pytest.param(*r, id=f'{r[0]}-nparts{r[1]}-n{r[2]}') for r in REDUCE])
def test_reduce_slab(nv, branch, nparts, n, alpha, accumulate):
    """out = alpha * (sum of the rows) (+ out) on integer slabs.  The fold branch works in place: it may rewrite its first 64 rows and
    nothing beyond nparts * n; the other branches leave the slab as it was."""
    assert reduce_branch(nparts, n) == branch
    if branch == 'tree':
        assert n % 4 and (nparts > 64 + 192) == (nparts == 300)          # the four-row loop runs only at 300
    g = gen(800 + nparts + n)
    slab, out0 = ints(g, -3, 3, (nparts, n)), ints(g, -4, 4, (n,))
    ref = bounded(alpha * slab.sum(0) + (out0 if accumulate else 0), 'reduce')

    slo = fin(slab.reshape(1, -1), TIGHT, 'slab')
    slo.is_input = branch != 'fold'
    oo = fio(out0.reshape(1, -1), TIGHT, 'out') if accumulate else fout(1, n, TIGHT, 'out')
    nv.call('iunet_reduce_slab', nv.ptr(slo.t), nparts, n, nv.ptr(oo.t), alpha, accumulate, nv.stream())
    sync()
    slo.check()
    oo.check()
    same_value(oo.logical(), ref, f'reduce_slab [{branch}]')
    if branch == 'fold':
        verify(torch.equal(slo.logical().reshape(nparts, n)[64:], slab[64:]), 'the fold wrote rows it only reads')


# ---------------------------------------------------------------------------------------------------------------- channel sum
@pytest.mark.parametrize('N', BATCH)
@pytest.mark.parametrize('vox', [pytest.param(285, id='vox285_two_strides_ragged'), pytest.param(7, id='vox7')])
def test_channel_sum(nv, vox, N):
    """t in the upper half of a buffer, as the transposed-conv bias gradient reads it."""
    C = 3
    assert (vox > 256) == (vox == 285) and vox % 256
    t = ints(gen(900 + vox), -3, 3, (N, C, vox))
    ref = bounded(t.sum((0, 2)), 'channel sum')

    def run(pl):
        to, oo = fin(t, pl['t'], 't'), scratch(C, 'out')
        nv.call('iunet_f32_channel_sum', nv.ptr(to.t), to.ss, nv.ptr(oo.t), C, N, vox, nv.stream())
        return {'out': oo}, [to, oo]

    same_value(over_placements(run, [None, {'t': 'upper'}, {'t': 'gap'}])['out'], ref, 'channel sum')


# ---------------------------------------------------------------------------------------------------------------- head
HEAD_GRIDS = {'3x5x19': (3, 5, 19), '1x15x19': (1, 15, 19)}


@functools.lru_cache(maxsize=None)
def head_data(ncls, C0, grid, N):
    g = gen(1001 + 10 * ncls + C0 + 100 * grid[0])
    x, w, b = ints(g, -2, 2, (N, C0) + grid), ints(g, -1, 1, (ncls, C0)), ints(g, -3, 3, (ncls,))
    logits = bounded(torch.einsum('kc,ncdhw->nkdhw', w, x) + b.view(1, -1, 1, 1, 1), 'head logits')
    mx = logits.max(1, keepdim=True).values
    is_max = logits == mx
    first = (is_max & (is_max.int().cumsum(1) == 1)).float().argmax(1)          # exactly one True per voxel: nothing left to the tie rule
    ties = int((is_max.sum(1) > 1).sum())
    return x, w, b, logits, torch.softmax(logits.double(), 1), first.to(torch.uint8), ties


LAYOUTS = ('planar', 'channels_last_padded')
HEAD = [pytest.param(ncls, C0, gk, LAYOUTS[(k + k // 2) % 2], ('logits', 'probs', 'cls'), 3, id=f'ncls{ncls}-C0_{C0}-{gk}-{LAYOUTS[(k + k // 2) % 2]}-all_outputs-N3')
        for k, (ncls, C0, gk) in enumerate((n, c, gk) for n in (2, 3, 10) for c in (32, 5) for gk in HEAD_GRIDS)]
HEAD += [pytest.param(10, 32, '1x15x19', 'planar', ('logits', 'probs', 'cls'), 1, id='ncls10-C0_32-1x15x19-planar-all_outputs-N1')]
HEAD += [pytest.param(3, 32, '3x5x19', 'planar', tuple(o for o in ('logits', 'probs', 'cls') if o != null), 3, id=f'ncls3-C0_32-3x5x19-planar-{null}_null-N3')
         for null in ('logits', 'probs', 'cls')]


def head_call(nv, xo, wo, bo, ncls, C0, outs, strides, divisor, accumulate, N, grid):
    D, H, W = grid
    p = {k: (nv.ptr(outs[k].t) if k in outs else None) for k in ('logits', 'probs', 'cls')}
    nv.call('iunet_f32_head_fwd', nv.ptr(xo.t), xo.ss, C0, nv.ptr(wo.t), nv.ptr(bo.t), ncls, p['logits'], p['probs'], p['cls'],
            nv.ll_array(strides), float(divisor), accumulate, N, D, H, W, nv.stream())


@pytest.mark.parametrize('ncls,C0,gk,layout,wanted,N', HEAD)
def test_head_fwd(nv, ncls, C0, gk, layout, wanted, N):
    """Logits exact on integers, cls the first arg-max (ties present), probabilities against the float64 softmax within 2e-6 x
    max(1, |ref|) (the bar of tests/test_gpu_train_f32.py's pointwise kernels); planar and padded channels-last output strides."""
    grid = HEAD_GRIDS[gk]
    vox = vol(grid)
    x, w, b, logits, probs, cls, ties = head_data(ncls, C0, grid, N)
    assert ties > 0 and vox == 285 and vox > 256 and vox % 256

    def run(pl):
        xo, wo, bo = fin(x, pl['x'], 'x'), vec(w, 'w'), vec(b, 'bias')
        outs = {}
        for k in wanted:
            if k == 'cls':
                outs[k] = fout(N, vox, TIGHT, 'cls', torch.uint8)
            elif layout == 'planar':
                outs[k] = fout(N, ncls * vox, pl['o'], k)
            else:
                outs[k] = StridedOutput((N, ncls) + grid, device=DEVICE, name=k)
        fl = [outs[k] for k in ('logits', 'probs') if k in outs]
        strides = planar_strides(fl[0].ss, ncls, *grid) if layout == 'planar' else fl[0].strides
        assert layout == 'planar' or (strides[1] == 1 and strides[4] > ncls and strides[3] > grid[2] * strides[4])
        head_call(nv, xo, wo, bo, ncls, C0, outs, strides, 1.0, 0, N, grid)
        return outs, [xo, wo, bo] + list(outs.values())

    res = over_placements(run, [None, {'x': 'upper', 'o': 'gap'}, {'x': 'gap', 'o': 'upper'}])
    assert set(res) == set(wanted)
    if 'logits' in res:
        same_value(res['logits'], logits, 'head logits')
    if 'cls' in res:
        same_value(res['cls'], cls, 'class map')
    if 'probs' in res:
        close(res['probs'], probs, 2e-6, 'head probabilities')
        verify(not bool(torch.isnan(res['probs']).any()), 'unwritten probability')


def test_head_fwd_accumulates_then_divides(nv):
    """probs = ((accumulate ? probs : 0) + p) / divisor: with P the bits of a plain run and B what the buffer held, accumulate = 1 and
    divisor = 3 must give the bits of (B + P) / 3 in fp32."""
    ncls, C0, N, grid = 3, 32, 3, HEAD_GRIDS['3x5x19']
    vox = vol(grid)
    x, w, b, logits, probs, _, _ = head_data(ncls, C0, grid, N)
    B = torch.randn(N, ncls * vox, generator=gen(1100))

    def run_with(preset, divisor, accumulate):
        def run(pl):
            xo, wo, bo = fin(x, pl['x'], 'x'), vec(w, 'w'), vec(b, 'bias')
            po = fio(preset, pl['o'], 'probs') if accumulate else fout(N, ncls * vox, pl['o'], 'probs')
            head_call(nv, xo, wo, bo, ncls, C0, {'probs': po}, planar_strides(po.ss, ncls, *grid), divisor, accumulate, N, grid)
            return {'probs': po}, [xo, wo, bo, po]
        return over_placements(run, [None, {'x': 'gap', 'o': 'upper'}])['probs']

    P = run_with(None, 1.0, 0)
    close(P, probs, 2e-6, 'head probabilities')
    got = run_with(B, 3.0, 1)
    same_bits(got, (B + P.reshape(N, -1)) / 3, 'accumulated probabilities')
    verify(not torch.equal(bits(got.reshape(N, -1)), bits(B + P.reshape(N, -1) / 3)), 'the data cannot tell the order of the division apart')


# ---------------------------------------------------------------------------------------------------------------- pointwise: bits
POINT = [pytest.param(285, 3, id='vox285_two_blocks_ragged-N3'), pytest.param(7, 3, id='vox7-N3'), pytest.param(285, 1, id='vox285_two_blocks_ragged-N1')]


@pytest.mark.parametrize('vox,N', POINT)
def test_bn_relu_fwd(nv, vox, N):
    """The kernel's stated contract: the bits of relu(((y - mean) / std) * gamma + beta), every operation rounded on its own."""
    C = 3
    g = gen(1200 + vox)
    y = torch.randn(N, C, vox, generator=g) * 2 + 0.5
    mean, std = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.3
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    v = lambda t: t.view(1, C, 1)
    ref = F.relu(((y - v(mean)) / v(std)) * v(gamma) + v(beta))
    assert 0.1 < float((ref > 0).float().mean()) < 0.9

    def run(pl):
        yo, zo = fin(y, pl['y'], 'y'), fout(N, C * vox, pl['z'], 'z')
        ps = [vec(t, k) for t, k in ((mean, 'mean'), (std, 'std'), (gamma, 'gamma'), (beta, 'beta'))]
        nv.call('iunet_f32_bn_relu_fwd', nv.ptr(yo.t), yo.ss, nv.ptr(zo.t), zo.ss, *[nv.ptr(o.t) for o in ps], C, N, vox, nv.stream())
        return {'z': zo}, [yo, zo] + ps

    same_bits(over_placements(run, [None, {'y': 'upper', 'z': 'gap'}, {'y': 'gap', 'z': 'lower'}])['z'], ref, 'bn_relu_fwd z')


def test_div_f32(nv):
    n, d = 257, 3.0
    x = torch.randn(1, n, generator=gen(1300)) * 100

    def run(pl):
        po = fio(x, pl['p'], 'p')
        nv.call('iunet_div_f32', nv.ptr(po.t), n, d, nv.stream())
        return {'p': po}, [po]

    same_bits(over_placements(run, [None, {'p': 'gap'}])['p'], x / torch.tensor(d), 'p / 3')


@pytest.mark.parametrize('case', ['clean', 'nan_at_last_index', 'inf_at_index_0', 'flag_already_set'])
def test_check_finite(nv, case):
    """n = 1024 x 256 + 1: the grid-stride loop runs twice for exactly one lane, which alone sees the last element."""
    n = 1024 * 256 + 1
    g = torch.randn(1, n, generator=gen(1400))
    if case == 'nan_at_last_index':
        g[0, n - 1] = float('nan')
    if case == 'inf_at_index_0':
        g[0, 0] = float('-inf')
    flag0 = torch.tensor([[1 if case == 'flag_already_set' else 0]], dtype=torch.int32)
    go, fo = fin(g, 'gap', 'g'), fio(flag0.view(F32), TIGHT, 'flag')
    nv.call('iunet_check_finite', nv.ptr(go.t), n, nv.ptr(fo.t), nv.stream())
    sync()
    go.check()
    fo.check()
    verify(int(bits(fo.logical())[0, 0]) == (0 if case == 'clean' else 1), f'flag after {case}')


# ---------------------------------------------------------------------------------------------------------------- BatchNorm: float64
BN_SHAPES = [pytest.param(3, 3, 285, id='C3-N3-vox285_two_strides'), pytest.param(3, 3, 7, id='C3-N3-vox7'), pytest.param(1, 1, 1, id='C1-N1-vox1_M_is_1')]
EPS, MOMENTUM = 1e-5, 0.1


@functools.lru_cache(maxsize=None)
def bn_data(C, N, vox):
    g = gen(1500 + vox)
    y = torch.randn(N, C, vox, generator=g) * (torch.rand(1, C, 1, generator=g) + 0.5) + torch.randn(1, C, 1, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5
    dz = torch.randn(N, C, vox, generator=g)
    yd = y.double()
    mu, var = yd.mean((0, 2)), yd.var((0, 2), unbiased=False)
    return y, gamma, beta, dz, mu, var


def within_one_ulp(got, ref32, what):
    got, ref = got.reshape(-1).double(), ref32.reshape(-1)
    ulp = torch.tensor(np.spacing(ref.abs().numpy().astype(np.float32)).astype(np.float64))
    verify(bool(((got - ref.double()).abs() <= ulp).all()), f'{what}: {got.tolist()} against {ref.tolist()}')


@pytest.mark.parametrize('running', [pytest.param(True, id='running_stats'), pytest.param(False, id='running_null')])
@pytest.mark.parametrize('C,N,vox', BN_SHAPES)
def test_bn_stats(nv, C, N, vox, running):
    """mean and std against the float64 statistics rounded through the kernel's last two fp32 operations (sqrt(float(var) + eps)) within
    one unit in the last place; the running statistics (momentum, UNBIASED variance; factor 1 at M = 1) within 2e-6 x max(1, |ref|),
    the bar tests/test_gpu_train_f32.py holds this update to."""
    y, _, _, _, mu, var = bn_data(C, N, vox)
    M = N * vox
    mean_ref = mu.float()
    std_ref = sqrt_rn(var.float() + torch.tensor(EPS, dtype=F32))
    g = gen(1600)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    rm_ref = (1 - MOMENTUM) * rm0.double() + MOMENTUM * mu
    rv_ref = (1 - MOMENTUM) * rv0.double() + MOMENTUM * var * (M / (M - 1) if M > 1 else 1.0)
    if M == 1:
        assert float(var) == 0.0 and torch.equal(rv_ref, 0.9 * rv0.double())

    def run(pl):
        yo, mo, so = fin(y, pl['y'], 'y'), scratch(C, 'mean'), scratch(C, 'std')
        outs, ops = {'mean': mo, 'std': so}, [yo, mo, so]
        if running:
            outs.update(run_mean=fio(rm0.reshape(1, -1), TIGHT, 'run_mean'), run_var=fio(rv0.reshape(1, -1), TIGHT, 'run_var'))
            ops += [outs['run_mean'], outs['run_var']]
        nv.call('iunet_f32_bn_stats', nv.ptr(yo.t), yo.ss, C, N, vox, EPS, MOMENTUM, nv.ptr(mo.t), nv.ptr(so.t),
                nv.ptr(outs['run_mean'].t) if running else None, nv.ptr(outs['run_var'].t) if running else None, nv.stream())
        return outs, ops

    res = over_placements(run, [None, {'y': 'upper'}, {'y': 'gap'}])
    within_one_ulp(res['mean'], mean_ref, 'mean')
    within_one_ulp(res['std'], std_ref, 'std')
    if running:
        close(res['run_mean'], rm_ref, 2e-6, 'running mean')
        close(res['run_var'], rv_ref, 2e-6, 'running variance')


@functools.lru_cache(maxsize=None)
def bn_bwd_ref(C, N, vox):
    y, gamma, beta, dz, mu, var = bn_data(C, N, vox)
    yr, gr, br = y.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    m, v = yr.mean((0, 2), keepdim=True), yr.var((0, 2), unbiased=False, keepdim=True)          # batch_norm(training=True) written out: F.batch_norm refuses M = 1
    pre = (yr - m) / torch.sqrt(v + EPS) * gr.view(1, C, 1) + br.view(1, C, 1)
    torch.relu(pre).backward(dz.double())
    return pre.detach(), yr.grad, gr.grad, br.grad


@pytest.mark.parametrize('C,N,vox', BN_SHAPES)
def test_bn_relu_bwd(nv, C, N, vox):
    """Against float64 autograd of relu(batch_norm(training = True)) within 5e-6 x max(1, max |ref|) (the bar of
    test_batchnorm_relu_and_pool_backward_kernels).  Elements whose float64 pre-activation lies within 1e-6 of zero may take either
    side of the ReLU: they are left out of the dy comparison (at most 1 % of them, on the reference alone) but must be finite."""
    y, gamma, beta, dz, mu, var = bn_data(C, N, vox)
    pre, dy_ref, dg_ref, db_ref = bn_bwd_ref(C, N, vox)
    keep = (pre.abs() > 1e-6).reshape(-1)
    assert float((~keep).float().mean()) <= 0.01
    mean, std = mu.float(), torch.sqrt(var + EPS).float()

    def run(pl):
        dzo, yo, dyo = fin(dz, pl['dz'], 'dz'), fin(y, pl['y'], 'y'), fout(N, C * vox, pl['dy'], 'dy')
        ps = [vec(t, k) for t, k in ((mean, 'mean'), (std, 'std'), (gamma, 'gamma'), (beta, 'beta'))]
        dgo, dbo = scratch(C, 'dgamma'), scratch(C, 'dbeta')
        nv.call('iunet_f32_bn_relu_bwd', nv.ptr(dzo.t), dzo.ss, nv.ptr(yo.t), yo.ss, nv.ptr(dyo.t), dyo.ss, *[nv.ptr(o.t) for o in ps],
                nv.ptr(dgo.t), nv.ptr(dbo.t), C, N, vox, nv.stream())
        return {'dy': dyo, 'dgamma': dgo, 'dbeta': dbo}, [dzo, yo, dyo, dgo, dbo] + ps

    res = over_placements(run, [None, {'dz': 'upper', 'y': 'gap', 'dy': 'lower'}, {'dz': 'gap', 'y': 'lower', 'dy': 'upper'}])
    dy = res['dy'].reshape(-1)
    verify(bool(torch.isfinite(dy).all()), 'non-finite dy')
    bar = 5e-6 * max(1.0, dy_ref.abs().max().item())
    err = (dy.double() - dy_ref.reshape(-1))[keep].abs().max().item() if bool(keep.any()) else 0.0
    verify(err <= bar, f'dy: max err {err:.3e} over the bar {bar:.3e}')
    close(res['dgamma'], dg_ref, 5e-6, 'dgamma')
    close(res['dbeta'], db_ref, 5e-6, 'dbeta')


# ---------------------------------------------------------------------------------------------------------------- head + loss
HL_VOX, HL_N, HL_C0, HL_ITER = 2048 + 256 + 37, 3, 32, 8


def head_loss_parts(N, vox):
    """iunet_f32_head_loss_num_parts restated: a workgroup takes 8 iterations of 256 voxels of one sample."""
    return N * -(-vox // (256 * HL_ITER))


@functools.lru_cache(maxsize=None)
def head_loss_data(ncls, weighted, t16, seed=1700):
    g = gen(seed + ncls)
    N, C0, vox = HL_N, HL_C0, HL_VOX
    x = torch.randn(N, C0, vox, generator=g)
    w, b = torch.randn(ncls, C0, generator=g) * 0.3, torch.randn(ncls, generator=g) * 0.1
    lab = torch.randint(0, ncls, (N, vox), generator=g)
    y = torch.stack([(lab == c) for c in range(ncls)], 1).float()
    wt = None
    if weighted:
        wt = ((torch.rand(N, 1, vox, generator=g) > 0.3).float() * (0.5 + torch.rand(N, 1, vox, generator=g))).repeat(1, ncls, 1)
        if t16:
            wt = wt.half().float()
        y = y * (wt > 0)
    return x, w, b, y, wt


@functools.lru_cache(maxsize=None)
def head_loss_ref(kind, ncls, weighted, t16):
    x, w, b, y, wt = head_loss_data(ncls, weighted, t16)
    xr, wr, br = [t.double().requires_grad_(True) for t in (x, w, b)]
    logits = torch.einsum('kc,ncv->nkv', wr, xr) + br.view(1, -1, 1)
    logits.retain_grad()
    p = torch.softmax(logits, 1)
    assert float((p.detach() - 0.5).abs().min()) > 1e-6, 'a probability within 1e-6 of 0.5: choose another seed'
    n4 = lambda t: None if t is None else t.detach().numpy().reshape(HL_N, ncls, 1, HL_VOX)
    loss = metrics_ref.loss(kind, n4(p), n4(y), n4(wt), axes=(0, 2, 3))
    p.backward(torch.tensor(metrics_ref.loss_grad(kind, n4(p), n4(y), n4(wt), axes=(0, 2, 3))).reshape(p.shape))
    rounded = metrics_ref.rounded_metrics(n4(p), n4(y), n4(wt), axes=(0, 2, 3))
    return float(loss), [float(r) for r in rounded], logits.grad, xr.grad, wr.grad, br.grad


HEAD_LOSS = [pytest.param(kind, 3, weighted, False, id=f'{kind}-{"weighted" if weighted else "unweighted"}-ncls3-targets_f32-2parts_second_breaks')
             for kind in metrics_ref.KINDS for weighted in (False, True)]
HEAD_LOSS += [pytest.param('mcc_ce', 2, True, True, id='mcc_ce-weighted-ncls2-targets_f16-2parts_second_breaks'),
              pytest.param('dice_ce', 10, True, True, id='dice_ce-weighted-ncls10-targets_f16-2parts_second_breaks')]


@pytest.mark.parametrize('kind,ncls,weighted,t16', HEAD_LOSS)
def test_head_loss(nv, kind, ncls, weighted, t16):
    """iunet_f32_head_loss_fwd / _bwd against the float64 softmax, oracle/metrics_ref.py and autograd: loss within 1e-6 x max(1, |loss|),
    rounded metrics within 2e-5 (test_gpu_train.py's _head_loss_case), dlogits and dx within 5e-6 x max(1, max |ref|).  dlogits is
    written with dl_ss = (ncls + 2) vox: two planes per sample keep the sentinel.  The dlogits then go through iunet_f32_wgrad (taps 1)
    and iunet_f32_channel_sum as train_engine_f32.py sends them: dW and db within 1e-4 of the tensor's maximum, the file's gradient bar."""
    N, C0, vox = HL_N, HL_C0, HL_VOX
    code = metrics_ref.KINDS.index(kind)
    parts = nv.lib().iunet_f32_head_loss_num_parts(N, vox)
    assert parts == head_loss_parts(N, vox) == 2 * N and 0 < vox - 2048 < 2048 and (vox - 2048) % 256          # the second part ends inside an iteration
    x, w, b, y, wt = head_loss_data(ncls, weighted, t16)
    loss_ref, rounded_ref, dl_ref, dx_ref, dw_ref, db_ref = head_loss_ref(kind, ncls, weighted, t16)
    tdt = torch.float16 if t16 else F32
    W = vox          # the head's weight gradient sees the voxels as one row
    splits = nv.lib().iunet_f32_wgrad_splits(2, N, 1, 1, W, C0, ncls)
    assert splits == wgrad_splits(2, N, (1, W), C0, ncls) == 256

    def run(pl):
        xo, wo, bo = fin(x, pl['x'], 'x'), vec(w, 'w'), vec(b, 'bias')
        yo = vec(y, 'target', tdt)
        wto = vec(wt, 'weight', tdt) if weighted else None
        slab, out4, coef = scratch(parts * ncls * 8, 'loss slab'), scratch(4, 'out4'), scratch(ncls * 3, 'coef')
        dlo, dxo = fout(N, (ncls + 2) * vox, TIGHT, 'dlogits'), fout(N, C0 * vox, pl['dx'], 'dx')
        dlo.partial = True
        wslab, dwo, dbo = scratch(splits * ncls * C0, 'dW slab'), scratch(ncls * C0, 'dW'), scratch(ncls, 'db')
        s = nv.stream()
        nv.call('iunet_f32_head_loss_fwd', nv.ptr(xo.t), xo.ss, C0, nv.ptr(wo.t), nv.ptr(bo.t), ncls, nv.ptr(yo.t), nv.ptr(wto.t) if weighted else None,
                int(t16), code, nv.ptr(slab.t), nv.ptr(out4.t), nv.ptr(coef.t), N, vox, s)
        nv.call('iunet_f32_head_loss_bwd', nv.ptr(xo.t), xo.ss, C0, nv.ptr(wo.t), nv.ptr(bo.t), ncls, nv.ptr(yo.t), nv.ptr(wto.t) if weighted else None,
                int(t16), nv.ptr(coef.t), nv.ptr(dlo.t), dlo.ss, nv.ptr(dxo.t), dxo.ss, N, vox, s)
        nv.call('iunet_f32_wgrad', 2, nv.ptr(xo.t), xo.ss, nv.ptr(dlo.t), dlo.ss, nv.ptr(wslab.t), N, 1, 1, W, C0, ncls, 1, s)
        nv.call('iunet_reduce_slab', nv.ptr(wslab.t), splits, ncls * C0, nv.ptr(dwo.t), 1.0, 0, s)
        nv.call('iunet_f32_channel_sum', nv.ptr(dlo.t), dlo.ss, nv.ptr(dbo.t), ncls, N, vox, s)
        return ({'out4': out4, 'dlogits': dlo, 'dx': dxo, 'dW': dwo, 'db': dbo},
                [xo, wo, bo, yo, slab, out4, coef, dlo, dxo, wslab, dwo, dbo] + ([wto] if weighted else []))

    res = over_placements(run, [None, {'x': 'gap', 'dx': 'upper'}, {'x': 'upper', 'dx': 'gap'}])
    out4 = res['out4'].reshape(-1).double()
    verify(abs(out4[0].item() - loss_ref) <= 1e-6 * max(1.0, abs(loss_ref)), f'loss {out4[0].item()!r} against {loss_ref!r}')
    verify(bool(np.allclose(out4[1:].numpy(), rounded_ref, atol=2e-5, rtol=0)), f'rounded metrics {out4[1:].tolist()} against {rounded_ref}')
    dl = res['dlogits'].reshape(N, ncls + 2, vox)
    verify(bool((bits(dl[:, ncls:]) == SENTINEL[F32]).all()) and not bool(torch.isnan(dl[:, :ncls]).any()), 'dlogits: the planes past ncls were written, or one of the first ncls was not')
    close(dl[:, :ncls], dl_ref, 5e-6, 'dlogits')
    close(res['dx'], dx_ref, 5e-6, 'dx')
    for k, ref in (('dW', dw_ref), ('db', db_ref)):
        err = (res[k].reshape(-1).double() - ref.reshape(-1)).abs().max().item()
        verify(err <= 1e-4 * ref.abs().max().item(), f'head {k}: max err {err:.3e} against 1e-4 x {ref.abs().max().item():.3e}')
