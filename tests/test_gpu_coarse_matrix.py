"""The coarse-logit kernels of csrc/deeplab.hip that DeepLabV3, Segformer and UPerNet train through (CoarseTrainEngine), through the C ABI:
iunet_dl_up_loss_fwd / _bwd, iunet_dl_head_bwd, iunet_dl_dropout and the pooling branch (iunet_dl_pool_gemv / _psb / _bwd).

Conventions of tests/test_gpu_kernel_matrix.py: every device operand sits in a sentinel-filled allocation of tests/arena.py, outputs and
scratch start as the NaN sentinel, after each call every operand's bands and every input's bits are checked, and where an entry point
takes sample strides every further placement row must give the bits of the all-tight one.

  1. upsample + softmax + loss, forward and backward: float64 throughout (F.interpolate align_corners=True, oracle/metrics_ref.py, autograd),
     at more than one workgroup row per sample, ragged and exactly full rows, ncls 2..10, f16 and f32 targets, with and without a weight,
     coarse extents of 1 and the scale factors 1 and 64.  In 2-D the adjoint is also checked on its own: the fine gradient the kernel left in
     `dfine`, pushed through the exact float64 transpose of the interpolation matrix, against `dcoarse` element by element at a bound derived
     from the fp32 evaluation of the source coordinate and the length of the sums (axis_bound, adjoint_tolerance) -- a tap of weight 0.01 that
     the gather's window missed fails it.
  2. head backward: small-integer data on which dx, dW and db are exact in fp32 in any summation order: bit for bit.
  3. dropout: powers of two and multiples of 1/4, the header's formula restated in fp32 torch: bit for bit, mask asymmetric in (n, c, v).
  4. pooling branch: float64 autograd at the gates of test_gpu_deeplabv3.py, at sizes where every kernel takes more than one workgroup; the
     eval form (fold from the running statistics) also bit for bit against the training form given tests/arena.py: fold_ref's scale and shift
     (the fold contract of tests/test_gpu_fold_contract.py promises bn_fold_scale / bn_fold_bias bit for bit).

The tables, the references and the conditions that make the comparisons legitimate are checked without a GPU by tests/test_coarse_matrix_cpu.py.
Needs an MI355X: run with -m gpu."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import metrics_ref
from tests.arena import BAND, SENTINEL, Operand, bits, fold_ref, scratch
from tests.test_gpu_kernel_matrix import DT, F32, assert_exact16, dev32, gen, ints, nv, out, over_placements, put  # noqa: F401 (nv: fixture)
from tests.test_gpu_kernels import blocked, unblocked  # noqa: F401 (blocked: through put)

pytestmark = pytest.mark.gpu

LOSS_CODE = {'ce': 0, 'dice': 1, 'iou': 2, 'mcc': 3, 'dice_ce': 4, 'iou_ce': 5, 'mcc_ce': 6}          # train_engine.LOSS_KINDS
UPL_PER = 8 * 256          # fine voxels per workgroup (= slab row) of iunet_dl_up_loss_fwd
HB_PER = 2048              # voxels per workgroup of iunet_dl_head_bwd's weight gradient
LSCALE = 4.0
MARGIN = 1e-3              # no probability of the float64 reference within this of 0.5: the rounded metrics are discontinuous there
DECIDED, SEEDS = 0.05, 96
U = 2.0 ** -24            # the unit roundoff of fp32


def parts(N, vox, per):
    return N * -(-vox // per)


def fine_of(nd, coarse, s):
    return tuple(c * s for c in coarse)


def vox_of(sp):
    return int(np.prod(sp))


# ---------------------------------------------------------------------------------------------------------------- 1. upsample + loss
# (nd, coarse grid, s, ncls, N); rows per sample = ceil(fine voxels / 2048)
#   2-D 6 x 7 x8      2688 voxels: two rows per sample, the second ends 2.5 chunks of 256 in; ncls 10 is the `default:` arm of DL_NCLS_SWITCH
#   2-D 3 x 5 x16     3840
#   2-D 1 x 9 x8      576: one axis with a coarse extent of 1 (the adjoint's window is the whole axis)
#   2-D 40 x 59 x1    2360: identity weights; ragged against 256 and 2048
#   2-D 1 x 1 x64     4096: the upper bound of dl_up_check, a coarse extent of 1 on both axes, exactly two full rows
#   2-D 3 x 7 x3      189: only the width pair (Ec, s) = (3, 3) is dyadic ((Ef - 1) / (Ec - 1) = 4): its fp32 weights are exact
#   3-D 3 x 3 x 5 x4  2880: two rows, the second ragged;  3-D 1 x 2 x 3 x8  3072: Dc = 1;  3-D 2 x 2 x 2 x8, N 1  16^3 = 4096: exactly two full rows
#   (2 x 2 x 2 x16 would be 32^3 = 32768 voxels, sixteen rows: the two full rows take the factor 8; the factor 16 is in the 2-D 3 x 5 row)
LOSS_TABLE = [(2, (6, 7), 8, 2, 3), (2, (6, 7), 8, 10, 3), (2, (3, 5), 16, 3, 3), (2, (1, 9), 8, 4, 3), (2, (40, 59), 1, 3, 3),
              (2, (1, 1), 64, 2, 3), (2, (3, 7), 3, 5, 3),
              (3, (3, 3, 5), 4, 2, 3), (3, (3, 3, 5), 4, 7, 3), (3, (1, 2, 3), 8, 3, 3), (3, (2, 2, 2), 8, 10, 1)]
TWO_ROW = {(2, (6, 7), 8), (3, (3, 3, 5), 4)}          # these keep dice_ce, the flagship loss's form
DYADIC = (3, 3)                                        # (Ec, s) of the 3 x 7 x3 row's width
CROSS = [('f32', False), ('f32', True), ('f16', False), ('f16', True)]          # (target dtype, weighted)
TDTYPE = {'f32': (0, torch.float32), 'f16': (1, torch.float16)}


def _loss_cases():
    """The table crossed with (tdtype, weight); one loss kind per case, rotating through all seven per dimension."""
    cases, turn = [], {2: 0, 3: 0}
    for nd, coarse, s, ncls, N in LOSS_TABLE:
        for td, weighted in CROSS:
            if (nd, coarse, s) in TWO_ROW:
                kind = 'dice_ce'
            else:
                kind = metrics_ref.KINDS[turn[nd] % 7]
                turn[nd] += 1
            cases.append((nd, coarse, s, ncls, N, td, weighted, kind))
    return cases


LOSS_CASES = _loss_cases()


def interp_matrix(Ec, Ef):
    """The align_corners=True linear interpolation of one axis as a float64 matrix [Ef][Ec]: fine o reads i0 = floor(src), i1 = min(i0 + 1,
    Ec - 1) with weights (1 - f, f), src = o (Ec - 1) / (Ef - 1)."""
    A = np.zeros((Ef, Ec))
    for o in range(Ef):
        src = o * (Ec - 1) / (Ef - 1) if Ef > 1 else 0.0
        i0 = min(int(np.floor(src)), Ec - 1)
        i1 = min(i0 + 1, Ec - 1)
        f = src - i0
        A[o, i0] += 1.0 - f
        A[o, i1] += f
    return A


def adjoint2d(b, Hc, Wc):
    """The exact adjoint of the 2-D upsampling: b [..., Hf, Wf] float64 -> [..., Hc, Wc], A_h^T b A_w."""
    Ah, Aw = interp_matrix(Hc, b.shape[-2]), interp_matrix(Wc, b.shape[-1])
    return np.einsum('hi,...hw,wj->...ij', Ah, b, Aw)


def src_delta(Ec, Ef):
    """The largest difference between resample_axis_corners's fp32 source coordinate sc * o, sc = fp32((Ec - 1) / (Ef - 1)), and the exact one."""
    if Ef <= 1 or Ec <= 1:
        return 0.0
    sc = np.float32(Ec - 1) / np.float32(Ef - 1)
    o = np.arange(Ef)
    src32 = (sc * o.astype(np.float32)).astype(np.float32)
    return float(np.abs(src32.astype(np.float64) - o * (Ec - 1) / (Ef - 1)).max())


def lerp_weights_f32(Ec, Ef):
    """resample_axis_corners in numpy float32: (i0, f) per fine index."""
    sc = np.float32(Ec - 1) / np.float32(Ef - 1) if Ef > 1 else np.float32(0)
    src = (sc * np.arange(Ef).astype(np.float32)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int32), Ec - 1)
    return i0, (src - i0.astype(np.float32)).astype(np.float32)


def axis_bound(Ec, Ef):
    """B [Ef][Ec] with |out_i - sum_o w_o in_o| <= sum_o B[o][i] |in_o| for one axis pass of dl_up_adjoint_kernel, which computes out_i as a
    chain of K fp32 fused multiply-adds over the fine indices o whose fp32 weight for i is not zero:
      * the fp32 weight differs from the exact w_o by at most delta + 2^-24: delta = src_delta (the weights are (1 - f, f), f = src - i0, the
        subtraction exact, `1 - f` one rounding) -- an ABSOLUTE error, whatever the size of w_o, and it can make a weight of exactly 0 a
        nonzero one: the fine indices within delta of the support of column i, taken here as the support widened by one index either way;
      * the chain adds at most (K + 1) 2^-24 |w_o| |in_o| per term (K: the longest column's support, two more for the widened one).
    Nothing here comes from a GPU run.  A tap of weight 0.01 that the window missed changes out_i by 0.01 |in_o|, four orders above its
    delta |in_o| <= 1e-6 |in_o| here.  (The shorter form (delta + (K + 1) 2^-24) sum |w_o| |in_o| is no bound: it scales the absolute weight
    error by |w_o|.  The emulated fp32 weights alone, summed in float64, exceed it on the 3 x 5 x16 row -- 1.08 of it -- and a weight of
    exactly 0 that fp32 makes 5e-7 beside a gradient orders above its neighbours' exceeds it without limit.)"""
    A = interp_matrix(Ec, Ef)
    near = A != 0
    near[1:] |= A[:-1] != 0
    near[:-1] |= A[1:] != 0
    K = int((A != 0).sum(0).max()) + 2
    return (src_delta(Ec, Ef) + U) * near + (K + 1) * U * A


def adjoint_tolerance(g, Hc, Wc):
    """The bound on |dcoarse - exact adjoint of the fp32 fine gradient g [..., Hf, Wf]|, element by element: the W pass errs by at most
    E1 = B_w^T |g| (axis_bound), which the H pass carries through its own weights, and the H pass adds B_h^T |tmp|, |tmp| <= A_w^T |g| + E1:
    tol = A_h^T E1 + B_h^T A_w^T |g|, times 1.01 for the second-order terms (E1 inside |tmp|, the fp32 weights inside the carried error),
    plus the underflow floor: all of the above is relative, and fp32 has no relative precision below its smallest normal number 2^-126
    (subnormal operands and results may be flushed): at most 2^-126 per operation, K_w of them carried through K_h weights <= 1 and K_h
    more.  It matters where a saturated softmax leaves a whole window of fine gradients subnormal, and nowhere else (1e-35)."""
    Hf, Wf = g.shape[-2:]
    Ah, Aw, Bh, Bw = interp_matrix(Hc, Hf), interp_matrix(Wc, Wf), axis_bound(Hc, Hf), axis_bound(Wc, Wf)
    Kh, Kw = int((Ah != 0).sum(0).max()) + 2, int((Aw != 0).sum(0).max()) + 2
    two = lambda L, R: np.einsum('hi,...hw,wj->...ij', L, np.abs(g), R)          # noqa: E731
    return 1.01 * (two(Ah, Bw) + two(Bh, Aw)) + (Kh * Kw + Kh) * 2.0 ** -126


def interp_matrix_f32(Ec, Ef):
    """The matrix of the weights resample_axis_corners computes in fp32 (lerp_weights_f32), as float64 values."""
    i0, f = lerp_weights_f32(Ec, Ef)
    A = np.zeros((Ef, Ec))
    for o in range(Ef):
        A[o, i0[o]] += float(np.float32(1) - f[o])
        A[o, min(i0[o] + 1, Ec - 1)] += float(f[o])
    return A


def check_adjoint_bound(g, Hc, Wc):
    """adjoint_tolerance against what it must cover, without a GPU: the adjoint through the emulated fp32 weights (interp_matrix_f32) against
    the exact one, both summed in float64, on a fine gradient g.  -> the worst share of the bound the weights' error takes"""
    Hf, Wf = g.shape[-2:]
    got = np.einsum('hi,...hw,wj->...ij', interp_matrix_f32(Hc, Hf), g, interp_matrix_f32(Wc, Wf))
    tol = adjoint_tolerance(g, Hc, Wc)
    share = float(np.max(np.abs(got - adjoint2d(g, Hc, Wc)) / np.maximum(tol, 1e-300)))
    assert share <= 1.0, f'the fp32 weights alone take {share:.2f} of the adjoint bound'
    return share


def worst_axis_factor(Ec, Ef):
    """The largest entry of axis_bound relative to a weight of 1: how small a missed tap the isolated check still sees."""
    return float(axis_bound(Ec, Ef).max())


def upsample64(lc, nd, s):
    return F.interpolate(lc.double(), scale_factor=s, mode='trilinear' if nd == 3 else 'bilinear', align_corners=True)


@functools.lru_cache(maxsize=None)
def loss_logits(nd, coarse, s, ncls, N):
    """The coarse fp32 logits of a table row: drawn, and scaled where needed, until no probability of the float64 reference lies within MARGIN
    of 0.5 (a probability there could round to the other side in fp32 and move the rounded metrics by a whole voxel's weight) and at least
    DECIDED of the fine voxels have a probability above 0.5 (else the rounded metrics see no prediction at all).  A sharper softmax has fewer
    fine voxels near 0.5 and more decided ones: per scale factor SEEDS draws are tried, then the factor grows by a half.
    -> lc, factor, margin, share of decided voxels"""
    for factor in [1.5 ** k for k in range(16)]:
        for k in range(SEEDS):
            lc = (torch.randn((N, ncls) + coarse, generator=gen(5000 + 1000 * nd + SEEDS * ncls + k)) * factor).float()
            p = torch.softmax(upsample64(lc, nd, s), 1)
            margin, decided = (p - 0.5).abs().min().item(), (p.max(1).values > 0.5).float().mean().item()
            if margin >= 2 * MARGIN and decided >= DECIDED:          # drawn with twice the margin asserted
                return lc, factor, margin, decided
    raise AssertionError(f'no logits with the margin for {(nd, coarse, s, ncls, N)}')


@functools.lru_cache(maxsize=None)
def loss_data(nd, coarse, s, ncls, N, td, weighted):
    """target, weight (or None) as fp32 tensors holding values of the target dtype (fp16 targets and weights are generated already rounded,
    so both sides read the same numbers): a one-hot target, zero where the weight is; weight = 0/1 mask x a factor in [0.5, 1.5)."""
    fine = fine_of(nd, coarse, s)
    g = gen(5500 + 10 * nd + ncls + (100 if weighted else 0))
    lab = torch.randint(0, ncls, (N,) + fine, generator=g)
    y = F.one_hot(lab, ncls).movedim(-1, 1).float().contiguous()
    wt = None
    if weighted:
        wt = (torch.rand((N, 1) + fine, generator=g) > 0.3).float() * (0.5 + torch.rand((N, 1) + fine, generator=g))
        wt = wt.to(TDTYPE[td][1]).float().expand(N, ncls, *fine).contiguous()
        y = y * (wt > 0)
    return y, wt


@functools.lru_cache(maxsize=None)
def loss_reference(nd, coarse, s, ncls, N, td, weighted, kind):
    """float64: probabilities, loss, rounded metrics, the fine logit gradient and the coarse one (autograd), unscaled."""
    lc = loss_logits(nd, coarse, s, ncls, N)[0]
    y, wt = loss_data(nd, coarse, s, ncls, N, td, weighted)
    axes = (0,) + tuple(range(2, 2 + nd))
    lcr = lc.double().requires_grad_(True)
    fine = upsample64(lcr, nd, s)
    fine.retain_grad()
    probs = torch.softmax(fine, 1)
    p, yn, wn = probs.detach().numpy(), y.numpy(), None if wt is None else wt.numpy()
    lv = metrics_ref.loss(kind, p, yn, wn, axes=axes)
    probs.backward(torch.tensor(metrics_ref.loss_grad(kind, p, yn, wn, axes=axes)))
    return dict(probs=probs.detach(), loss=lv, rounded=metrics_ref.rounded_metrics(p, yn, wn, axes=axes), dfine=fine.grad.clone(), dcoarse=lcr.grad.clone())


def wide(t, dtype, name):
    """A target / weight / mask operand whose bands are as long as the operand itself (at least arena.BAND): a load that reads it as a wider
    type, or through a transposed index, stays inside the allocation and shows in the result instead."""
    t = t.reshape(-1)
    return Operand(1, t.numel(), dtype, 'tight', t, name=name, band=max(BAND, t.numel()))


def up_loss_run(nv, case):
    nd, coarse, s, ncls, N, td, weighted, kind = case
    lc = loss_logits(nd, coarse, s, ncls, N)[0]
    y, wt = loss_data(nd, coarse, s, ncls, N, td, weighted)
    code, tt = TDTYPE[td]
    Dc, Hc, Wc = coarse if nd == 3 else (1,) + coarse
    Df, Hf, Wf = (Dc * s if nd == 3 else 1), Hc * s, Wc * s
    vox = Df * Hf * Wf
    np_ = nv.lib().iunet_dl_up_loss_num_parts(N, vox)
    assert np_ == parts(N, vox, UPL_PER)
    lco, yo = dev32(lc, 'lc'), wide(y, tt, 'target')
    wo = wide(wt, tt, 'weight') if weighted else None
    slab, out4, coef = scratch(np_ * ncls * 8, name='slab'), scratch(4, name='out4'), scratch(ncls * 3, name='coef')
    ls = dev32(torch.tensor([LSCALE]), 'lscale')
    dfine, tmp = scratch(N * ncls * vox, name='dfine'), scratch(N * ncls * Df * Hf * Wc, name='tmp')
    dco = scratch(lc.numel(), name='dcoarse')
    wp = None if wo is None else nv.ptr(wo.t)
    nv.call('iunet_dl_up_loss_fwd', nd, nv.ptr(lco.t), ncls, Dc, Hc, Wc, s, nv.ptr(yo.t), wp, code, LOSS_CODE[kind], nv.ptr(slab.t),
            nv.ptr(out4.t), nv.ptr(coef.t), N, nv.stream())
    nv.call('iunet_dl_up_loss_bwd', nd, nv.ptr(lco.t), ncls, Dc, Hc, Wc, s, nv.ptr(yo.t), wp, code, nv.ptr(coef.t), nv.ptr(ls.t),
            nv.ptr(dfine.t), nv.ptr(tmp.t), nv.ptr(dco.t), N, nv.stream())
    torch.cuda.synchronize()
    for o in [lco, yo, slab, out4, coef, ls, dfine, tmp, dco] + ([wo] if wo is not None else []):
        o.check()          # bands of slab, out4, coef, dfine, tmp, dcoarse intact; lc, target, weight, lscale unchanged bit for bit
    return {k: o.logical().reshape(-1) for k, o in (('out4', out4), ('coef', coef), ('dcoarse', dco), ('dfine', dfine), ('slab', slab))}


@pytest.mark.parametrize('nd,coarse,s,ncls,N,td,weighted,kind', LOSS_CASES)
def test_up_loss(nv, nd, coarse, s, ncls, N, td, weighted, kind):
    case = (nd, coarse, s, ncls, N, td, weighted, kind)
    ref = loss_reference(*case)
    a, b = up_loss_run(nv, case), up_loss_run(nv, case)
    for k in ('out4', 'coef', 'dcoarse'):
        assert torch.equal(bits(a[k]), bits(b[k])), f'{k}: two calls on fresh buffers differ'
    assert bool(torch.isfinite(a['slab']).all()), 'a slab row was left unwritten'
    lv, got4 = ref['loss'], a['out4'].double()
    r = np.array(ref['rounded'])
    dco = a['dcoarse'].double().reshape(ref['dcoarse'].shape) / LSCALE
    gate = 1e-4 * max(1e-3, ref['dcoarse'].abs().max().item()) + 1e-7
    print(f'loss {got4[0].item():.7f} vs {lv:.7f}; rounded metrics max diff {np.abs(got4[1:].numpy() - r).max():.2e}; '
          f'dcoarse max err {(dco - ref["dcoarse"]).abs().max().item():.2e} (gate {gate:.2e})')
    assert abs(got4[0].item() - lv) <= 1e-4 * max(1.0, abs(lv)), (got4[0].item(), lv)
    assert np.abs(got4[1:].numpy() - r).max() <= 2e-5, (got4[1:], r)
    assert (dco - ref['dcoarse']).abs().max().item() <= gate
    fine = fine_of(nd, coarse, s)
    dfine = a['dfine'].double().reshape((N, ncls) + fine) / LSCALE
    fgate = 1e-4 * max(1e-3, ref['dfine'].abs().max().item()) + 1e-7
    if nd == 2:
        assert (dfine - ref['dfine']).abs().max().item() <= fgate          # `dfine` still holds the fine gradient
        g32 = a['dfine'].reshape((N, ncls) + fine).double().numpy()        # the kernel's own fp32 fine gradient, scaled
        want = adjoint2d(g32, *coarse)
        tol = adjoint_tolerance(g32, *coarse)
        err = np.abs(a['dcoarse'].double().numpy().reshape(want.shape) - want)
        print(f'adjoint alone: worst err / tol {np.max(err / np.maximum(tol, 1e-300)):.3f}')
        assert bool((err <= tol).all()), f'adjoint: {int((err > tol).sum())} coarse elements off, worst err / tol {np.max(err / np.maximum(tol, 1e-300)):.2f}'
    else:
        # the H pass of the adjoint wrote its output over the first N ncls Df Hc Wc floats of `dfine`; the rest is the fine gradient still
        used = N * ncls * fine[0] * coarse[1] * coarse[2]
        rest = (dfine - ref['dfine']).abs().reshape(-1)[used:]
        assert rest.numel() > 0 and rest.max().item() <= fgate


# ---------------------------------------------------------------------------------------------------------------- 2. head backward
# (C, ncls, N, coarse grid): 740 voxels = one row of DL_HB_PER, ragged against 256; 2360 = two rows, the second ragged; C 8 = one plane + the
# bias plane; C 256 = 33 planes: (planes + 1) x 80 = 2720 outputs, the reduce kernel over more than one workgroup
HB_CASES = [(32, 2, 3, (20, 37)), (64, 10, 1, (40, 59)), (8, 3, 3, (3, 10, 13)), (256, 5, 2, (9, 11))]
STRIDE_ROWS = lambda a, b: [None, {a: 'gap', b: 'gap'}, {a: 'upper', b: 'lower'}]          # noqa: E731


@functools.lru_cache(maxsize=None)
def head_bwd_data(C, ncls, N, sp):
    """dl integers in -3..3, w multiples of 1/8 in [-1, 1], x integers in -4..4: dx is a multiple of 1/8 below 32 (exact in fp32, f16 and
    bf16), every partial sum of dW and db an integer below 2^24 in any order.  -> dl, w, x, dx, dW, db (float64 references)"""
    g = gen(6000 + C + ncls)
    vox = vox_of(sp)
    dl = ints(g, -3, 3, (N, ncls, vox))
    w = ints(g, -8, 8, (ncls, C)) / 8
    x = ints(g, -4, 4, (N, C) + tuple(sp))
    dx = torch.einsum('nkv,kc->ncv', dl.double(), w.double()).reshape((N, C) + tuple(sp))
    dW = torch.einsum('nkv,ncv->kc', dl.double(), x.double().reshape(N, C, vox))
    db = dl.double().sum((0, 2))
    return dl, w, x, dx, dW, db


def check_head_bwd_exact(C, ncls, N, sp):
    """The conditions of the bit-for-bit comparison, on the reference alone."""
    dl, w, x, dx, dW, db = head_bwd_data(C, ncls, N, sp)
    vox = vox_of(sp)
    assert torch.einsum('nkv,ncv->kc', dl.abs().double(), x.abs().double().reshape(N, C, vox)).max().item() < 2 ** 24          # sum |dl x| per output
    assert dl.abs().sum((0, 2)).max().item() < 2 ** 24
    assert torch.equal(dx * 8, (dx * 8).round()) and torch.einsum('nkv,kc->ncv', dl.abs().double(), w.abs().double()).max().item() < 32
    for T in DT.values():
        assert torch.equal(dx.float().to(T).double(), dx) and torch.equal(x.to(T).float(), x)          # representable: one rounding changes nothing
    assert (dx.abs() > 256).float().mean().item() <= 0.02          # assert_exact16's cap, far from it
    assert dW.abs().max().item() > 0 and bool((db != 0).any())


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('C,ncls,N,sp', HB_CASES)
def test_head_bwd(nv, dt, C, ncls, N, sp):
    dtype = DT[dt]
    dl, w, x, dx_ref, dW_ref, db_ref = head_bwd_data(C, ncls, N, sp)
    vox = vox_of(sp)
    np_ = nv.lib().iunet_dl_head_bwd_parts(N, vox)
    assert np_ == parts(N, vox, HB_PER)
    code = nv.DTYPE_CODE[dtype]

    def run(pl):
        xo, wo, dlo = put(x, dtype, pl['x'], 'x'), dev32(w, 'w'), dev32(dl, 'dl')
        dxo = out(N, C, vox, dtype, pl['dx'], 'dx')
        slab = scratch(np_ * (C // 8 + 1) * 80, name='slab')
        dW, db = scratch(ncls * C, name='dW'), scratch(ncls, name='db')          # sentinel first: every output written, nothing beyond
        nv.call('iunet_dl_head_bwd', code, nv.ptr(xo.t), xo.ss, C, nv.ptr(wo.t), nv.ptr(dlo.t), ncls, nv.ptr(dxo.t), dxo.ss, nv.ptr(slab.t),
                nv.ptr(dW.t), nv.ptr(db.t), N, vox, nv.stream())
        return {'dx': dxo, 'dW': dW, 'db': db}, [xo, wo, dlo, dxo, slab, dW, db]

    res = over_placements(nv, run, STRIDE_ROWS('x', 'dx'))
    assert torch.equal(res['dW'].logical().reshape(ncls, C).double(), dW_ref), 'dW'
    assert torch.equal(res['db'].logical().reshape(-1).double(), db_ref), 'db'
    got = unblocked(res['dx'].logical().float().reshape(-1), N, C, tuple(sp))
    assert_exact16(got, dx_ref, dtype, 'head dx')


# ---------------------------------------------------------------------------------------------------------------- 3. dropout
DROP_SHAPES = [(8, 3, 390), (72, 3, 5 * 7 * 9), (256, 1, 300)]          # (C, N, vox): vox never a multiple of 256
DROP_P = [0.5, 0.1]          # keep = 1 / (1 - p): 2 exactly; inexact, where the one rounding to T matters


@functools.lru_cache(maxsize=None)
def dropout_data(C, N, vox, p):
    """scale a power of two per channel, shift multiples of 1/4, y integers in -8..8; the mask random at rate p per (n, c, v)."""
    g = gen(7000 + C + int(100 * p))
    scale = 2.0 ** torch.randint(-1, 2, (C,), generator=g).float()
    shift = ints(g, -8, 8, (C,)) / 4
    y = ints(g, -8, 8, (N, C, vox))
    mask = (torch.rand((N, C, vox), generator=g) >= p).to(torch.uint8)
    return scale, shift, y, mask


def keep_of(p):
    """1.f / (1.f - p) as the host computes it: p as fp32, two correctly rounded fp32 operations."""
    one = torch.tensor(1.0, dtype=F32)
    return one / (one - torch.tensor(p, dtype=F32))


def dropout_ref(C, N, vox, p, mode, masked, dtype):
    """include/iunet.h restated in fp32 torch.  mode 0: out = T(T(relu(scale y + shift)) * keep); mode 1: out = T(y * keep); keep = mask / (1 - p),
    1 without a mask: one fp32 multiply and one rounding to T."""
    scale, shift, y, mask = dropout_data(C, N, vox, p)
    z = y if mode == 1 else torch.relu(scale.view(1, -1, 1) * y + shift.view(1, -1, 1)).to(dtype).float()
    if masked:
        z = torch.where(mask.bool(), z * keep_of(p), torch.zeros_like(z))
    return z.to(dtype)


def check_dropout_exact(C, N, vox, p):
    scale, shift, y, mask = dropout_data(C, N, vox, p)
    t = scale.double().view(1, -1, 1) * y.double() + shift.double().view(1, -1, 1)
    assert torch.equal(t * 4, (t * 4).round()) and t.abs().max().item() <= 18          # multiples of 1/4 up to 18: 7 bits, exact in fp32 / f16 / bf16
    for T in DT.values():
        assert torch.equal(torch.relu(t).float().to(T).double(), torch.relu(t)) and torch.equal(y.to(T).float(), y)
    assert vox % 256 != 0
    # the mask is not symmetric under an exchange of sample, channel or voxel: two channels differ, two samples differ, and the transposed
    # index (n, v, c) read where it stays inside [N][C][vox] differs from (n, c, v)
    assert not torch.equal(mask[:, 0], mask[:, 1]) and (N == 1 or not torch.equal(mask[0], mask[1]))
    k = min(C, vox)
    assert not torch.equal(mask[:, :k, :k], mask[:, :k, :k].transpose(1, 2))
    frac = mask.float().mean().item()
    assert abs(frac - (1 - p)) < 0.05
    assert float(keep_of(0.5)) == 2.0 and float(keep_of(0.1)).hex() != (1 / 0.9).hex()


@pytest.mark.parametrize('dt', ['f16', 'bf16'])
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('p', DROP_P)
@pytest.mark.parametrize('C,N,vox', DROP_SHAPES)
def test_dropout(nv, dt, mode, masked, p, C, N, vox):
    dtype = DT[dt]
    scale, shift, y, mask = dropout_data(C, N, vox, p)
    ref = dropout_ref(C, N, vox, p, mode, masked, dtype)
    if masked:
        assert not torch.equal(mask[:, 0], mask[:, 1]) and (N == 1 or not torch.equal(mask[0], mask[1]))          # a transposed mask index cannot pass
    code = nv.DTYPE_CODE[dtype]

    def run(pl):
        yo, oo = put(y, dtype, pl['y'], 'y'), out(N, C, vox, dtype, pl['out'], 'out')
        so, ho = dev32(scale, 'scale'), dev32(shift, 'shift')
        ops = [yo, oo, so, ho]
        mo = None
        if masked:
            mo = Operand(1, mask.numel(), torch.uint8, 'tight', mask.reshape(-1), name='mask', band=BAND + vox * (vox + N * C))
            ops.append(mo)
        nv.call('iunet_dl_dropout', code, mode, nv.ptr(yo.t), yo.ss, nv.ptr(oo.t), oo.ss, nv.ptr(so.t), nv.ptr(ho.t),
                None if mo is None else nv.ptr(mo.t), p, C, N, vox, nv.stream())
        return {'out': oo}, ops

    res = over_placements(nv, run, STRIDE_ROWS('y', 'out'))
    got = unblocked(res['out'].logical().reshape(-1), N, C, (vox,))
    assert torch.equal(bits(got), bits(ref)), f'{int((bits(got) != bits(ref)).sum())} elements differ'


# ---------------------------------------------------------------------------------------------------------------- 4. pooling branch
# (N, Cb, C): N C = 360, C C = 5184, C Cb = 2880: every kernel multi-workgroup and ragged; N C > C C: the other arm of n1; C > 256: the
# per-channel BatchNorm backward itself takes two workgroups
POOL_CASES = [(5, 40, 72), (9, 8, 8), (2, 264, 264)]
POOL_EPS = 1e-5
POOL_VAR_MIN = 0.05          # every channel's batch variance of ypool stays above this (pool_data)


@functools.lru_cache(maxsize=None)
def pool_data(N, Cb, C):
    g = gen(8000 + N + C)
    d = dict(xmean=torch.randn(N, Cb, generator=g), wpool=torch.randn(C, Cb, generator=g) * 0.2, wproj=torch.randn(C, 5 * C, generator=g) * 0.2,
             gamma=torch.rand(C, generator=g) + 0.5, beta=torch.randn(C, generator=g) * 0.2, dpsb=torch.randn(N, C, generator=g),
             ypool=torch.randn(N, C, generator=g), rmean=torch.randn(C, generator=g) * 0.2, rvar=torch.rand(C, generator=g) + 0.5,
             pgamma=torch.rand(C, generator=g) + 0.5, pvar=torch.rand(C, generator=g) + 0.5)
    # a channel whose batch variance is small against the float64 reference's own sensitivity (N = 2: |a - b| of the order of the fp32 rounding of
    # ypool over eps) makes the BatchNorm backward ill-conditioned: such a row of wpool is moved along the first sample's centred mean
    v = d['xmean'][0] - d['xmean'].mean(0)
    var = (d['xmean'].double() @ d['wpool'].double().t()).var(0, unbiased=False)
    d['wpool'][var < POOL_VAR_MIN] += (v / v.dot(v)).float()
    return d


def check_pool_conditioning(N, Cb, C):
    d = pool_data(N, Cb, C)
    var = (d['xmean'].double() @ d['wpool'].double().t()).var(0, unbiased=False)
    assert var.min().item() >= POOL_VAR_MIN, var.min().item()


@functools.lru_cache(maxsize=None)
def pool_reference(N, Cb, C):
    """float64 torch with autograd, as tests/test_gpu_deeplabv3.py: test_aspp_dgrad_one_launch_and_pool."""
    d = pool_data(N, Cb, C)
    m = d['xmean'].double().requires_grad_(True)
    wp, wj = d['wpool'].double().requires_grad_(True), d['wproj'].double().requires_grad_(True)
    ga, be = d['gamma'].double().requires_grad_(True), d['beta'].double().requires_grad_(True)
    yp = m @ wp.t()
    psb = torch.relu(F.batch_norm(yp, None, None, ga, be, training=True, eps=POOL_EPS)) @ wj[:, 4 * C:].t()
    psb.backward(d['dpsb'].double())
    return dict(yp=yp.detach(), psb=psb.detach(), dwproj=wj.grad[:, 4 * C:], dgamma=ga.grad, dbeta=be.grad, dwpool=wp.grad, dxmean=m.grad)


def close(a, b):
    """The gate of test_aspp_dgrad_one_launch_and_pool; a NaN (an unwritten element) fails."""
    return bool(((a.double() - b).abs().max() <= 1e-3 * max(1.0, b.abs().max().item())).item())


@pytest.mark.parametrize('N,Cb,C', POOL_CASES)
def test_pool_branch(nv, N, Cb, C):
    d, ref = pool_data(N, Cb, C), pool_reference(N, Cb, C)
    s = nv.stream()
    i = {k: dev32(d[k], k) for k in ('xmean', 'wpool', 'wproj', 'gamma', 'beta', 'dpsb')}
    rm, rv = dev32(torch.zeros(C), 'running_mean'), dev32(torch.ones(C), 'running_var')
    rm.is_input = rv.is_input = False          # updated in place
    o = {k: scratch(n, name=k) for k, n in (('ypool', N * C), ('stats', N * C * 2), ('scale', C), ('shift', C), ('mean', C), ('invstd', C),
                                            ('bp', N * C), ('psb', N * C), ('dwproj', C * 5 * C), ('dgamma', C), ('dbeta', C),
                                            ('dwpool', C * Cb), ('dxmean', N * Cb), ('scratch', 2 * N * C))}
    P = lambda k: nv.ptr((i[k] if k in i else o[k]).t)          # noqa: E731
    nv.call('iunet_dl_pool_gemv', P('xmean'), P('wpool'), P('ypool'), P('stats'), N, Cb, C, s)
    nv.call('iunet_bn_finalize', P('stats'), N, C, float(N), P('gamma'), P('beta'), nv.ptr(rm.t), nv.ptr(rv.t), 0.1, POOL_EPS, P('scale'),
            P('shift'), P('mean'), P('invstd'), s)
    nv.call('iunet_dl_pool_psb', P('ypool'), P('scale'), P('shift'), None, None, None, None, POOL_EPS, P('bp'), P('wproj'), None, None,
            P('psb'), N, C, s)
    torch.cuda.synchronize()
    fwd = {k: o[k].logical().clone() for k in ('ypool', 'mean', 'invstd', 'bp')}
    nv.call('iunet_dl_pool_bwd', P('dpsb'), P('bp'), P('ypool'), P('mean'), P('invstd'), P('gamma'), P('wproj'), P('wpool'), P('xmean'),
            P('dwproj'), P('dgamma'), P('dbeta'), P('dwpool'), P('dxmean'), P('scratch'), N, Cb, C, s)
    torch.cuda.synchronize()
    for op in list(i.values()) + list(o.values()) + [rm, rv]:
        op.check()
    for k, v in fwd.items():
        assert torch.equal(bits(v), bits(o[k].logical())), f'{k}: the backward modified its input'
    L = lambda k: o[k].logical().reshape(-1)          # noqa: E731
    assert close(L('ypool').view(N, C), ref['yp']) and close(L('psb').view(N, C), ref['psb'])
    assert torch.allclose(rm.logical().reshape(-1).double(), 0.1 * ref['yp'].mean(0), atol=1e-4)
    dwj = L('dwproj').view(C, 5 * C)
    assert bool((bits(dwj[:, :4 * C]) == SENTINEL[F32]).all()), 'dWproj: a column outside 4C..5C was written'
    for k, got in (('dwproj', dwj[:, 4 * C:]), ('dgamma', L('dgamma')), ('dbeta', L('dbeta')), ('dwpool', L('dwpool').view(C, Cb)),
                   ('dxmean', L('dxmean').view(N, Cb))):
        assert close(got, ref[k]), (k, (got.double() - ref[k]).abs().max().item(), ref[k].abs().max().item())


@pytest.mark.parametrize('fold', [False, True])
@pytest.mark.parametrize('N,Cb,C', POOL_CASES)
def test_pool_psb_eval(nv, N, Cb, C, fold):
    """scale = NULL: bp from the running statistics' fold, with and without the projection's eval BatchNorm scale on psb; against float64, and
    bit for bit against the training form handed fold_ref's (scale, shift): bn_fold_scale / bn_fold_bias are under the fold contract."""
    d = pool_data(N, Cb, C)
    bn = (d['gamma'], d['beta'], d['rmean'], d['rvar'])
    sc, sh = fold_ref(torch.ones(C), bn, POOL_EPS, False)
    a = d['gamma'].double() / torch.sqrt(d['rvar'].double() + POOL_EPS)
    bp_ref = torch.relu(a * d['ypool'].double() + (d['beta'].double() - d['rmean'].double() * a))
    psb_ref = bp_ref @ d['wproj'].double()[:, 4 * C:].t()
    if fold:
        psb_ref = psb_ref * (d['pgamma'].double() / torch.sqrt(d['pvar'].double() + POOL_EPS))
    s = nv.stream()
    got = []
    for form in ('eval', 'train'):
        i = {k: dev32(d[k], k) for k in ('ypool', 'wproj', 'gamma', 'beta', 'rmean', 'rvar', 'pgamma', 'pvar')}
        i['scale'], i['shift'] = dev32(sc, 'scale'), dev32(sh, 'shift')
        bp, psb = scratch(N * C, name='bp'), scratch(N * C, name='psb')
        P = lambda k: nv.ptr(i[k].t)          # noqa: E731
        pg, pv = (P('pgamma'), P('pvar')) if fold else (None, None)
        if form == 'eval':
            nv.call('iunet_dl_pool_psb', P('ypool'), None, None, P('gamma'), P('beta'), P('rmean'), P('rvar'), POOL_EPS, nv.ptr(bp.t),
                    P('wproj'), pg, pv, nv.ptr(psb.t), N, C, s)
        else:
            nv.call('iunet_dl_pool_psb', P('ypool'), P('scale'), P('shift'), None, None, None, None, POOL_EPS, nv.ptr(bp.t), P('wproj'), pg, pv,
                    nv.ptr(psb.t), N, C, s)
        torch.cuda.synchronize()
        for op in list(i.values()) + [bp, psb]:
            op.check()
        got.append((bp.logical().reshape(N, C), psb.logical().reshape(N, C)))
    assert close(got[0][0], bp_ref) and close(got[0][1], psb_ref)
    assert torch.equal(bits(got[0][0]), bits(got[1][0])), 'bp: the eval fold differs from the training form on the folded scale and shift'
    assert torch.equal(bits(got[0][1]), bits(got[1][1])), 'psb'
