"""Data and CPU references of the numeric-contract tests (tests/test_gpu_head_contract.py, tests/test_gpu_fold_contract.py), and the
properties of that data the tests' assertions lean on -- asserted here, on the reference alone, so that tests/test_numeric_contracts_cpu.py
checks them without a GPU.  Nothing in this module touches a device."""
import functools

import torch

from tests.arena import fold_ref, sqrt_rn

F32 = torch.float32


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------- head
HEAD_N, HEAD_C0, ACT_SCALE = 2, 32, 64.0
HEAD_GRIDS = {'2d_8x40': (1, 8, 40), '3d_2x8x24': (2, 8, 24)}
HEAD_NCLS = (2, 5, 10)
TIED = {2: (0, 1), 5: (1, 3), 10: (2, 7)}          # the two classes whose biases tie for the largest


def first_max(p):
    """[N, C, ...] -> the index of the first maximum along dim 1, written out (no library's tie rule involved)."""
    is_max = p == p.max(1, keepdim=True).values
    return (is_max & (is_max.int().cumsum(1) == 1)).int().argmax(1).long()


@functools.lru_cache(maxsize=None)
def head_data(ncls, gk):
    """Features in -2..2 (every 16th voxel or so all zero: its logits are the biases, whose largest value two classes share), weights
    multiples of 1/8 in [-1, 1], biases multiples of 1/4.  -> x [N, C0, D, H, W], w [ncls, C0], b [ncls], logits fp32, first-max class of the
    logits, share of voxels with a tie for the maximum."""
    grid = HEAD_GRIDS[gk]
    g = gen(4100 + 10 * ncls + grid[0])
    x = torch.randint(-2, 3, (HEAD_N, HEAD_C0) + grid, generator=g).float()
    x = x * (torch.rand((HEAD_N, 1) + grid, generator=g) >= 1 / 16).float()
    w = torch.randint(-8, 9, (ncls, HEAD_C0), generator=g).float() / 8
    b = torch.randint(-8, 9, (ncls,), generator=g).float() / 4
    b[list(TIED[ncls])] = float(b.max()) + 0.25
    l64 = torch.einsum('kc,ncdhw->nkdhw', w.double(), x.double()) + b.double().view(1, -1, 1, 1, 1)
    logits = l64.float()
    # every logit -- and every partial sum of it, in any order: sums of multiples of 1/8 bounded by sum |w x| + |b| -- is a multiple of 1/8
    # below 2^7, so exact in fp32 whatever the summation order and whether the products are fused or not
    bound = float((w.abs().sum(1) * 2 + b.abs()).max())
    assert bound < 128 and torch.equal(logits.double(), l64) and torch.equal(l64 * 8, (l64 * 8).round())
    # ... the features are exact in f16 and bf16, and as split words at act_scale 64 with a zero lo word
    assert torch.equal(x.half().float(), x) and torch.equal(x.bfloat16().float(), x)
    hi = (x * ACT_SCALE).half()
    assert torch.equal(hi.float(), x * ACT_SCALE) and float((x * ACT_SCALE).abs().max()) <= 128
    is_max = logits == logits.max(1, keepdim=True).values
    ties = (is_max.sum(1) > 1).float().mean().item()
    cls = first_max(logits)
    assert ties >= 0.01, f'only {100 * ties:.2f} % of the voxels tie for the maximum'
    assert bool(((is_max.sum(1) > 1) & (cls == TIED[ncls][0])).any())          # ties whose first maximum is the class the biases tie at
    return x, w, b, logits, cls.to(torch.uint8), ties


def nhwc8(x, dtype):
    """[N, C, D, H, W] -> the blocked layout [N, C / 8 planes, vox, 8] of the 16-bit kernels, flat per sample."""
    N, C = x.shape[:2]
    return x.reshape(N, C // 8, 8, -1).permute(0, 1, 3, 2).contiguous().to(dtype).reshape(N, -1)


def split_words(x):
    """[N, C, D, H, W] -> [hi planes | lo planes] of act_scale * x in f16, flat per sample (the lo planes C / 8 planes further on)."""
    v = x * ACT_SCALE
    hi = v.half()
    lo = (v - hi.float()).half()
    assert not bool(lo.float().abs().max())          # zero lo words: the features are exact as hi words alone
    return torch.cat([nhwc8(hi.float(), torch.float16), nhwc8(lo.float(), torch.float16)], 1)


UP_SHAPES = [(2, (5, 7), 8, 2), (3, (3, 2, 2), 2, 5)]          # (nd, coarse grid, s, ncls): two of test_upsample_head_contract's


@functools.lru_cache(maxsize=None)
def up_data(nd, coarse, s, ncls):
    return torch.randn((HEAD_N, ncls) + coarse, generator=gen(4300 + nd))


# ---------------------------------------------------------------------------------------------------------------- fold and scales
EPS = 2.0 ** -16          # a power of two, so that a channel's var + eps can be exactly 1
POW2_CH, ZERO_CH = 3, 5          # the channel whose max |w'| is an exact power of two (2^-3), the all-zero channel
ACT_IN, ACT_OUT = 64.0, 32.0


def fused_bias(bn, eps):
    """What ONE fused multiply-add gives for the bias: beta - mean * a with the product not rounded (fp32 x fp32 is exact in float64)."""
    gamma, beta, mean, var = bn
    a = gamma / sqrt_rn(var + torch.tensor(eps, dtype=F32))
    return (beta.double() - mean.double() * a.double()).float()


@functools.lru_cache(maxsize=None)
def bn_data(C, seed):
    """gamma, var in [0.5, 1.5], mean and beta of order 0.2; channel POW2_CH folds with a = 1 exactly."""
    g = gen(seed)
    gamma, var = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5
    beta, mean = 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    gamma[POW2_CH], var[POW2_CH] = 1.0, 1.0 - EPS
    bn = (gamma, beta, mean, var)
    a = gamma / sqrt_rn(var + torch.tensor(EPS, dtype=F32))
    assert float(a[POW2_CH]) == 1.0
    sep = beta - mean * a
    differ = int((sep != fused_bias(bn, EPS)).sum())
    assert differ > 0, 'the fused and the separately rounded bias agree on every channel: the data cannot tell them apart'
    return bn


def operator(shape, co_axis, seed):
    """Random weights; along the output-channel axis, channel POW2_CH has max |w| = 2^-3 exactly and channel ZERO_CH is all zero."""
    w = torch.randn(shape, generator=gen(seed)) * 0.1
    idx = [slice(None)] * len(shape)
    idx[co_axis] = POW2_CH
    row = w[tuple(idx)].clamp(-0.12, 0.12)
    row.view(-1)[7] = -0.125
    w[tuple(idx)] = row
    idx[co_axis] = ZERO_CH
    w[tuple(idx)] = 0.0
    return w


def row_scale(wf, co_axis):
    """s = 2^k per output channel with max |w'| s in [2^9, 2^10) (k clamped to +-40; 1 for an all-zero row)."""
    m = wf.abs().transpose(0, co_axis).reshape(wf.shape[co_axis], -1).max(1).values
    _, e = torch.frexp(m)          # m = f 2^e, f in [0.5, 1)
    s = torch.where(m > 0, torch.ldexp(torch.ones_like(m), (10 - e).clamp(-40, 40)), torch.ones_like(m))
    ms = m * s
    assert bool((((ms >= 512) & (ms < 1024)) | (m == 0)).all())
    assert float(ms[POW2_CH]) == 512.0 and float(m[POW2_CH]) == 0.125 and float(m[ZERO_CH]) == 0.0 and float(s[ZERO_CH]) == 1.0
    return s


def split_ref(w, bn, bias_in, transposed):
    """The split-precision operator preparation on the CPU: w' = fold(w), s, hi = f16(w' s), lo = f16(w' s - hi), oscale, bias_out."""
    co_axis = 1 if transposed else 0
    if bn is not None:
        wf, bias = fold_ref(w, bn, EPS, transposed)
    else:
        wf, bias = w, (bias_in if bias_in is not None else torch.zeros(w.shape[co_axis]))
    s = row_scale(wf, co_axis)
    shape = [1] * w.dim()
    shape[co_axis] = -1
    v = wf * s.view(shape)
    assert torch.equal(v.double(), wf.double() * s.double().view(shape)) and float(v.abs().max()) < 65504          # a power of two: exact
    hi = v.half()
    res = v - hi.float()
    assert torch.equal(res.double(), v.double() - hi.double())          # the residual is exact in fp32
    lo = res.half()
    return hi.float(), lo.float(), torch.tensor(ACT_OUT) / (torch.tensor(ACT_IN) * s), bias * ACT_OUT


def x2_virtual_conv(hi, lo, kc):
    """kind 0: [Cout][Cin][taps] -> [Cout][3 Cin][taps], per chunk of kc channels the rows [hi | hi | lo]."""
    cout, cin, taps = hi.shape
    h, l = hi.view(cout, cin // kc, kc, taps), lo.view(cout, cin // kc, kc, taps)
    return torch.stack([h, h, l], 2).reshape(cout, 3 * cin, taps)


def x2_chunked_convT(hi, lo, kc):
    """kind 2: [Cin][Cout][npos] -> [2 Cin][Cout][npos], chunks of kc k-steps of 32 channels [chunk][hi | lo][kc][32]."""
    cin, cout, npos = hi.shape
    h, l = hi.view(cin // (32 * kc), kc * 32, cout, npos), lo.view(cin // (32 * kc), kc * 32, cout, npos)
    return torch.stack([h, l], 1).reshape(2 * cin, cout, npos)


def lk_convT_ref(wf, nd):
    """iunet_lk_pack kind 2 restated: w' [Cin][Cout][4^d] -> [2^d classes][Cout][2^d taps x Cin]; class p and tap t pick, per axis, filter
    index 2 - 2 b (odd output parity) or 1 + 2 b (even), b = the tap's bit."""
    cin, cout = wf.shape[:2]
    ntap = 1 << nd
    out = torch.zeros(ntap, cout, ntap * cin)
    for p in range(ntap):
        for t in range(ntap):
            k = [(2 - 2 * ((t >> a) & 1)) if (p >> a) & 1 else (1 + 2 * ((t >> a) & 1)) for a in range(nd)]          # axis 0 = w, 1 = h, 2 = d
            kidx = sum(k[a] * 4 ** a for a in range(nd))
            out[p, :, t * cin:(t + 1) * cin] = wf[:, :, kidx].t()
    return out
