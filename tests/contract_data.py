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


# ---------------------------------------------------------------------------------------------------------------- split-precision matrix
# Data on which the prediction kernels (tests/test_gpu_x2_matrix.py) are EXACT, and the conditions that make them so, asserted here.
import numpy as np
import torch.nn.functional as F

from oracle import unet_ref

X2_ACT_IN, X2_ACT_OUT = 64.0, 16.0          # fp16x2 exact rows: the accumulator is divided by 4
X2_EXACT_BOUND = float(1 << 17)
X2M_EXACT_BOUND = float(1 << 18)


def conv_nd(nd):
    return F.conv2d if nd == 2 else F.conv3d


def convT_nd(nd):
    return F.conv_transpose2d if nd == 2 else F.conv_transpose3d


def e4m3_round(v):
    """The nearest e4m3 value (ties to even, saturating at +-448) by the project's CPU codec, as fp32."""
    return torch.from_numpy(unet_ref.round_e4m3(np.clip(v.detach().numpy().astype(np.float32), -448.0, 448.0)))


def e4m3_codes(v):
    """The e4m3 byte of every value (rounded by the codec first: the cast itself is then exact)."""
    return e4m3_round(v).to(torch.float8_e4m3fn).view(torch.uint8)


def e4m3_values(codes):
    return codes.contiguous().view(torch.float8_e4m3fn).float()


def lo8_interval(lo_words):
    """The interval rule for a lo8 byte beside NON-exact words (hi, lo): the residual the device rounded lies in the fp16 rounding
    interval [l-, l+] of the lo word it stored, and e4m3 rounding is monotone, so e4m3(16 l-) <= byte <= e4m3(16 l+) as e4m3 VALUES.
    lo_words: fp32 tensor of fp16 values -> (lowest, highest) admissible value."""
    l = lo_words.numpy().astype(np.float16)
    dn = (l.astype(np.float64) + np.nextafter(l, np.float16(-np.inf)).astype(np.float64)) / 2
    up = (l.astype(np.float64) + np.nextafter(l, np.float16(np.inf)).astype(np.float64)) / 2
    f = lambda a: e4m3_round(torch.from_numpy((16.0 * a).astype(np.float32)))          # (12 significant bits: exact in fp32)
    return f(dn), f(up)


def lo8_in_interval(codes, lo_words):
    """[bool]: every byte obeys the interval rule; the count of bytes that do not."""
    lo, hi = lo8_interval(lo_words)
    v = e4m3_values(codes)
    bad = ~((v >= lo) & (v <= hi))          # (a NaN code fails; -0 == +0 as values)
    return int(bad.sum())


def pool_key(hi_words, lo8_codes):
    """common.h's x2m_pool_keys on the CPU: the 24-bit key [sortable hi word | sortable lo8 byte] (sign-magnitude -> offset binary) as int64.
    hi_words: fp16 tensor, lo8_codes: uint8 tensor of the same shape."""
    h = hi_words.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF
    b = lo8_codes.to(torch.int64)
    hs = torch.where(h >= 0x8000, h ^ 0xFFFF, h ^ 0x8000)
    bs = torch.where(b >= 0x80, b ^ 0xFF, b ^ 0x80)
    return (hs << 8) | bs


def pool_unkey(key):
    hs, bs = key >> 8, key & 0xFF
    h = torch.where(hs >= 0x8000, hs ^ 0x8000, hs ^ 0xFFFF)
    b = torch.where(bs >= 0x80, bs ^ 0x80, bs ^ 0xFF)
    h = torch.where(h >= 0x8000, h - 0x10000, h).to(torch.int16).view(torch.float16)
    return h, b.to(torch.uint8)


def windows(t, nd):
    """[N, C, (D,) H, W] -> [N, C, (D/2,) H/2, W/2, 2^nd]: the candidates of every 2^nd pool window."""
    if nd == 2:
        N, C, H, W = t.shape
        return t.reshape(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)
    N, C, D, H, W = t.shape
    return t.reshape(N, C, D // 2, 2, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(N, C, D // 2, H // 2, W // 2, 8)


def pool_by_key(hi_words, lo8_codes, nd):
    """The pooled (hi words, lo8 bytes): per window the pair with the largest key."""
    return pool_unkey(windows(pool_key(hi_words, lo8_codes), nd).max(-1).values)


POOL_HI = torch.tensor([0.0, -0.0, 1.0, -1.0, 2.0, -2.0, 0.5, 3.0], dtype=torch.float16)          # both zero signs, negative values


@functools.lru_cache(maxsize=None)
def pool_tie_data(N, C, sp, seed):
    """hi words from POOL_HI, a second word in -2..2 (lo words as they are; lo8 bytes as e4m3 codes of them): windows whose maximum hi is
    shared while the second word decides (>= 5 %), windows whose whole best pair ties (>= 1 %).  -> hi fp16 [N, C, *sp], second fp32."""
    g, nd = gen(seed), len(sp)
    hi = POOL_HI[torch.randint(0, len(POOL_HI), (N, C) + tuple(sp), generator=g)]
    lo = torch.randint(-2, 3, (N, C) + tuple(sp), generator=g).float()
    hw, lw = windows(hi.float(), nd), windows(lo, nd)
    top = hw == hw.max(-1, keepdim=True).values
    shared = top.sum(-1) > 1
    best_lo = torch.where(top, lw, torch.full_like(lw, -9.0)).max(-1, keepdim=True).values
    whole = (top & (lw == best_lo)).sum(-1) > 1
    decides = shared & (torch.where(top, lw, torch.full_like(lw, 9.0)).min(-1).values < best_lo.squeeze(-1))
    assert decides.float().mean().item() >= 0.05, f'the second word decides only {100 * decides.float().mean().item():.1f} % of the windows'
    assert whole.float().mean().item() >= 0.01, f'only {100 * whole.float().mean().item():.2f} % of the windows tie in the whole pair'
    assert bool((hi.view(torch.int16) == -32768).any()) and bool((hi.float() < 0).any())
    return hi, lo


@functools.lru_cache(maxsize=None)
def x2m_exact_operator(nd, co, ci, seed):
    """Entries 16 a + b / 256: |a| in {36, 40, .., 60} (w_hi = 16 a exactly: |b| / 256 stays under half an fp16 ulp of it; a is an e4m3 value =
    w_hi8), b in 16 x {-3 .. 3} (= w_lo8).  -> a, b, w"""
    g = gen(seed)
    shape = (co, ci) + (3,) * nd
    a = (torch.randint(9, 16, shape, generator=g) * 4).float() * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()
    b = (torch.randint(-3, 4, shape, generator=g) * 16).float()
    w = 16.0 * a + b / 256.0
    assert torch.equal(w.double(), 16.0 * a.double() + b.double() / 256.0) and torch.equal((16.0 * a).half().float(), 16.0 * a)
    assert torch.equal(w.half().float(), 16.0 * a) and torch.equal(e4m3_round(a), a) and torch.equal(e4m3_round(b), b)
    m = w.abs().reshape(co, -1).max(1).values
    assert bool(((m >= 512) & (m < 1024)).all())          # the row scale is 1
    return a, b, w


@functools.lru_cache(maxsize=None)
def x2m_exact_input(N, ci, sp, seed):
    """hi planes sparse -1 / 0 / 1 (hi8 = hi / 256 exactly, a subnormal of e4m3), hand-made lo8 planes in -4..4."""
    g = gen(seed)
    X = (torch.randint(-1, 2, (N, ci) + tuple(sp), generator=g) * (torch.rand((N, ci) + tuple(sp), generator=g) < 0.25)).float()
    L8 = torch.randint(-4, 5, (N, ci) + tuple(sp), generator=g).float()
    assert torch.equal(e4m3_round(X / 256.0), X / 256.0) and torch.equal(e4m3_round(L8), L8)
    return X, L8


def x2m_exact_ref(nd, X, L8, a, b):
    """float64 x_hi w_hi + x_lo8 w_hi8 + x_hi8 w_lo8 (the accumulator: 64 x the value stored at act_out = 1), one conv over [X | L8]."""
    want = conv_nd(nd)(torch.cat([X, L8], 1).double(), torch.cat([16.0 * a + b / 256.0, a], 1).double(), padding=1)
    assert float(want.abs().max()) < X2M_EXACT_BOUND          # + 4 fraction bits = 22: hi + lo hold acc / 64 exactly
    return want


@functools.lru_cache(maxsize=None)
def split_exact_operator(shape, co_axis, seed):
    """A sparse operator whose nonzero entries are h + r: |h| a multiple of 1/2 in [512, 1024) (an fp16 value at spacing 1/2, so w_hi = h and
    the row scale is 1), r in {0, +-1/16, +-2/16, +-3/16} (under half that spacing: w_lo = r exactly).  About 120 nonzero entries per
    output channel whatever the shape.  (|h| starts at 512.5: 512 - 3/16 would fall into the binade below, spacing 1/4.)  -> h, r (fp32, the operator is h + r)"""
    g = gen(seed)
    per_row = int(np.prod(shape)) // shape[co_axis]
    keep = torch.rand(shape, generator=g) < min(0.5, 120.0 / per_row)
    h = (torch.randint(1025, 2048, shape, generator=g).float() / 2) * (torch.randint(0, 2, shape, generator=g) * 2 - 1).float() * keep
    r = torch.randint(-3, 4, shape, generator=g).float() / 16 * keep
    w = h + r
    assert torch.equal(w.double(), h.double() + r.double()) and torch.equal(w.half().float(), h) and torch.equal((w - h).half().float(), r)
    m = w.abs().transpose(0, co_axis).reshape(shape[co_axis], -1).max(1).values
    assert bool(((m >= 512) & (m < 1024)).all())          # every output channel has an entry: its row scale is 1
    assert float((r[keep] != 0).float().mean()) >= 0.25
    return h, r


@functools.lru_cache(maxsize=None)
def split_exact_input(N, ci, sp, seed):
    """Hand-made planes (a non-canonical split: the kernels only consume words): x_hi sparse integers in -1..1, x_lo multiples of 1/8 in
    [-3/8, 3/8], drawn independently of x_hi and nonzero on about half of the elements."""
    g = gen(seed)
    shape = (N, ci) + tuple(sp)
    xh = (torch.randint(-1, 2, shape, generator=g) * (torch.rand(shape, generator=g) < 0.25)).float()
    xl = torch.randint(-3, 4, shape, generator=g).float() / 8 * (torch.rand(shape, generator=g) < 0.5)
    assert float((xl != 0).float().mean()) > 0.3 and float(((xl != 0) & (xh == 0)).float().mean()) > 0.2
    return xh, xl


def split_exact_ref(nd, xh, xl, h, r, transposed):
    """float64 op(x_hi, w_hi) + op(x_lo, w_hi) + op(x_hi, w_lo) -- the kernels drop the fourth term by design -- as two operations:
    op(x_hi, w_hi + w_lo) + op(x_lo, w_hi).  Every term is a multiple of 1/16 and the sum of the absolute terms stays below 2^17 everywhere,
    so every partial sum in any order is exact in fp32 (21 bits)."""
    op = (lambda x, w: convT_nd(nd)(x, w, stride=2)) if transposed else (lambda x, w: conv_nd(nd)(x, w, padding=1))
    want = op(xh.double(), (h + r).double()) + op(xl.double(), h.double())
    mag = op(xh.abs().double(), (h.abs() + r.abs()).double()) + op(xl.abs().double(), h.abs().double())
    assert float(mag.max()) < X2_EXACT_BOUND, f'sum of absolute terms {float(mag.max()):.0f}'
    assert torch.equal(want * 16, (want * 16).round())
    return want


def split_store(acc, bias):
    """What an exact row stores, before any ReLU: v = acc x act_out / act_in + act_out x bias (integer biases; the row scale is 1) -- a
    multiple of 1/64 below 2^15 + 64, at most 22 significant bits.  -> v (float64)"""
    shape = [1, -1] + [1] * (acc.dim() - 2)
    v = acc * (X2_ACT_OUT / X2_ACT_IN) + X2_ACT_OUT * bias.double().view(shape)
    return v


def split_words_of(v):
    """float64 values (exact in fp32) -> hi = f16(v), lo = f16(v - hi), asserted to return v exactly."""
    assert float(v.abs().max()) < 65504 and torch.equal(v.float().double(), v)
    hi = v.float().half().float()
    lo = (v.float() - hi).half().float()
    assert torch.equal(hi.double() + lo.double(), v)
    return hi, lo
