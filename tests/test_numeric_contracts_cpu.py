"""Without a GPU: the properties of the data that tests/test_gpu_head_contract.py and tests/test_gpu_fold_contract.py lean on (exact
logits, ties, a fused bias that differs from the separately rounded one, the power-of-two and the all-zero channel), the CPU references'
own layout arithmetic, and that each shared numeric contract of csrc/ has exactly one definition."""
import glob
import os
import re

import pytest
import torch

from tests import contract_data as cd
from tests.arena import fold_ref, sqrt_rn

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'interactive-unet_amd', 'csrc')


@pytest.mark.parametrize('gk', list(cd.HEAD_GRIDS))
@pytest.mark.parametrize('ncls', cd.HEAD_NCLS)
def test_head_data_is_exact_and_has_ties(ncls, gk):
    x, w, b, logits, cls, ties = cd.head_data(ncls, gk)          # asserts exactness and the tie share itself
    D, H, W = cd.HEAD_GRIDS[gk]
    vox = D * H * W
    assert vox > 256 and vox % 256, 'two workgroups of 256 voxels, the second ragged'
    assert ties >= 0.01 and x.shape == (cd.HEAD_N, cd.HEAD_C0, D, H, W)
    assert float(x.abs().max()) == 2 and torch.equal(w * 8, (w * 8).round()) and float(w.abs().max()) <= 1 and torch.equal(b * 4, (b * 4).round())
    # exact in ANY order: the fp32 sum over the channels in reverse, and in four groups of eight, gives the same bits
    rev = torch.einsum('kc,ncdhw->nkdhw', w.flip(1), x.flip(1)) + b.view(1, -1, 1, 1, 1)
    grp = sum(torch.einsum('kc,ncdhw->nkdhw', w[:, i:i + 8], x[:, i:i + 8]) for i in range(0, 32, 8)) + b.view(1, -1, 1, 1, 1)
    assert torch.equal(rev, logits) and torch.equal(grp, logits)
    # the layouts the 16-bit and the split-precision head read hold the same values
    back = cd.nhwc8(x, torch.float16).float().view(cd.HEAD_N, 4, vox, 8).permute(0, 1, 3, 2).reshape(x.shape)
    assert torch.equal(back, x)
    words = cd.split_words(x).float().view(cd.HEAD_N, 2, 4, vox, 8)
    assert torch.equal(words[:, 0].permute(0, 1, 3, 2).reshape(x.shape), x * cd.ACT_SCALE) and not bool(words[:, 1].abs().max())
    # the tie rule: the first maximum, and at a tie that is not the last one
    is_max = logits == logits.max(1, keepdim=True).values
    tie = is_max.sum(1) > 1
    last = (ncls - 1) - is_max.flip(1).int().argmax(1)
    assert bool((cls.long()[tie] < last[tie]).all()) and bool((cls.long()[~tie] == last[~tie]).all())


def test_fold_data_tells_a_fused_bias_from_a_separately_rounded_one():
    bn = cd.bn_data(32, 5001)
    gamma, beta, mean, var = bn
    assert 0.5 <= float(gamma.min()) and float(gamma.max()) <= 1.5 and 0.5 <= float(var.min()) and float(var.max()) <= 1.5
    _, sep = fold_ref(torch.zeros(32, 1), bn, cd.EPS, 0)
    fused = cd.fused_bias(bn, cd.EPS)
    differ = int((sep != fused).sum())
    assert differ > 0
    # ... by one unit in the last place at the most
    ulp = torch.maximum(sep.abs(), fused.abs()) * 2.0 ** -23
    assert bool(((sep - fused).abs() <= ulp).all())
    a = gamma / sqrt_rn(var + torch.tensor(cd.EPS))
    assert float(a[cd.POW2_CH]) == 1.0


@pytest.mark.parametrize('transposed', [0, 1])
def test_split_reference_channels(transposed):
    shape = (64, 32, 4) if transposed else (32, 16, 27)
    w = cd.operator(shape, 1 if transposed else 0, 7)
    hi, lo, oscale, bias = cd.split_ref(w, cd.bn_data(32, 5001), None, transposed)          # asserts [2^9, 2^10), the 2^-3 and the zero channel
    sel = (lambda t, c: t[:, c]) if transposed else (lambda t, c: t[c])
    assert float(sel(hi, cd.POW2_CH).abs().max()) == 512.0 and not bool(sel(hi, cd.ZERO_CH).abs().max()) and not bool(sel(lo, cd.ZERO_CH).abs().max())
    assert float(oscale[cd.ZERO_CH]) == cd.ACT_OUT / cd.ACT_IN and float(oscale[cd.POW2_CH]) == cd.ACT_OUT / (cd.ACT_IN * 4096)
    assert bool(lo.abs().max() > 0) and torch.equal(hi.half().float(), hi) and torch.equal(lo.half().float(), lo)


def test_reference_layouts():
    hi, lo = torch.arange(2 * 32 * 3).float().view(2, 32, 3), -torch.arange(2 * 32 * 3).float().view(2, 32, 3)
    v = cd.x2_virtual_conv(hi, lo, 16)          # per chunk of 16 channels: [hi | hi | lo]
    assert v.shape == (2, 96, 3) and torch.equal(v[:, 0:16], hi[:, :16]) and torch.equal(v[:, 16:32], hi[:, :16]) and torch.equal(v[:, 32:48], lo[:, :16])
    assert torch.equal(v[:, 48:64], hi[:, 16:]) and torch.equal(v[:, 80:96], lo[:, 16:])
    h, l = torch.arange(64 * 2 * 4).float().view(64, 2, 4), -torch.arange(64 * 2 * 4).float().view(64, 2, 4)
    c1, c2 = cd.x2_chunked_convT(h, l, 1), cd.x2_chunked_convT(h, l, 2)
    assert torch.equal(c1[0:32], h[:32]) and torch.equal(c1[32:64], l[:32]) and torch.equal(c1[64:96], h[32:]) and torch.equal(c1[96:], l[32:])
    assert torch.equal(c2[:64], h) and torch.equal(c2[64:], l)
    wf = torch.randn(3, 2, 16, generator=cd.gen(9))
    r = cd.lk_convT_ref(wf, 2)          # class p = (ph, pw), tap t = (bh, bw): filter index (kh, kw), k = 2 - 2 b (odd parity) or 1 + 2 b (even)
    assert r.shape == (4, 2, 12)
    for p in range(4):
        for t in range(4):
            kw = (2 - 2 * (t & 1)) if p & 1 else (1 + 2 * (t & 1))
            kh = (2 - 2 * (t >> 1)) if p >> 1 else (1 + 2 * (t >> 1))
            assert torch.equal(r[p, :, 3 * t:3 * t + 3], wf[:, :, kh * 4 + kw].t())


ONE_DEFINITION = ['float bn_fold_scale(', 'float bn_fold_mul(', 'float bn_fold_bias(', 'float round_e4m3(', 'unsigned char encode_e4m3(',
                  'float e4m3_scale(', 'float split_row_scale(', 'float block_max_256(', 'void head_store(', 'struct HeadOut {',
                  # the resident-volume rules (volume_rules.h): plane point, inside test, samplers, class, streaming select, host helpers
                  'double plane_point(', 'double slab_point(', 'bool coord_inside(', 'double coord_nearest(', 'int volume_mirror(',
                  'unsigned char volume_sample_linear(', 'TopByte volume_top_byte(', 'void volume_select_kernel(', 'void volume_select_launch(',
                  'long long volume_align16(', 'bool volume_ok(', 'unsigned int volume_grid(', 'define VOLUME_REQUIRE_DIMS(',
                  # the decoders' grid-moving rules (resample.h): channel groups, the tap record and its three index rules, the tap walk, the adjoint
                  'struct ChanGroup {', 'void group_load(', 'void group_store(', 'struct ResampleAx {', 'ResampleAx resample_axis_f32(',
                  'ResampleAx resample_axis_exact(', 'ResampleAx resample_axis_corners(', 'void resample_taps(', 'void resample_adj_range(',
                  'long long pn_adj_extent(', 'float resample_adj_w(', 'void resample_adjoint_kernel(', 'void resample_adjoint_wide_kernel(']
HOMES = ('common.h', 'head_out.h', 'volume_rules.h', 'resample.h')
RETIRED_RESAMPLE = (r'\b(sf_axis|pn_axis|dl_lerp|SfAx|PnAx|pn_load|pn_store|pn_act|PnLay|ma_ld|ma_st|ma_act|MaLay|sf_pro|sf_adj_range|pn_adj_range|'
                    r'sf_adj_w|pn_adj_w|sf_adjoint_kernel|pn_adjoint_kernel)\b')


def test_each_shared_contract_is_defined_once():
    text = {p: open(p).read() for p in glob.glob(os.path.join(CSRC, '*.h')) + glob.glob(os.path.join(CSRC, '*.hip'))}
    for needle in ONE_DEFINITION:
        hits = [(os.path.basename(p), t.count(needle)) for p, t in text.items() if needle in t]
        assert len(hits) == 1 and hits[0][1] == 1 and hits[0][0] in HOMES, (needle, hits)
    # what the single definitions replaced stays gone: hand-written folds, the second e4m3 codec, the head's fields copied into a struct,
    # the resident-volume kernels' own mirrors, alignment helpers and streaming passes
    for p, t in text.items():
        assert not re.search(r'\b(slab_mirror|mirror_idx|cc_align16|ed_align16|filter_kernel|select_kernel)\b', t), \
            f'{os.path.basename(p)}: a retired copy of a resident-volume rule is back'
        assert not re.search(RETIRED_RESAMPLE, t), f'{os.path.basename(p)}: a retired copy of a resampling or channel-group rule is back'
        if os.path.basename(p) in HOMES:
            continue
        assert not re.search(r'/\s*sqrtf\(\s*(\w+\.)?var\b', t), f'{os.path.basename(p)}: a BatchNorm scale written out by hand'
        assert not re.search(r'\b(f8_round_e4m3|f8_encode_e4m3|mul_rn)\b', t), f'{os.path.basename(p)}: a retired copy is back'
        assert not re.search(r'long long oN, oC, oD, oH, oW;', t), f'{os.path.basename(p)}: the head output fields copied by hand'
