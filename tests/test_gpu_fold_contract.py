"""The eval-mode BatchNorm fold (csrc/common.h: bn_fold_scale / bn_fold_mul / bn_fold_bias) and the split-precision row scale
(split_row_scale) read back from the pack entry points that had no read-back test: iunet_x2_prep (kinds 0 and 2), iunet_x2m_prep_nd
(nd 2 and 3), iunet_lk_pack and iunet_dl_pack (fp32 operators).  Everything is compared bit for bit with tests/arena.py: fold_ref -- every
operation rounded on its own, the root correctly rounded -- and, for the split operators, with
    s = 2^k, max |w'| s in [2^9, 2^10);  hi = f16(w' s), lo = f16(w' s - hi);  oscale = act_out / (act_in s);  bias_out = bias act_out.
One output channel's max |w'| is an exact power of two, one is all zero (s = 1); the BatchNorm vectors are such that ONE fused multiply-add
would give another bias than the two separately rounded operations on some channels (tests/contract_data.py asserts all of it).
Every operand sits in a sentinel arena.  Needs an MI355X: run with -m gpu."""
import pytest
import torch

from tests import contract_data as cd
from tests.arena import SENTINEL, Operand, bits, fold_ref, scratch

pytestmark = pytest.mark.gpu

F32 = torch.float32
COUT = 32


@pytest.fixture(scope='module')
def nv():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from interactive_unet import _native
    _native.lib()
    return _native


def vec(t, name):
    return Operand(1, t.numel(), F32, 'tight', t.reshape(1, -1), name=name)


def same_bits(got, ref, what):
    got, ref = got.reshape(-1), ref.reshape(-1)
    assert got.numel() == ref.numel() and torch.equal(bits(got), bits(ref)), \
        f'{what}: {int((bits(got) != bits(ref)).sum()) if got.numel() == ref.numel() else "size"} of {ref.numel()} elements differ in their bits'


def bn_operands(bn):
    return [vec(t, k) for t, k in zip(bn, ('gamma', 'beta', 'mean', 'var'))]


def finish(inputs, outputs):
    torch.cuda.synchronize()
    for o in inputs:
        o.check_unchanged()
    for o in outputs:
        o.check_outside()


X2_PREP = [pytest.param(0, 16, 27, 16, 'fold', id='kind0-cin16-27taps-kc16-fold'), pytest.param(0, 32, 9, 32, 'fold', id='kind0-cin32-9taps-kc32-fold'),
           pytest.param(2, 96, 4, 1, 'bias_in', id='kind2-cin96-4pos-bias_in'), pytest.param(2, 64, 8, 2, 'fold', id='kind2-cin64-8pos-fold')]


@pytest.mark.parametrize('kind,cin,taps,kc,bias', X2_PREP)
def test_x2_prep_read_back(nv, kind, cin, taps, kc, bias):
    transposed = kind == 2
    w = cd.operator((cin, COUT, taps) if transposed else (COUT, cin, taps), 1 if transposed else 0, 5100 + cin + taps)
    bn = cd.bn_data(COUT, 5001) if bias == 'fold' else None
    bias_in = 0.3 * torch.randn(COUT, generator=cd.gen(5200)) if bias == 'bias_in' else None
    hi, lo, oscale, bias_out = cd.split_ref(w, bn, bias_in, transposed)
    assert bool(lo.abs().max() > 0)
    if transposed:
        assert kc == nv.lib().iunet_x2_convT_kc(cin)
        ref = cd.x2_chunked_convT(hi, lo, kc)
    else:
        ref = cd.x2_virtual_conv(hi, lo, kc)
    wo = vec(w, 'w')
    bno = bn_operands(bn) if bn is not None else []
    bio = vec(bias_in, 'bias_in') if bias_in is not None else None
    wv, osc, bo = scratch(ref.numel(), name='wv'), scratch(COUT, name='oscale'), scratch(COUT, name='bias_out')
    nv.call('iunet_x2_prep', nv.ptr(wo.t), nv.ptr(wv.t), nv.ptr(osc.t), nv.ptr(bo.t), *([nv.ptr(o.t) for o in bno] or [None] * 4),
            None if bio is None else nv.ptr(bio.t), cd.EPS, cd.ACT_IN, cd.ACT_OUT, COUT, cin, taps, kind, kc, nv.stream())
    finish([wo] + bno + ([bio] if bio is not None else []), [wv, osc, bo])
    same_bits(wv.logical(), ref, 'virtual operator (hi and lo words)')
    same_bits(osc.logical(), oscale, 'oscale')
    same_bits(bo.logical(), bias_out, 'bias_out')


@pytest.mark.parametrize('nd', [pytest.param(2, id='2d_9taps'), pytest.param(3, id='3d_27taps')])
def test_x2m_prep_read_back(nv, nd):
    cin, taps = 32, 3 ** nd
    w = cd.operator((COUT, cin, taps), 0, 5300 + nd)
    bn = cd.bn_data(COUT, 5001)
    hi, _, oscale, bias_out = cd.split_ref(w, bn, None, 0)
    nbytes = int(nv.lib().iunet_x2m_w8_bytes_nd(nd, COUT, cin))
    assert nbytes > 0
    wo, bno = vec(w, 'w'), bn_operands(bn)
    whi, w8 = scratch(w.numel(), name='whi'), scratch(nbytes, torch.uint8, name='w8')
    osc, bo = scratch(COUT, name='oscale'), scratch(COUT, name='bias_out')
    nv.call('iunet_x2m_prep_nd', nd, nv.ptr(wo.t), nv.ptr(whi.t), nv.ptr(w8.t), nv.ptr(osc.t), nv.ptr(bo.t), *[nv.ptr(o.t) for o in bno], cd.EPS,
            cd.ACT_IN, cd.ACT_OUT, COUT, cin, nv.stream())
    finish([wo] + bno, [whi, w8, osc, bo])
    same_bits(whi.logical(), hi, 'whi')
    same_bits(osc.logical(), oscale, 'oscale')
    same_bits(bo.logical(), bias_out, 'bias_out')


def decoder_pack_ref(which):
    """-> (w, bn, the fp32 operator the entry point must write with NaN where it writes nothing, folded bias, the call's arguments)."""
    cin, nd = 16, 2
    bn = cd.bn_data(COUT, 5001)
    if which == 'lk_kind0':
        w = cd.operator((COUT, cin), 0, 5400)
        wf, bias = fold_ref(w, bn, cd.EPS, 0)
        ref = torch.zeros(COUT, 32)          # K = 16 padded to 32 with zeros
        ref[:, :cin] = wf
    elif which == 'lk_kind2':
        w = cd.operator((cin, COUT, 4 ** nd), 1, 5401)
        wf, bias = fold_ref(w, bn, cd.EPS, 1)
        ref = cd.lk_convT_ref(wf, nd)          # [4][Cout][4 Cin = 64]: no padding
    else:
        cin_tot, ci_off, k_off, ld = 24, 8, 32, 192
        w = cd.operator((COUT, cin_tot, 9), 0, 5402)
        wf, bias = fold_ref(w, bn, cd.EPS, 0)
        ref = torch.full((COUT, ld), float('nan'))
        ref[:, k_off:k_off + 9 * cin] = wf[:, ci_off:ci_off + cin].permute(0, 2, 1).reshape(COUT, -1)          # [co][kidx * Cin + ci]
    return w, bn, ref, bias


@pytest.mark.parametrize('which', ['lk_kind0', 'lk_kind2', 'dl_mode0'])
def test_decoder_pack_fold_read_back(nv, which):
    """The fp32 operators of iunet_lk_pack / iunet_dl_pack element by element, and bias_out: beta - (mean * a), two roundings.  (Before the
    fold was written once, common.h's helper let the compiler fuse the two: bias_out was one unit off on 7 of these 32 channels.)"""
    nd, cin = 2, 16
    w, bn, ref, bias = decoder_pack_ref(which)
    fused = cd.fused_bias(bn, cd.EPS)
    assert int((fused != bias).sum()) > 0
    wo, bno = vec(w, 'w'), bn_operands(bn)
    dst, bo = scratch(ref.numel(), name='dst'), scratch(COUT, name='bias_out')
    bnp = [nv.ptr(o.t) for o in bno]
    if which.startswith('lk'):
        kind = 0 if which == 'lk_kind0' else 2
        assert int(nv.lib().iunet_lk_pack_elems(nd, kind, COUT, cin)) == ref.numel()
        nv.call('iunet_lk_pack', 2, nd, kind, nv.ptr(wo.t), *bnp, cd.EPS, nv.ptr(dst.t), nv.ptr(bo.t), COUT, cin, nv.stream())
    else:
        nv.call('iunet_dl_pack', 2, nd, 0, 3, nv.ptr(wo.t), *bnp, cd.EPS, nv.ptr(dst.t), nv.ptr(bo.t), COUT, cin, 24, 8, 32, 192, nv.stream())
    finish([wo] + bno, [dst, bo])
    got = dst.logical().view(ref.shape)
    skip = torch.isnan(ref)          # columns of a wider row that belong to other operators: still the sentinel
    assert bool((bits(got)[skip] == SENTINEL[F32]).all()), 'a column outside the operator was written'
    same_bits(got[~skip], ref[~skip], 'fp32 operator')
    got_b = bo.logical().reshape(-1)
    print(f'{which}: bias_out differs from the separately rounded fold on {int((bits(got_b) != bits(bias)).sum())} of {COUT} channels, '
          f'from the fused one on {int((bits(got_b) != bits(fused)).sum())}')
    same_bits(got_b, bias, 'bias_out')
