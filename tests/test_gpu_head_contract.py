"""The output contract of the prediction heads (csrc/head_out.h: head_store) across the forms that share it, through the C ABI on
sentinel arenas: iunet_head_fwd (f16, bf16), iunet_f32_head_fwd, iunet_x2_head_fwd and iunet_dl_up_head.  (iunet_x2m_conv_head_fwd is held
to the x2 head bit for bit in tests/test_gpu_x2m.py.)

Data (tests/contract_data.py, which asserts all of this on the reference): N = 2, C0 = 32, features in -2..2, weights multiples of 1/8,
biases multiples of 1/4 -- every logit is exact in fp32 in any summation order, in 16-bit storage of the features and as split words at
act_scale 64 --, and at least 1 % of the voxels tie for the maximum.  Grids: 8 x 40 (320 voxels: two workgroups, the second ragged) and
2 x 8 x 24.  Per form:
  1. the logits have the bits of the CPU reference;
  2. the fp32 and the split-precision head return the same probability bits and the same class map;
  3. so do the f16 and the bf16 head, as each other;
  4. cls is the first maximum of the form's own returned probabilities, and a second call with accumulate = 1, divisor = 3 into the output
     of a first call (accumulate = 0, divisor = 1) gives the bits of fp32 (p + p) / 3 computed on the CPU from the first call's bits;
  5. logits and probabilities are written as class planes of a wider channels-last tensor whose sentinels stay intact.
Needs an MI355X: run with -m gpu."""
import pytest
import torch

from tests import contract_data as cd
from tests.arena import Operand, StridedOutput, bits

pytestmark = pytest.mark.gpu

F32 = torch.float32
FORMS = ('f16', 'bf16', 'f32', 'x2')


@pytest.fixture(scope='module')
def nv():
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    from interactive_unet import _native
    _native.lib()
    return _native


def vec(t, name):
    return Operand(1, t.numel(), t.dtype, 'tight', t.reshape(1, -1), name=name)


def same_bits(got, ref, what):
    assert got.shape == ref.shape and torch.equal(bits(got), bits(ref)), f'{what}: {int((bits(got) != bits(ref)).sum())} of {ref.numel()} elements differ in their bits'


class Outputs:
    """logits and probs as the class planes of wider channels-last tensors (sC = 1, every pitch larger than its extent), cls tight."""

    def __init__(self, N, ncls, grid, want_logits=True):
        vox = grid[0] * grid[1] * grid[2]
        self.logits = StridedOutput((N, ncls) + grid, name='logits') if want_logits else None
        self.probs = StridedOutput((N, ncls) + grid, name='probs')
        self.cls = Operand(N, vox, torch.uint8, 'tight', None, name='cls')
        self.strides = self.probs.strides
        assert self.strides[1] == 1 and self.strides[4] > ncls and (not want_logits or self.logits.strides == self.strides)

    def check(self):
        for o in (self.logits, self.probs, self.cls):
            if o is not None:
                o.check()


def run_contract(call, N, ncls, grid, want_logits=True):
    """call(outs, divisor, accumulate) launches the head.  First call: plain; second: accumulate = 1, divisor = 3 into the first one's
    probabilities.  Asserts 4. and 5.; -> (logits or None, first-call probabilities, class map)."""
    o = Outputs(N, ncls, grid, want_logits)
    call(o, 1.0, 0)
    torch.cuda.synchronize()
    o.check()
    P, cls = o.probs.logical(), o.cls.logical().view((N,) + grid)
    logits = o.logits.logical() if want_logits else None
    assert not bool(torch.isnan(P).any()) and (logits is None or not bool(torch.isnan(logits).any())), 'an output element was never written'
    assert torch.equal(cls.long(), cd.first_max(P)), f'cls is not the first maximum of the returned probabilities at {int((cls.long() != cd.first_max(P)).sum())} voxels'
    call(o, 3.0, 1)
    torch.cuda.synchronize()
    o.check()
    same_bits(o.probs.logical(), (P + P) / 3, 'accumulate = 1, divisor = 3 on top of the first call')
    assert torch.equal(o.cls.logical().view((N,) + grid), cls)
    if logits is not None:
        same_bits(o.logits.logical(), logits, 'logits of the second call')
    return logits, P, cls


def feature_call(nv, form, ncls, grid, x, w, b):
    N, C0 = cd.HEAD_N, cd.HEAD_C0
    D, H, W = grid
    wo, bo = vec(w, 'w'), vec(b, 'bias')
    if form in ('f16', 'bf16'):
        dt = torch.float16 if form == 'f16' else torch.bfloat16
        xo = Operand(N, C0 * D * H * W, dt, 'gap', cd.nhwc8(x, dt), name='x')
    elif form == 'f32':
        xo = Operand(N, C0 * D * H * W, F32, 'gap', x.reshape(N, -1), name='x')
    else:
        xo = Operand(N, 2 * C0 * D * H * W, torch.float16, 'gap', cd.split_words(x), name='x')

    def call(o, divisor, accumulate):
        outs = (nv.ptr(o.logits.t), nv.ptr(o.probs.t), nv.ptr(o.cls.t), nv.ll_array(o.strides), float(divisor), accumulate, N, D, H, W, nv.stream())
        if form in ('f16', 'bf16'):
            nv.call('iunet_head_fwd', 0 if form == 'f16' else 1, nv.ptr(xo.t), xo.ss, C0, nv.ptr(wo.t), nv.ptr(bo.t), ncls, *outs)
        elif form == 'f32':
            nv.call('iunet_f32_head_fwd', nv.ptr(xo.t), xo.ss, C0, nv.ptr(wo.t), nv.ptr(bo.t), ncls, *outs)
        else:
            nv.call('iunet_x2_head_fwd', nv.ptr(xo.t), xo.ss, C0 // 8, C0, nv.ptr(wo.t), nv.ptr(bo.t), cd.ACT_SCALE, ncls, *outs)
    return call, (xo, wo, bo)


@pytest.mark.parametrize('gk', list(cd.HEAD_GRIDS))
@pytest.mark.parametrize('ncls', cd.HEAD_NCLS)
def test_head_output_contract_across_forms(nv, ncls, gk):
    grid = cd.HEAD_GRIDS[gk]
    x, w, b, logits_ref, cls_ref, ties = cd.head_data(ncls, gk)
    assert ties >= 0.01 and (grid[0] * grid[1] * grid[2]) % 256 and grid[0] * grid[1] * grid[2] > 256
    res = {}
    for form in FORMS:
        call, inputs = feature_call(nv, form, ncls, grid, x, w, b)
        logits, P, cls = run_contract(call, cd.HEAD_N, ncls, grid)
        for o in inputs:
            o.check()
        same_bits(logits, logits_ref, f'{form}: logits against the CPU reference')          # 1.
        res[form] = (P, cls)
    same_bits(res['x2'][0], res['f32'][0], 'probabilities, split-precision head against the fp32 head')          # 2.
    assert torch.equal(res['x2'][1], res['f32'][1]), 'class map, split-precision head against the fp32 head'
    same_bits(res['bf16'][0], res['f16'][0], 'probabilities, bf16 head against the f16 head')          # 3.
    assert torch.equal(res['bf16'][1], res['f16'][1]), 'class map, bf16 head against the f16 head'
    # (where the logits tie the probabilities tie, in every form: the class map there is the reference's first maximum)
    tie = (logits_ref == logits_ref.max(1, keepdim=True).values).sum(1) > 1
    for form in FORMS:
        assert torch.equal(res[form][1][tie].int(), cls_ref[tie].int()), f'{form}: class at the tied voxels'


@pytest.mark.parametrize('nd,coarse,s,ncls', [pytest.param(*r, id=f'{r[0]}d-coarse{"x".join(map(str, r[1]))}-s{r[2]}-ncls{r[3]}') for r in cd.UP_SHAPES])
def test_upsampling_head_output_contract(nv, nd, coarse, s, ncls):
    lc = cd.up_data(nd, coarse, s, ncls)
    c3 = coarse if nd == 3 else (1,) + coarse
    grid = tuple(c * s for c in coarse) if nd == 3 else (1,) + tuple(c * s for c in coarse)
    lo = Operand(1, lc.numel(), F32, 'tight', lc.reshape(1, -1), name='coarse logits')

    def call(o, divisor, accumulate):
        nv.call('iunet_dl_up_head', nd, nv.ptr(lo.t), ncls, *c3, s, nv.ptr(o.logits.t), nv.ptr(o.probs.t), nv.ptr(o.cls.t), nv.ll_array(o.strides),
                float(divisor), accumulate, cd.HEAD_N, nv.stream())

    run_contract(call, cd.HEAD_N, ncls, grid)
    lo.check()
