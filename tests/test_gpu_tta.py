"""The symmetry ensemble on the device: iunet_sym_block and iunet_sym_accumulate bit for bit against the definition
tests/tta_ref.py, and the host layer on top of them -- predict_volume_array(tta=, return_spread=), predict_slab(tta=) -- against the same
composition written here from existing pieces only.  Every comparison is exact."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import tta_ref as tr
from tests.volume_inputs import random_slicer

TRANSPOSING = tuple(8 * pi + f for pi in (1, 3, 4, 5) for f in range(8))
# ragged tiles / a degenerate axis and a row longer than a tile (the issue's three); rows of whole 16-byte chunks (the wide row copy)
BLOCK_SHAPES = ((8, 16, 24), (5, 7, 67), (1, 1, 130), (6, 10, 48))
ACC_SHAPES = ((8, 16, 24), (5, 7, 67))


def _bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _sym_block(xd, sym, out=None):
    from interactive_unet import _native as nv
    D, H, W = xd.shape
    if out is None:
        out = torch.empty(tr.shape(xd.shape, sym), dtype=torch.uint8, device='cuda')
    nv.call('iunet_sym_block', nv.ptr(xd), D, H, W, sym, nv.ptr(out), nv.stream())
    return out


@pytest.mark.parametrize('n', BLOCK_SHAPES)
def test_sym_block_is_the_restatement(n):
    x = _bytes(n, 1)
    xd = torch.tensor(x).cuda()
    got = [_sym_block(xd, sym) for sym in range(48)]
    again = [_sym_block(xd, sym) for sym in range(48)]
    for sym in range(48):
        assert got[sym].shape == tr.shape(n, sym)
        assert np.array_equal(got[sym].cpu().numpy(), tr.forward(x, sym)), (n, sym)
        assert torch.equal(got[sym], again[sym]), (n, sym)


def test_sym_block_walks_several_ragged_tiles():
    n = (33, 65, 70)
    x = _bytes(n, 2)
    xd = torch.tensor(x).cuda()
    for sym in TRANSPOSING:
        assert np.array_equal(_sym_block(xd, sym).cpu().numpy(), tr.forward(x, sym)), sym


@pytest.mark.parametrize('n', ((6, 10, 48), (5, 7, 67)))
def test_sym_block_on_buffers_at_odd_addresses(n):
    x = _bytes(n, 3)
    vox = int(np.prod(n))
    src = torch.zeros(vox + 17, dtype=torch.uint8, device='cuda')
    for off_in, off_out in ((1, 1), (1, 0), (0, 3), (16, 16)):
        xin = src[off_in:off_in + vox].view(n)
        xin.copy_(torch.tensor(x))
        assert xin.data_ptr() % 16 == off_in % 16
        for sym in (0, 4, 7, 16 + 5, 8, 24 + 6, 47):
            dst = torch.full((vox + 32,), 0xa5, dtype=torch.uint8, device='cuda')
            out = dst[off_out:off_out + vox].view(tr.shape(n, sym))
            _sym_block(xin, sym, out=out)
            assert np.array_equal(out.cpu().numpy(), tr.forward(x, sym)), (n, off_in, off_out, sym)
            rest = torch.cat([dst[:off_out], dst[off_out + vox:]])
            assert bool((rest == 0xa5).all()), (n, off_in, off_out, sym)          # nothing written beside the block


# ---- iunet_sym_accumulate
def _members(name):
    if name == 'shuffled':
        return tuple(int(s) for s in np.random.default_rng(7).permutation(48)[:5])
    return tr.SETS[name]


class _Scratch:
    """sum / mn / mx / mean / spread of one block, pre-filled with NaN: index 0 must ignore what it finds."""

    def __init__(self, n, C, trio=True, alias=False, offset=0):
        nan = lambda *shape: torch.full((int(np.prod(shape)) + offset,), float('nan'), dtype=torch.float32, device='cuda')[offset:].view(shape)
        self.n, self.C = n, C
        self.sum = nan(*n, C)
        self.mn, self.mx, self.spread = (nan(*n, C), nan(*n, C), nan(*n)) if trio else (None, None, None)
        self.mean = self.sum if alias else nan(*n, C)

    def add(self, qd, sym, index, count):
        from interactive_unet import _native as nv
        inv = float(np.float32(1) / np.float32(count))
        nv.call('iunet_sym_accumulate', nv.ptr(qd), self.n[0], self.n[1], self.n[2], self.C, sym, index, count, inv, nv.ptr(self.sum),
                nv.ptr(self.mn), nv.ptr(self.mx), nv.ptr(self.mean), nv.ptr(self.spread), nv.stream())


def _member_outputs(n, C, syms, seed):
    rng = np.random.default_rng(seed)
    return [rng.random(tr.shape(n, sym) + (C,), dtype=np.float32) for sym in syms]


def _check_every_step(n, C, syms, seed=11, offset=0):
    qs = _member_outputs(n, C, syms, seed)
    steps = tr.ensemble_steps(qs, syms)
    mean, spread = tr.ensemble(qs, syms)
    sc = _Scratch(n, C, offset=offset)
    snaps = []
    for k, sym in enumerate(syms):
        qd = torch.tensor(qs[k]).cuda()
        if offset:
            qd = torch.cat([torch.zeros(offset, device='cuda'), qd.reshape(-1)])[offset:].view(qs[k].shape)
        sc.add(qd, sym, k, len(syms))
        snaps.append((sc.sum.clone(), sc.mn.clone(), sc.mx.clone()))
    for k, (snap, want) in enumerate(zip(snaps, steps)):
        for name, g, w in zip(('sum', 'mn', 'mx'), snap, want):
            assert np.array_equal(g.cpu().numpy(), w), (n, C, syms[k], k, name)
    assert np.array_equal(sc.mean.cpu().numpy(), mean) and np.array_equal(sc.spread.cpu().numpy(), spread), (n, C)
    return qs, mean, spread


@pytest.mark.parametrize('name', ('flips', 'full', 'shuffled'))
@pytest.mark.parametrize('C', (1, 2, 4, 5, 16))
@pytest.mark.parametrize('n', ACC_SHAPES)
def test_sym_accumulate_is_the_restatement(n, C, name):
    _check_every_step(n, C, _members(name))


@pytest.mark.parametrize('C', (2, 16))
def test_sym_accumulate_walks_several_ragged_tiles(C):
    """37 > the widest tile along the transposed axis (32 voxels), 70 > the tile along W (64)."""
    _check_every_step((3, 37, 70), C, TRANSPOSING)
    _check_every_step((37, 3, 70), C, TRANSPOSING[::3])


def test_sym_accumulate_on_buffers_aligned_to_four_bytes_only():
    """C = 2 and 4 take one access per voxel where every buffer is aligned to it, C scalar accesses otherwise: the same bits."""
    for C in (2, 4):
        _check_every_step((5, 7, 67), C, (0, 5, 10, 29, 43), offset=1)


def test_sym_accumulate_modes():
    n, C, syms = (5, 7, 67), 2, (0, 44, 6, 19, 33)
    qs = _member_outputs(n, C, syms, 5)
    mean, spread = tr.ensemble(qs, syms)
    qd = [torch.tensor(q).cuda() for q in qs]
    # the mean only (no mn / mx / spread), and mean written over sum
    for trio, alias in ((False, False), (False, True), (True, True)):
        sc = _Scratch(n, C, trio=trio, alias=alias)
        for k, sym in enumerate(syms):
            sc.add(qd[k], sym, k, len(syms))
        assert np.array_equal(sc.mean.cpu().numpy(), mean), (trio, alias)
        if trio:
            assert np.array_equal(sc.spread.cpu().numpy(), spread)
    # a repeated ensemble on used scratch: the same bits
    sc = _Scratch(n, C)
    for rep in range(2):
        for k, sym in enumerate(syms):
            sc.add(qd[k], sym, k, len(syms))
        assert np.array_equal(sc.mean.cpu().numpy(), mean) and np.array_equal(sc.spread.cpu().numpy(), spread)
    # one member: the member itself, spread 0
    for sym in (0, 29):
        q = _member_outputs(n, C, (sym,), 6)[0]
        sc = _Scratch(n, C)
        sc.add(torch.tensor(q).cuda(), sym, 0, 1)
        assert np.array_equal(sc.mean.cpu().numpy(), tr.inverse(q, sym)) and np.array_equal(sc.sum.cpu().numpy(), tr.inverse(q, sym))
        assert not sc.spread.cpu().numpy().any()
    # before the last call mean and spread are untouched
    sc = _Scratch(n, C)
    sc.add(qd[0], syms[0], 0, 3)
    sc.add(qd[1], syms[1], 1, 3)
    assert bool(torch.isnan(sc.mean).all()) and bool(torch.isnan(sc.spread).all())


# ---- end to end with the 3-D net ------------------------------------------------------------------------------------------
VSHAPE = (40, 48, 56)


@pytest.fixture(scope='module')
def model():
    from interactive_unet.unet import UNet
    from oracle import unet_ref
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = UNet(dim=3, levels=4, base=32, infer_dtype='fp16', pretrained=False)
    m.load_named(unet_ref.init_params(dim=3, levels=4, base=32, seed=3, randomize_bn=True))
    return m.cuda().eval()


@pytest.fixture(scope='module')
def volume():
    return np.random.default_rng(4).integers(1, 256, VSHAPE, dtype=np.uint8)


def _forward(eng, blocks):
    """The engine's forward on a list of equally shaped uint8 [D, H, W] host blocks as ONE batch -> fp32 [D, H, W, C] host arrays."""
    D, H, W = blocks[0].shape
    C, vox, nb = eng.ncls, D * H * W, len(blocks)
    x = torch.tensor(np.stack(blocks)).cuda()
    probs = torch.empty((nb, D, H, W, C), dtype=torch.float32, device='cuda')
    eng.infer(x, (vox, vox, H * W, W, 1), nb, D, H, W, probs=probs, out_strides=(vox * C, 1, H * W * C, W * C, C))
    return [p for p in probs.cpu().numpy()]


def _ensemble_of(eng, block, syms, batch):
    """tta_ref's ensemble over the engine's forwards of the transformed bytes, `batch` members of one shape per forward."""
    qs, k = [], 0
    while k < len(syms):
        nb = 1
        while nb < batch and k + nb < len(syms) and tr.shape(block.shape, syms[k + nb]) == tr.shape(block.shape, syms[k]):
            nb += 1
        qs += _forward(eng, [tr.forward(block, s) for s in syms[k:k + nb]])
        k += nb
    return tr.ensemble(qs, syms)


def test_the_identity_member_is_the_plain_prediction(model, volume):
    from interactive_unet import predict
    plain = predict.predict_volume_array(model, volume, input_size=32)
    assert plain.shape == VSHAPE + (2,) and plain.dtype == torch.uint8
    assert len(torch.unique(plain)) > 16                                          # a prediction, not a constant
    assert torch.equal(predict.predict_volume_array(model, volume, input_size=32, tta=[0]), plain)
    assert torch.equal(predict.predict_volume_array(model, volume, input_size=32, tta=None), plain)


@pytest.fixture(scope='module')
def flips(model, volume):
    from interactive_unet import predict
    return predict.predict_volume_array(model, volume, input_size=32, tta='flips', return_spread=True)


def test_the_flips_ensemble_is_the_composition_of_existing_pieces(model, volume, flips):
    from interactive_unet import predict
    pred, spread_u8 = flips
    assert pred.shape == VSHAPE + (2,) and pred.dtype == torch.uint8 and spread_u8.shape == VSHAPE and spread_u8.dtype == torch.uint8
    S, C, syms, eng = 32, 2, tr.SETS['flips'], model.engine('eval')
    vd = torch.tensor(volume).cuda()
    bc, pbc, lbc = predict.get_block_coordinates(np.array(VSHAPE), input_size=S, overlap=0.25)
    assert len(bc) == 8
    acc = predict.VolumeAccumulator(VSHAPE, C, S, vd.device)
    acc_s = predict.VolumeAccumulator(VSHAPE, 1, S, vd.device)
    for i in range(len(bc)):
        block = predict.gather_block(vd, pbc[i], S).cpu().numpy()
        mean, spread = _ensemble_of(eng, block, syms, predict.BLOCK_BATCH)
        acc.blend(bc[i], lbc[i], probs=torch.tensor(mean).cuda())
        acc_s.blend(bc[i], lbc[i], probs=torch.tensor(spread[..., None]).cuda())
    assert torch.equal(pred, acc.finalize())
    assert torch.equal(spread_u8, acc_s.finalize()[..., 0])
    assert spread_u8.max().item() > 0                                             # the members do disagree somewhere
    # the ensemble is not the plain prediction, and a second run gives the same bytes
    assert not torch.equal(pred, predict.predict_volume_array(model, volume, input_size=32))
    # block_range / accumulator / finalize keep working, and reset() zeroes the spread accumulators too
    a = predict.predict_volume_array(model, volume, input_size=32, tta='flips', return_spread=True, block_range=(0, 3), finalize=False)
    assert a.spread_pred is not None and a.spread_weight.max().item() > 0
    a.reset()
    assert a.spread_pred.max().item() == 0 and a.spread_weight.max().item() == 0 and a.weight.max().item() == 0
    for lo, hi in ((0, 3), (3, 8)):
        predict.predict_volume_array(model, volume, input_size=32, tta='flips', return_spread=True, block_range=(lo, hi), accumulator=a, finalize=False)
    assert torch.equal(a.finalize(), pred) and torch.equal(a.finalize_spread(), spread_u8)


def test_score_planes_reads_the_spread_volume(flips):
    from interactive_unet import propose
    _, spread_u8 = flips
    E = np.eye(3)
    c = np.array(VSHAPE, dtype=np.float64) / 2
    planes = np.array([[E[1], E[2], c], [E[0], E[2], c + 0.5], [E[0], (E[1] + E[2]) / np.sqrt(2), c]])
    got = propose.score_planes(spread_u8, planes, 32)
    want = propose.score_planes(spread_u8.cpu().numpy(), planes, 32)
    assert np.array_equal(got.cpu().numpy(), want) and want[:, 0].min() > 0


@pytest.mark.parametrize('spec', ('planar', (0, 8 * 3 + 2, 8 * 4 + 5, 8 * 5)))
def test_predict_slab_ensemble(model, volume, spec):
    """'planar' keeps the slab's shape; pi = 3, 4, 5 turn the (16, 32, 32) slab into (32, 32, 16) / (32, 16, 32)."""
    from interactive_unet import predict, tta
    vd = torch.tensor(volume).cuda()
    s = random_slicer(VSHAPE, 6)
    T, S = 16, 32
    slab, cls, probs = predict.predict_slab(model, vd, s, slice_width=S, depth=T, tta=spec)
    assert torch.equal(slab, s.get_slab(vd, axis=0, slice_width=S, depth=T, order=1))
    assert cls.shape == (T, S, S) and cls.dtype == torch.uint8 and probs.shape == (T, S, S, 2) and probs.dtype == torch.float32
    syms = tta.members(spec)
    if spec != 'planar':
        assert {tr.shape((T, S, S), m) for m in syms} == {(16, 32, 32), (32, 32, 16), (32, 16, 32)}
    mean, _ = _ensemble_of(model.engine('eval'), slab.cpu().numpy(), syms, 1)
    assert np.array_equal(probs.cpu().numpy(), mean)
    assert np.array_equal(cls.cpu().numpy(), np.argmax(mean, axis=-1))           # numpy: the first maximum
    assert len(np.unique(cls.cpu().numpy())) == 2
    # predict_slice_3d passes tta through: the centre plane's probabilities
    pr = predict.predict_slice_3d(vd, s, slice_width=S, depth=T, return_probabilities=True, model=model, tta=spec)
    assert np.array_equal(pr[0], mean[T // 2])
