"""Nearest-seed feature transform and instance labels on the device: iunet_edt_feature, iunet_edt_feature_mask,
iunet_edt_assign and iunet_label_remap bit for bit against the definition tests/instances_ref.py (single seeds against the closed form), and
the host layer interactive_unet/instances.py end to end -- on random, sparse, tie-heavy, planted and degenerate volumes and on a real
prediction of the 3-D net.  Every comparison is exact equality; every output starts from a pattern, so an element left unwritten shows."""
import functools
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import instances_ref as ir
from tests.test_instances_cpu import grains, label_map, planted_leak, planted_split
from tests.test_morphology_cpu import sparse_input
from tests.volume_inputs import offset_copy, random_pred

# ragged; a row; flat; one voxel; one axis longer than any workgroup, in turn along the row and along either column
SHAPES = {'ragged': (37, 41, 150), 'row': (1, 1, 300), 'flat': (33, 2, 65), 'one voxel': (1, 1, 1), 'long x': (3, 5, 2100),
          'long y': (3, 2100, 5), 'long z': (2100, 3, 5)}
SHAPE_NAMES = tuple(SHAPES)
KINDS = ('p50', 'p01', 'none', 'all', 'plane', 'lattice')
MAX_SQ = 2 ** 31 - 2


@functools.lru_cache(maxsize=None)
def _volume(kind, name):
    shape = SHAPES[name]
    seed = SHAPE_NAMES.index(name)
    if kind == 'p50':
        v = (np.random.default_rng(seed).random(shape) < 0.5).astype(np.uint8)
    elif kind == 'p01':
        v = (np.random.default_rng(10 + seed).random(shape) < 0.01).astype(np.uint8)
    elif kind == 'sparse':
        assert shape == (37, 41, 150)
        v = sparse_input().astype(np.uint8)
    elif kind == 'none':
        v = np.zeros(shape, np.uint8)
    elif kind == 'all':
        v = np.ones(shape, np.uint8)
    elif kind == 'plane':
        v = np.zeros(shape, np.uint8)
        v[0] = 1
    elif kind == 'lattice':                                # ties along every axis
        z, y, x = np.indices(shape)
        v = ((z % 4 == 0) & (y % 3 == 0) & (x % 5 == 0)).astype(np.uint8)
    elif kind == 'grains':
        v = grains(shape, 20 + seed)
    else:
        v = random_pred(shape, int(kind), 30 + seed)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _want_of(kind, name, target, invert):
    d2, idx = ir.feature(_volume(kind, name), target, invert)
    d2.setflags(write=False)
    idx.setflags(write=False)
    return d2, idx


def _want(kind, name, target, invert):
    """The definition's (d2, idx), computed once and shared.  A map of zeros and ones has two seed sets only: the ones and the zeros."""
    if _volume(kind, name).ndim == 3 and kind != 'grains' and target in (0, 1):
        return _want_of(kind, name, 1, (target == 1) == bool(invert))
    return _want_of(kind, name, target, bool(invert))


def _ws(Z, Y, X):
    from interactive_unet import _native as nv
    ws_bytes = nv.lib().iunet_edt_feature_ws_bytes(Z, Y, X)
    assert ws_bytes == (8 * Z * Y * X + 15) // 16 * 16 + (4 * Z * Y * X + 15) // 16 * 16
    return torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device='cuda'), ws_bytes


def _feat(srcd, target, invert, want_cls=True):
    """The entry point itself."""
    from interactive_unet import _native as nv
    Z, Y, X = srcd.shape[:3]
    C = 1 if srcd.ndim == 3 else srcd.shape[3]
    d2 = torch.full((Z, Y, X), -7, dtype=torch.int32, device='cuda')
    idx = torch.full((Z, Y, X), -9, dtype=torch.int32, device='cuda')
    cls = torch.full((Z, Y, X), 77, dtype=torch.uint8, device='cuda') if want_cls else None
    ws, ws_bytes = _ws(Z, Y, X)
    nv.call('iunet_edt_feature', nv.ptr(srcd), Z, Y, X, C, target, int(invert), nv.ptr(d2), nv.ptr(idx), nv.ptr(cls), nv.ptr(ws), ws_bytes,
            nv.stream())
    return d2, idx, cls


def _fmask(prevd, r2, above):
    from interactive_unet import _native as nv
    Z, Y, X = prevd.shape
    d2 = torch.full((Z, Y, X), -7, dtype=torch.int32, device='cuda')
    idx = torch.full((Z, Y, X), -9, dtype=torch.int32, device='cuda')
    ws, ws_bytes = _ws(Z, Y, X)
    nv.call('iunet_edt_feature_mask', nv.ptr(prevd), Z, Y, X, r2, int(above), nv.ptr(d2), nv.ptr(idx), nv.ptr(ws), ws_bytes, nv.stream())
    return d2, idx


def _assign(idxd, d2d, seedd, r2, group=None, offset=0, out=None):
    from interactive_unet import _native as nv
    Z, Y, X = idxd.shape
    out = torch.full((Z, Y, X), 55, dtype=torch.int32, device='cuda') if out is None else out
    nv.call('iunet_edt_assign', nv.ptr(idxd), nv.ptr(d2d), nv.ptr(seedd), nv.ptr(group), offset, Z, Y, X, r2, nv.ptr(out), nv.stream())
    return out


def _remap(labelsd, K, tabled):
    from interactive_unet import _native as nv
    Z, Y, X = labelsd.shape
    nv.call('iunet_label_remap', nv.ptr(labelsd), Z, Y, X, K, nv.ptr(tabled), nv.stream())
    return labelsd


def _same(got, want, where):
    assert np.array_equal(got[0].cpu().numpy(), want[0]), ('d2', where)
    assert np.array_equal(got[1].cpu().numpy(), want[1]), ('idx', where)


def _check(kind, name, target, invert, want_cls=True):
    v = _volume(kind, name)
    srcd = torch.tensor(v).cuda()
    d2, idx, cls = _feat(srcd, target, invert, want_cls)
    _same((d2, idx), _want(kind, name, target, invert), (kind, name, target, invert))
    if want_cls:
        assert np.array_equal(cls.cpu().numpy(), ir.class_map(v)[0]), (kind, name)
    else:
        assert cls is None
    return srcd, d2, idx


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', SHAPE_NAMES)
def test_class_maps(name, kind):
    for target in (0, 1):
        for invert in (False, True):
            _check(kind, name, target, invert, want_cls=(target == 1) != invert)     # cls asked and not


def test_the_sparse_volume():
    """108 seeds in 37 x 41 x 150: rows and a whole plane without a seed (tests/test_morphology_cpu.py shows it has them)."""
    _, d2, idx = _check('sparse', 'ragged', 1, False)
    assert int(d2.max()) > 100 and int(idx.min()) >= 0
    _check('sparse', 'ragged', 1, True)
    _check('sparse', 'ragged', 0, True, want_cls=False)


@pytest.mark.parametrize('name', SHAPE_NAMES)
def test_one_seed_against_the_closed_form(name):
    shape = SHAPES[name]
    z, y, x = np.indices(shape)
    for at in ((0, 0, 0), tuple(n - 1 for n in shape)):
        v = np.zeros(shape, np.uint8)
        v[at] = 3
        want = ((z - at[0]) ** 2 + (y - at[1]) ** 2 + (x - at[2]) ** 2).astype(np.int32)
        d2, idx, cls = _feat(torch.tensor(v).cuda(), 3, False)
        assert np.array_equal(d2.cpu().numpy(), want) and np.array_equal(cls.cpu().numpy(), v), (name, at)
        assert bool((idx == int(np.ravel_multi_index(at, shape))).all()), (name, at)


def test_long_distances_from_one_seed_in_the_last_voxel():
    shape = (2, 2, 16384)
    v = np.zeros(shape, np.uint8)
    v[-1, -1, -1] = 1
    z, y, x = np.indices(shape)
    want = ((z - 1) ** 2 + (y - 1) ** 2 + (x - 16383) ** 2).astype(np.int32)
    d2, idx, _ = _feat(torch.tensor(v).cuda(), 1, False, want_cls=False)
    assert np.array_equal(d2.cpu().numpy(), want) and bool((idx == 4 * 16384 - 1).all())


@pytest.mark.parametrize('C', (2, 5))
@pytest.mark.parametrize('name', ('ragged', 'flat', 'long y', 'one voxel'))
def test_predicted_volumes(name, C):
    for target in (0, 1):
        for invert in (False, True):
            _check(str(C), name, target, invert, want_cls=not invert)


@pytest.mark.parametrize('kind,name', (('p50', 'ragged'), ('lattice', 'flat'), ('5', 'ragged'), ('p01', 'long z'), ('none', 'row')))
def test_the_distances_are_those_of_the_plain_transform(kind, name):
    from interactive_unet import _native as nv
    srcd = torch.tensor(_volume(kind, name)).cuda()
    Z, Y, X = srcd.shape[:3]
    for invert in (False, True):
        d2, _, cls = _feat(srcd, 1, invert)
        plain = torch.full((Z, Y, X), -7, dtype=torch.int32, device='cuda')
        pcls = torch.full((Z, Y, X), 77, dtype=torch.uint8, device='cuda')
        ws_bytes = nv.lib().iunet_edt_ws_bytes(Z, Y, X)
        ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device='cuda')
        nv.call('iunet_edt_sq', nv.ptr(srcd), Z, Y, X, 1 if srcd.ndim == 3 else srcd.shape[3], 1, int(invert), nv.ptr(plain), nv.ptr(pcls), nv.ptr(ws),
                ws_bytes, nv.stream())
        assert torch.equal(d2, plain) and torch.equal(cls, pcls), (kind, name, invert)


@functools.lru_cache(maxsize=None)
def _distance_map(name):
    """The distance of the grains' class 1 to its outside: the map split_touching thresholds."""
    d = ir.feature(_volume('grains', name), 1, True)[0]
    d.setflags(write=False)
    return d


@pytest.mark.parametrize('above', (False, True))
@pytest.mark.parametrize('name', ('ragged', 'flat', 'long z'))
def test_seeds_from_a_map(name, above):
    prev = _distance_map(name)
    prevd = torch.tensor(prev).cuda()
    for r2 in (0, 4, 9, MAX_SQ):
        _same(_fmask(prevd, r2, above), ir.feature_mask(prev, r2, above), (name, r2, above))
    assert np.array_equal(prevd.cpu().numpy(), prev)
    d2, idx = _fmask(torch.full_like(prevd, ir.INF), MAX_SQ, above)           # INF > every r2: all seeds above, none below
    if above:
        assert not d2.any() and torch.equal(idx.reshape(-1), torch.arange(prev.size, dtype=torch.int32, device='cuda'))
    else:
        assert bool((d2 == ir.INF).all()) and bool((idx == -1).all())


@functools.lru_cache(maxsize=None)
def _assign_case(shape):
    """(idx, d2, seed_labels, group) on the host: seeds with labels 1 .. 6, a group map with zeros that cuts across the cells."""
    rng = np.random.default_rng(int(np.prod(shape)))
    s = rng.random(shape) < (0.4 if np.prod(shape) < 10 else 0.02)
    s.reshape(-1)[0] = True
    d2, idx = ir.feature_of(s)
    seed_labels = np.where(s, rng.integers(1, 7, shape), 0).astype(np.int32)
    group = (rng.integers(0, 3, [max(1, (n + 6) // 7) for n in shape]).repeat(7, 0).repeat(7, 1).repeat(7, 2)[:shape[0], :shape[1], :shape[2]]).astype(np.int32)
    return idx, d2, seed_labels, np.ascontiguousarray(group)


@pytest.mark.parametrize('shape', ((37, 41, 150), (1, 1, 3), (1, 5, 821), (1, 1, 1)))
def test_assign(shape):
    idx, d2, seed_labels, group = _assign_case(shape)
    assert (group == 0).any() or np.prod(shape) < 10
    dev = [torch.tensor(a).cuda() for a in (idx, d2, seed_labels, group)]
    narrow = [offset_copy(t, 4) for t in dev]                                  # 4 bytes off 16: the one-voxel path
    assert all(t.data_ptr() % 16 == 0 for t in dev)
    for r2 in (0, 9, MAX_SQ):
        for g, offset in ((None, 0), (3, 0), (3, 1000)):
            want = ir.assign(idx, d2, seed_labels, r2, group=None if g is None else group, offset=offset)
            for i, d, s, gr in (dev, narrow):
                got = _assign(i, d, s, r2, group=None if g is None else gr, offset=offset)
                assert np.array_equal(got.cpu().numpy(), want), (shape, r2, g, offset)
            out = offset_copy(torch.full(shape, 55, dtype=torch.int32, device='cuda'), 8)
            got = _assign(dev[0], dev[1], dev[2], r2, group=None if g is None else dev[3], offset=offset, out=out)
            assert got is out and np.array_equal(out.cpu().numpy(), want), (shape, r2, g, offset)
    if np.prod(shape) > 10:
        assert (ir.assign(idx, d2, seed_labels, 9, group=group, offset=1000) >= 1000).any() and (ir.assign(idx, d2, seed_labels, 9) == 0).any()
    none = torch.full(shape, -1, dtype=torch.int32, device='cuda')             # no seed at all
    inf = torch.full(shape, ir.INF, dtype=torch.int32, device='cuda')
    assert not _assign(none, inf, dev[2], MAX_SQ).any()
    assert np.array_equal(_assign(none, inf, dev[2], MAX_SQ, group=dev[3], offset=7).cpu().numpy(), np.where(group > 0, 7 + group, 0))
    assert not _assign(none, dev[1], dev[2], MAX_SQ).any()                     # idx decides, whatever d2 holds
    in_place = dev[1].clone()                                                  # out may be d2
    assert np.array_equal(_assign(dev[0], in_place, dev[2], 9, out=in_place).cpu().numpy(), ir.assign(idx, d2, seed_labels, 9))


@pytest.mark.parametrize('shape', ((37, 41, 150), (1, 1, 3), (1, 5, 821), (1, 1, 1)))
def test_remap(shape):
    rng = np.random.default_rng(5)
    K = 40
    lab = rng.integers(0, K + 1, shape).astype(np.int32)
    lab.reshape(-1)[::11] = K + 5                                              # outside 0 .. K: left as they are
    lab.reshape(-1)[::13] = -2
    for table in (np.arange(K + 1), np.concatenate([[0], 1 + rng.permutation(K)]), np.zeros(K + 1)):
        table = table.astype(np.int32)
        want = ir.remap(lab, table)
        for labd in (torch.tensor(lab).cuda(), offset_copy(torch.tensor(lab).cuda(), 4)):
            assert _remap(labd, K, torch.tensor(table).cuda()) is labd and np.array_equal(labd.cpu().numpy(), want), shape
    assert np.array_equal(ir.remap(lab, np.arange(K + 1)), lab)
    zero = torch.zeros(shape, dtype=torch.int32, device='cuda')
    assert bool((_remap(zero, 0, torch.tensor([9], dtype=torch.int32).cuda()) == 9).all())


def test_repeated_launches_and_a_second_stream_give_the_same_bytes():
    for kind, name in (('p50', 'ragged'), ('5', 'ragged'), ('lattice', 'long y')):
        srcd = torch.tensor(_volume(kind, name)).cuda()
        a = _feat(srcd, 1, False)
        b = _feat(srcd, 1, False)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        ma, mb = _fmask(a[0], 4, True), _fmask(b[0], 4, True)
        assert torch.equal(ma[0], mb[0]) and torch.equal(ma[1], mb[1])
        seed = (a[0] == 0).to(torch.int32) * 3
        oa = _assign(a[1], a[0], seed, 9, group=seed + 1, offset=2)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            c = _feat(srcd, 1, False)
            mc = _fmask(c[0], 4, True)
            oc = _assign(c[1], c[0], seed, 9, group=seed + 1, offset=2)
        side.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(a, c)) and torch.equal(ma[0], mc[0]) and torch.equal(ma[1], mc[1]) and torch.equal(oa, oc)


def test_nearest_and_expand_labels_on_resident_volumes():
    from interactive_unet import instances
    for kind, name, targets in (('grains', 'ragged', (1, 2)), ('2', 'flat', (0, 1)), ('5', 'ragged', (0, 3)), ('all', 'one voxel', (0, 1))):
        v = _volume(kind, name)
        vd = torch.tensor(v).cuda()
        for target in targets:
            for invert in (False, True):
                got = instances.nearest(vd, target, invert)
                assert got[0].is_cuda and got[0].dtype == torch.int32 and got[1].dtype == torch.int32
                _same(got, _want(kind, name, target, invert), (kind, name, target, invert))
        assert np.array_equal(vd.cpu().numpy(), v)                             # the input is left alone
    for shape, seed, p in (((37, 41, 150), 0, 0.002), ((1, 1, 300), 1, 0.05), ((33, 2, 65), 2, 0.0), ((1, 1, 1), 3, 1.0)):
        lab = label_map(shape, seed, p)
        labd = torch.tensor(lab).cuda()
        _same(instances.nearest_labelled(labd), ir.feature_of(lab > 0), shape)
        for distance in (0, 1, 1.5, 3):
            got = instances.expand_labels(labd, distance)
            assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), ir.expand_labels(lab, distance)), (shape, distance)
        assert np.array_equal(labd.cpu().numpy(), lab)


def _split_volumes():
    yield 'planted split', planted_split(), 1
    yield 'planted leak', planted_leak(), 1
    yield 'grains', _volume('grains', 'ragged'), 1
    yield 'grains, class 2', _volume('grains', 'ragged'), 2
    yield 'predicted', _volume('5', 'flat'), 0
    yield 'one voxel', _volume('all', 'one voxel'), 1
    yield 'row', _volume('p50', 'row'), 1
    yield 'nothing', _volume('none', 'flat'), 1


@pytest.mark.parametrize('conn', (6, 26))
@pytest.mark.parametrize('radius', (0, 1.5, 4))
def test_split_touching_on_resident_volumes(radius, conn):
    from interactive_unet import instances
    for what, v, target in _split_volumes():
        vd = torch.tensor(v).cuda()
        labels, count = instances.split_touching(vd, target, radius, conn)
        want, k = ir.split_touching(v, target, radius, conn)
        assert labels.is_cuda and labels.dtype == torch.int32 and isinstance(count, int)
        assert count == k and np.array_equal(labels.cpu().numpy(), want), (what, radius, conn)
        sizes, first = instances.instance_table(labels, count)
        assert sizes.is_cuda and sizes.cpu().tolist() == [0] + np.bincount(want.reshape(-1), minlength=k + 1)[1:].tolist()
        assert first.cpu().tolist() == [-1] + [int(np.flatnonzero(want.reshape(-1) == i)[0]) for i in range(1, k + 1)]
        assert np.array_equal(vd.cpu().numpy(), v)
    if radius == 4 and conn == 6:
        assert instances.split_touching(torch.tensor(planted_split()).cuda(), 1, 4)[1] == 4
        labels, count = instances.split_touching(torch.tensor(planted_leak()).cuda(), 1, 2)
        assert count == 3 and torch.bincount(labels.reshape(-1))[1:].tolist() == [925, 525, 8]


def test_host_refusals_on_resident_volumes():
    from interactive_unet import instances
    vd = torch.tensor(_volume('grains', 'flat')).cuda()
    with pytest.raises(ValueError):
        instances.nearest(vd[:, :, ::2])
    with pytest.raises(ValueError):
        instances.split_touching(vd.to(torch.int32), 1, 1)
    with pytest.raises(ValueError, match='radius'):
        instances.split_touching(vd, 1, -1)
    with pytest.raises(ValueError, match='connectivity'):
        instances.split_touching(vd, 1, 1, 7)
    lab = torch.zeros((4, 5, 6), dtype=torch.int32, device='cuda')
    for bad in (lab.to(torch.int64), lab[0], lab[:, :, ::2], lab.cpu()):
        with pytest.raises(ValueError):
            instances.expand_labels(bad, 1)
        with pytest.raises(ValueError):
            instances.instance_table(bad, 0)
    with pytest.raises(ValueError, match='distance'):
        instances.expand_labels(lab, -1)


def test_split_touching_of_a_real_prediction():
    from interactive_unet import instances, predict
    from interactive_unet.unet import UNet
    from oracle import unet_ref
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = UNet(dim=3, levels=4, base=32, pretrained=False)
    m.load_named(unet_ref.init_params(dim=3, levels=4, base=32, seed=3, randomize_bn=True))
    m = m.cuda().eval()
    shape = (40, 36, 44)
    vol = np.random.default_rng(5).integers(0, 256, shape, dtype=np.uint8)
    pd = predict.predict_volume_array(m, torch.tensor(vol).cuda(), input_size=32, num_classes=2)
    assert pd.shape == shape + (2,) and pd.dtype == torch.uint8
    pred = pd.cpu().numpy()
    for target in (1, 0):
        for radius in (0, 1.5):
            labels, count = instances.split_touching(pd, target, radius)
            want, k = ir.split_touching(pred, target, radius)
            assert labels.is_cuda and count == k and np.array_equal(labels.cpu().numpy(), want), (target, radius)
