"""Geodesic seeded growth on the device: iunet_geo_init, iunet_geo_init_mask, iunet_geo_relax and iunet_geo_finish
bit for bit against the definition tests/geodesic_ref.py (the corridor against its closed form), and the host layer
interactive_unet/geodesic.py end to end -- on random, full, seedless, planted and degenerate volumes and on a real prediction of the 3-D
net.  Every comparison is exact equality; every output starts from a pattern and the workspace from 0xA5, so an element left unwritten
shows.  No case at volume scale: at 1030 x 1024 x 1024 the 8-byte keys take 8.6 GB and the maps beside them 4.3 GB each, over 30 GB with
the test's own copies (and that volume passes the chamfer metric's overflow limit)."""
import functools
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import geodesic_ref as gr
from tests.test_geodesic_cpu import grains, planted_leak, planted_split, sealed_pocket, serpentine
from tests.volume_inputs import offset_copy, random_pred

# ragged; a row; flat; one voxel; one axis longer than any workgroup, in turn along the row and along either column
SHAPES = {'ragged': (37, 41, 150), 'row': (1, 1, 300), 'flat': (33, 2, 65), 'one voxel': (1, 1, 1), 'long x': (3, 5, 2100),
          'long y': (3, 2100, 5), 'long z': (2100, 3, 5)}
SHAPE_NAMES = tuple(SHAPES)
DOMAINS = ('p60', 'all')
SEEDS = ('p01', 'none', 'all', 'plane')
TILE = (8, 8, 64)


@functools.lru_cache(maxsize=None)
def _domain(kind, name):
    """uint8 [Z, Y, X]: 1 on A."""
    shape = SHAPES[name]
    v = np.ones(shape, np.uint8) if kind == 'all' else (np.random.default_rng(SHAPE_NAMES.index(name)).random(shape) < 0.6).astype(np.uint8)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _seeds(kind, name):
    """int32 [Z, Y, X]: labels 1 .. 8, on and off A alike."""
    shape = SHAPES[name]
    rng = np.random.default_rng(50 + SHAPE_NAMES.index(name))
    lab = rng.integers(1, 9, shape).astype(np.int32)
    if kind == 'p01':
        s = np.where(rng.random(shape) < 0.01, lab, 0)
    elif kind == 'none':
        s = np.zeros(shape, np.int32)
    elif kind == 'all':
        s = lab
    else:
        s = np.zeros(shape, np.int32)
        s[0] = lab[0]
    s = np.ascontiguousarray(s, dtype=np.int32)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _want(dkind, skind, name, metric):
    """The definition's fixed point as the workspace holds it, computed once and shared."""
    key = gr.device_keys(gr.grow_keys(_domain(dkind, name) == 1, _seeds(skind, name), metric)[0])
    key.setflags(write=False)
    return key


def _ws(Z, Y, X):
    from interactive_unet import _native as nv
    ws_bytes = nv.lib().iunet_geo_ws_bytes(Z, Y, X)
    tiles = -(-Z // TILE[0]) * -(-Y // TILE[1]) * -(-X // TILE[2])
    assert ws_bytes == (8 * Z * Y * X + 15) // 16 * 16 + 2 * ((4 * tiles + 15) // 16 * 16)
    return torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device='cuda'), ws_bytes


def _init(srcd, seedsd, target=1, mask=False):
    """The entry points themselves: a workspace in its initial state."""
    from interactive_unet import _native as nv
    Z, Y, X = srcd.shape[:3]
    ws, ws_bytes = _ws(Z, Y, X)
    if mask:
        nv.call('iunet_geo_init_mask', nv.ptr(srcd), Z, Y, X, nv.ptr(seedsd), nv.ptr(ws), ws_bytes, nv.stream())
    else:
        C = 1 if srcd.ndim == 3 else srcd.shape[3]
        nv.call('iunet_geo_init', nv.ptr(srcd), Z, Y, X, C, target, nv.ptr(seedsd), nv.ptr(ws), ws_bytes, nv.stream())
    return ws, ws_bytes, (Z, Y, X)


def _relax(state, weights, rounds=8, limit=5000):
    """Calls of `rounds` rounds until no tile changes; the number of rounds."""
    from interactive_unet import _native as nv
    ws, ws_bytes, (Z, Y, X) = state
    changed = torch.full((1,), -3, dtype=torch.int32, device='cuda')
    done = 0
    while True:
        nv.call('iunet_geo_relax', nv.ptr(ws), ws_bytes, Z, Y, X, weights[0], weights[1], weights[2], rounds, nv.ptr(changed), nv.stream())
        done += rounds
        n = int(changed.item())
        assert 0 <= n and done <= limit
        if n == 0:
            return done


def _finish(state, want_g=True, fallback=None, offset=0, labels=None, g=None):
    from interactive_unet import _native as nv
    ws, ws_bytes, (Z, Y, X) = state
    labels = torch.full((Z, Y, X), -7, dtype=torch.int32, device='cuda') if labels is None else labels
    g = (torch.full((Z, Y, X), -9, dtype=torch.int32, device='cuda') if g is None else g) if want_g else None
    nv.call('iunet_geo_finish', nv.ptr(ws), ws_bytes, Z, Y, X, nv.ptr(labels), nv.ptr(g), nv.ptr(fallback), offset, nv.stream())
    return labels, g


def _keys(state):
    ws, _, (Z, Y, X) = state
    return ws[:8 * Z * Y * X].view(torch.int64).reshape(Z, Y, X).cpu().numpy()


def _grown(srcd, seedsd, metric, target=1, mask=False):
    """init, relax to rest, finish: (keys, labels, g) on the host."""
    state = _init(srcd, seedsd, target, mask)
    _relax(state, gr.weights_of(metric))
    labels, g = _finish(state)
    return _keys(state), labels.cpu().numpy(), g.cpu().numpy()


def _same(got, key, where):
    """got = (keys, labels, g) against the definition's state."""
    assert np.array_equal(got[0], key), ('keys', where)
    labels, g = gr.split_keys(key.view(np.uint64))
    assert np.array_equal(got[2], g), ('g', where)
    assert np.array_equal(got[1], labels), ('labels', where)


@pytest.mark.parametrize('skind', SEEDS)
@pytest.mark.parametrize('dkind', DOMAINS)
@pytest.mark.parametrize('name', SHAPE_NAMES)
def test_class_maps(name, dkind, skind):
    srcd, seedsd = torch.tensor(_domain(dkind, name)).cuda(), torch.tensor(_seeds(skind, name)).cuda()
    for metric in ((6, 18, 26, 'chamfer') if name == 'ragged' else (6, 'chamfer')):
        _same(_grown(srcd, seedsd, metric), _want(dkind, skind, name, metric), (name, dkind, skind, metric))
    assert np.array_equal(srcd.cpu().numpy(), _domain(dkind, name)) and np.array_equal(seedsd.cpu().numpy(), _seeds(skind, name))


def test_weights_that_leave_a_rank_out_and_other_targets():
    v = _domain('p60', 'ragged')
    srcd, seedsd = torch.tensor(v * 3).cuda(), torch.tensor(_seeds('p01', 'ragged')).cuda()
    for weights in ((2, 0, 3), (5, 7, 0), (255, 255, 255)):
        key = gr.device_keys(gr.grow_keys(v == 1, _seeds('p01', 'ragged'), weights)[0])
        _same(_grown(srcd, seedsd, weights, target=3), key, weights)
    key = gr.device_keys(gr.grow_keys(v == 0, _seeds('p01', 'ragged'), 6)[0])
    _same(_grown(srcd, seedsd, 6, target=0), key, 'target 0')


def _corridor(perm):
    """The serpentine corridor of 5 x 40 x 150, its axes permuted: (a uint8, path)."""
    a, path = serpentine((5, 40, 150))
    return np.ascontiguousarray(np.transpose(a, perm)), path[:, list(perm)]


@pytest.mark.parametrize('perm', ((0, 1, 2), (2, 0, 1), (1, 2, 0)))
def test_the_serpentine_corridor(perm):
    """About 3000 steps that cross and re-enter tiles many times: more than one round; g against the closed form."""
    a, path = _corridor(perm)
    n = len(path)
    assert n == 20 * 150 + 19 and a.shape == tuple(np.array((5, 40, 150))[list(perm)])
    ad = torch.tensor(a).cuda()
    at = tuple(path.T)
    pos = np.arange(n)
    for weights in ((1, 0, 0), (3, 0, 0)):
        seeds = np.zeros(a.shape, np.int32)
        seeds[tuple(path[0])] = 4
        state = _init(ad, torch.tensor(seeds).cuda())
        rounds = _relax(state, weights, rounds=1)
        assert rounds > 2                                               # the last round only finds that nothing changes
        labels, g = (t.cpu().numpy() for t in _finish(state))
        assert np.array_equal(g[at], weights[0] * pos) and (g[a == 0] == gr.INF).all(), (perm, weights)
        assert (labels[a == 1] == 4).all() and not labels[a == 0].any()
        # a seed at each end: the midpoint, at the same distance of both, goes to the smaller label
        seeds[tuple(path[0])], seeds[tuple(path[-1])] = 9, 2
        _, labels, g = _grown(ad, torch.tensor(seeds).cuda(), weights)
        assert n % 2 == 1 and np.array_equal(g[at], weights[0] * np.minimum(pos, n - 1 - pos))
        assert np.array_equal(labels[at], np.where(pos < n // 2, 9, 2)) and labels[tuple(path[n // 2])] == 2


def test_max_rounds_on_the_corridor():
    from interactive_unet import geodesic
    a, path = _corridor((0, 1, 2))
    seeds = np.zeros(a.shape, np.int32)
    seeds[tuple(path[0])] = 1
    ad, sd = torch.tensor(a).cuda(), torch.tensor(seeds).cuda()
    with pytest.raises(RuntimeError, match='max_rounds'):
        geodesic.grow(ad, sd, 1, 6, max_rounds=1)
    labels, g = geodesic.grow(ad, sd, 1, 6)
    assert np.array_equal(g.cpu().numpy()[tuple(path.T)], np.arange(len(path))) and bool((labels[ad == 1] == 1).all())


def test_a_tie_and_a_sealed_pocket_across_a_tile_seam():
    # a line of five voxels across the seam of two tiles, along each axis in turn: seeds 7 and 3 at its ends
    for axis, lo in ((2, 62), (1, 6), (0, 6)):
        shape = [3, 3, 3]
        shape[axis] = lo + 8
        a, seeds = np.zeros(shape, np.uint8), np.zeros(shape, np.int32)
        line = [1, 1, 1]
        for k in range(5):
            line[axis] = lo + k
            a[tuple(line)] = 1
            seeds[tuple(line)] = {0: 7, 4: 3}.get(k, 0)
        for metric in (6, 'chamfer'):
            got = _grown(torch.tensor(a).cuda(), torch.tensor(seeds).cuda(), metric)
            _same(got, gr.device_keys(gr.grow_keys(a == 1, seeds, metric)[0]), (axis, metric))
            assert got[1][a == 1].tolist() == [7, 7, 3, 3, 3]
    # a wall on the first plane of the second tile: nothing behind it is reached
    for axis, n, wall in ((2, 80, 64), (1, 20, 8), (0, 20, 8)):
        shape = [5, 6, 7]
        shape[axis] = n
        a = np.ones(shape, np.uint8)
        index = [slice(None)] * 3
        index[axis] = wall
        a[tuple(index)] = 0
        seeds = np.zeros(shape, np.int32)
        seeds[2, 2, 1] = 4
        index[axis] = slice(wall + 1, None)
        for metric in (6, 'chamfer'):
            got = _grown(torch.tensor(a).cuda(), torch.tensor(seeds).cuda(), metric)
            _same(got, gr.device_keys(gr.grow_keys(a == 1, seeds, metric)[0]), (axis, metric))
            assert (got[2][tuple(index)] == gr.INF).all() and not got[1][tuple(index)].any() and (got[1] == 4).sum() == a.sum() - a[tuple(index)].sum()
    a, seeds, pocket = sealed_pocket()
    got = _grown(torch.tensor(a.astype(np.uint8)).cuda(), torch.tensor(seeds).cuda(), 26)
    assert (got[2][pocket] == gr.INF).all() and (got[1][a & ~pocket] == 4).all()


@pytest.mark.parametrize('C', (2, 5))
@pytest.mark.parametrize('name', ('ragged', 'flat', 'one voxel'))
def test_predicted_volumes(name, C):
    pred = random_pred(SHAPES[name], C, 30 + SHAPE_NAMES.index(name))
    predd, seedsd = torch.tensor(pred).cuda(), torch.tensor(_seeds('p01' if name == 'ragged' else 'plane', name)).cuda()
    seeds = seedsd.cpu().numpy()
    for target in (0, 1):
        for metric in (6, 'chamfer'):
            key = gr.device_keys(gr.grow_keys(gr.members(pred, target), seeds, metric)[0])
            _same(_grown(predd, seedsd, metric, target=target), key, (name, C, target, metric))
            _same(_grown(predd, offset_copy(seedsd, 4), metric, target=target), key, (name, C, target, metric, 'narrow'))


@pytest.mark.parametrize('name', ('ragged', 'flat', 'long y', 'one voxel'))
def test_the_domain_from_a_label_map(name):
    shape = SHAPES[name]
    rng = np.random.default_rng(7)
    dom = np.where(rng.random(shape) < 0.65, rng.integers(1, 2 ** 31 - 1, shape), -rng.integers(0, 5, shape)).astype(np.int32)
    seeds = _seeds('p01' if name == 'ragged' else 'plane', name)
    domd, seedsd = torch.tensor(dom).cuda(), torch.tensor(seeds).cuda()
    for metric in (6, 'chamfer'):
        key = gr.device_keys(gr.grow_keys(dom > 0, seeds, metric)[0])
        _same(_grown(domd, seedsd, metric, mask=True), key, (name, metric))
        _same(_grown(offset_copy(domd, 4), seedsd, metric, mask=True), key, (name, metric, 'narrow'))
        _same(_grown(torch.tensor((dom > 0).astype(np.uint8)).cuda(), offset_copy(seedsd, 8), metric), key, (name, metric, 'class map, narrow'))
    assert np.array_equal(domd.cpu().numpy(), dom)


def test_rounds_one_at_a_time_in_batches_and_after_rest_give_the_same_bytes():
    from interactive_unet import _native as nv
    for dkind, skind, name, metric in (('p60', 'p01', 'ragged', 'chamfer'), ('all', 'plane', 'long x', 6), ('p60', 'plane', 'flat', 18)):
        srcd, seedsd = torch.tensor(_domain(dkind, name)).cuda(), torch.tensor(_seeds(skind, name)).cuda()
        weights = gr.weights_of(metric)
        one, eight = _init(srcd, seedsd), _init(srcd, seedsd)
        assert torch.equal(one[0], eight[0])
        r1, r8 = _relax(one, weights, rounds=1), _relax(eight, weights, rounds=8)
        assert r1 >= 1 and r8 % 8 == 0 and torch.equal(one[0], eight[0]), (name, r1, r8)
        assert np.array_equal(_keys(one), _want(dkind, skind, name, metric))
        # at rest: a further call reports 0 and leaves every byte
        before = one[0].clone()
        changed = torch.full((1,), -3, dtype=torch.int32, device='cuda')
        for rounds in (1, 3):
            nv.call('iunet_geo_relax', nv.ptr(one[0]), one[1], *one[2], *weights, rounds, nv.ptr(changed), nv.stream())
            assert int(changed.item()) == 0 and torch.equal(one[0], before)
        # a second stream
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            other = _init(srcd, seedsd)
            _relax(other, weights, rounds=8)
            lo, go = _finish(other)
        side.synchronize()
        la, ga = _finish(one)
        assert torch.equal(other[0], one[0]) and torch.equal(lo, la) and torch.equal(go, ga)


@pytest.mark.parametrize('shape', ((1, 1, 3), (1, 5, 821), (37, 41, 150)))
def test_finish_with_and_without_g_and_fallback_at_any_alignment(shape):
    """N = 3 and N = 4096 + 9: the voxels past the last whole step; outputs 4 and 8 bytes off 16: the one-voxel path."""
    rng = np.random.default_rng(int(np.prod(shape)))
    a = rng.random(shape) < 0.5                                            # sparse enough to leave voxels of A unreached
    seeds = np.where(rng.random(shape) < 0.02, rng.integers(1, 9, shape), 0).astype(np.int32)
    seeds[0, 0, 0] = 5
    fb = rng.integers(1, 40, shape).astype(np.int32)
    key = gr.grow_keys(a, seeds, 6)[0]
    assert np.prod(shape) < 10 or ((key == gr._UNREACHED).any() and (key < gr._UNREACHED).any())
    state = _init(torch.tensor(a.astype(np.uint8)).cuda(), torch.tensor(seeds).cuda())
    _relax(state, (1, 0, 0))
    fbd = torch.tensor(fb).cuda()
    pattern = lambda by, value: offset_copy(torch.full(shape, value, dtype=torch.int32, device='cuda'), by)
    for fallback, offset in ((None, 0), (fbd, 0), (fbd, 1000), (offset_copy(fbd, 4), 1000)):
        want = gr.finish(key, None if fallback is None else fb, offset)
        for by_l, by_g in ((0, 0), (4, 0), (0, 8), (12, 4)):
            labels, g = _finish(state, fallback=fallback, offset=offset, labels=pattern(by_l, -7), g=pattern(by_g, -9))
            assert np.array_equal(labels.cpu().numpy(), want[0]) and np.array_equal(g.cpu().numpy(), want[1]), (shape, offset, by_l, by_g)
            labels, g = _finish(state, want_g=False, fallback=fallback, offset=offset, labels=pattern(by_l, -7))
            assert g is None and np.array_equal(labels.cpu().numpy(), want[0]), (shape, offset, by_l)
    assert np.array_equal(fbd.cpu().numpy(), fb)


@functools.lru_cache(maxsize=None)
def _split_volumes():
    g = grains(SHAPES['ragged'], 20)
    return (('planted split', planted_split(), 1), ('planted leak', planted_leak(), 1), ('grains', g, 1), ('grains, class 2', g, 2),
            ('predicted', random_pred(SHAPES['flat'], 5, 32), 0), ('one voxel', np.ones((1, 1, 1), np.uint8), 1), ('row', _domain('p60', 'row'), 1),
            ('nothing', np.zeros(SHAPES['flat'], np.uint8), 1))


@functools.lru_cache(maxsize=None)
def _split_want(what, radius, conn, metric):
    v, target = next((v, t) for w, v, t in _split_volumes() if w == what)
    return gr.split_touching(v, target, radius, conn, metric)


@pytest.mark.parametrize('conn', (6, 26))
@pytest.mark.parametrize('radius', (0, 1.5, 4))
def test_split_touching_on_resident_volumes(radius, conn):
    from interactive_unet import geodesic
    for what, v, target in _split_volumes():
        vd = torch.tensor(v).cuda()
        for metric in ('chamfer',) if radius != 1.5 else ('chamfer', 6):
            labels, count = geodesic.split_touching(vd, target, radius, conn, metric)
            want, k = _split_want(what, radius, conn, metric)
            assert labels.is_cuda and labels.dtype == torch.int32 and isinstance(count, int)
            assert count == k and np.array_equal(labels.cpu().numpy(), want), (what, radius, conn, metric)
        assert np.array_equal(vd.cpu().numpy(), v)
    if radius == 4 and conn == 6:
        labels, count = geodesic.split_touching(torch.tensor(planted_split()).cuda(), 1, 4)
        assert count == 4 and torch.bincount(labels.reshape(-1))[1:].tolist() == [924, 887, 933, 33]
        for r in (2, 3):
            labels, count = geodesic.split_touching(torch.tensor(planted_leak()).cuda(), 1, r)
            assert count == 2 and torch.bincount(labels.reshape(-1))[1:].tolist() == [925, 533]


def test_grow_and_grow_in_on_resident_volumes():
    from interactive_unet import geodesic
    for v, target in ((_split_volumes()[2][1], 1), (random_pred(SHAPES['flat'], 2, 31), 0), (random_pred(SHAPES['ragged'], 5, 30), 3),
                      (np.ones((1, 1, 1), np.uint8), 1), (planted_leak(), 1), (planted_split(), 1)):
        shape = v.shape[:3]
        seeds = np.where(np.random.default_rng(3).random(shape) < 0.01, np.random.default_rng(4).integers(1, 9, shape), 0).astype(np.int32)
        vd, sd = torch.tensor(v).cuda(), torch.tensor(seeds).cuda()
        for metric in ('chamfer', 6, (2, 0, 3)):
            labels, g = geodesic.grow(vd, sd, target, metric)
            want = gr.grow(v, seeds, target, metric)
            assert labels.is_cuda and labels.dtype == torch.int32 and g.dtype == torch.int32
            assert np.array_equal(g.cpu().numpy(), want[1]) and np.array_equal(labels.cpu().numpy(), want[0]), (shape, target, metric)
        dom = np.where(gr.members(v, target), 9, 0).astype(np.int32)
        labels, g = geodesic.grow_in(torch.tensor(dom).cuda(), sd)
        want = gr.grow_in(dom, seeds)
        assert np.array_equal(g.cpu().numpy(), want[1]) and np.array_equal(labels.cpu().numpy(), want[0]), shape
        assert np.array_equal(vd.cpu().numpy(), v) and np.array_equal(sd.cpu().numpy(), seeds)


def test_host_refusals_on_resident_volumes():
    from interactive_unet import geodesic
    vd = torch.tensor(grains(SHAPES['flat'], 22)).cuda()
    sd = torch.zeros(SHAPES['flat'], dtype=torch.int32, device='cuda')
    for bad in (vd[:, :, ::2], vd.to(torch.int32), vd.cpu()):
        with pytest.raises(ValueError):
            geodesic.grow(bad, sd)
        with pytest.raises(ValueError):
            geodesic.split_touching(bad, 1, 1)
    for bad in (sd.to(torch.int64), sd[0], sd[:, :, ::2], sd.cpu(), sd.cpu().numpy(), sd[:, :, :64].contiguous(), None):
        with pytest.raises(ValueError, match='seeds'):
            geodesic.grow(vd, bad)
        with pytest.raises(ValueError, match='seeds'):
            geodesic.grow_in(sd, bad)
    for bad in (sd.to(torch.int64), sd[0], sd[:, :, ::2], sd.cpu()):
        with pytest.raises(ValueError):
            geodesic.grow_in(bad, sd)
    with pytest.raises(ValueError, match='metric'):
        geodesic.grow(vd, sd, 1, 7)
    with pytest.raises(ValueError, match='radius'):
        geodesic.split_touching(vd, 1, -1)
    with pytest.raises(ValueError, match='connectivity'):
        geodesic.split_touching(vd, 1, 1, 7)
    with pytest.raises(ValueError, match='max_rounds'):
        geodesic.grow(vd, sd, max_rounds=0)


def test_split_touching_of_a_real_prediction():
    from interactive_unet import geodesic, predict
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
            labels, count = geodesic.split_touching(pd, target, radius)
            want, k = geodesic.split_touching(pred, target, radius)
            assert labels.is_cuda and count == k and np.array_equal(labels.cpu().numpy(), want), (target, radius)
            ref = gr.split_touching(pred, target, radius)
            assert k == ref[1] and np.array_equal(want, ref[0]), (target, radius)
