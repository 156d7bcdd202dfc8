"""Grayscale reconstruction on the device: iunet_rec_init, iunet_rec_relax, iunet_rec_landscape and iunet_rec_select
bit for bit against the definition tests/reconstruct_ref.py (the corridor and the cracks against their closed forms too), and the host
layer interactive_unet/reconstruction.py end to end -- on small-range and full-range landscapes, planted and degenerate volumes and a
real prediction of the 3-D net.  Every comparison is exact equality; every output starts from a pattern (r -7, out 0xA5, the flags 0xA5),
so an element left unwritten shows.  No case at volume scale: at 1030 x 1024 x 1024 marker, mask and r take 4.3 GB each and the test's
own copies as much again; the 64-bit indexing is covered by the limits tests/test_reconstruct_cpu.py checks through the library."""
import functools
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import reconstruct_ref as rr
from tests.reconstruct_inputs import blobs, landscape_values, planted, serpentine
from tests.volume_inputs import offset_copy, random_pred

# ragged; a row; flat; one voxel; one axis longer than any workgroup, in turn along the row and along either column
SHAPES = {'ragged': (37, 41, 150), 'row': (1, 1, 300), 'flat': (33, 2, 65), 'one voxel': (1, 1, 1), 'long x': (3, 5, 2100),
          'long y': (3, 2100, 5), 'long z': (2100, 3, 5)}
SHAPE_NAMES = tuple(SHAPES)
KINDS = ('small', 'full')
TILE = (8, 8, 64)
LOW, HIGH = -2 ** 31, 2 ** 31 - 1
HEIGHTS = (0, 1, HIGH)


@functools.lru_cache(maxsize=None)
def _maps(kind, name):
    """(marker, mask) int32 [Z, Y, X].  small: values -3 .. 3, so that plateaus span the tile seams; full: the whole int32 range, a twentieth
    of the voxels each at -2^31 and at 2^31 - 1."""
    shape = SHAPES[name]
    rng = np.random.default_rng(10 * SHAPE_NAMES.index(name) + KINDS.index(kind))
    out = []
    for _ in range(2):
        if kind == 'small':
            m = rng.integers(-3, 4, shape)
        else:
            m = rng.integers(LOW, HIGH + 1, shape)
            pick = rng.random(shape)
            m = np.where(pick < 0.05, LOW, np.where(pick > 0.95, HIGH, m))
        m = np.ascontiguousarray(m, dtype=np.int32)
        m.setflags(write=False)
        out.append(m)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _want(kind, name, conn, erosion, h, alias=False):
    """The definition's fixed point, computed once and shared."""
    marker, mask = _maps(kind, name)
    r = rr.reconstruct(mask if alias else marker, mask, conn, erosion, h)
    r.setflags(write=False)
    return r


def _tiles(Z, Y, X):
    return -(-Z // TILE[0]) * -(-Y // TILE[1]) * -(-X // TILE[2])


def _init(markerd, maskd, h=0, erosion=False, r=None):
    """The entry point itself: (r, mask, ws, ws_bytes, dims) in the initial state."""
    from interactive_unet import _native as nv
    Z, Y, X = maskd.shape
    ws_bytes = nv.lib().iunet_rec_ws_bytes(Z, Y, X)
    assert ws_bytes == 2 * ((4 * _tiles(Z, Y, X) + 15) // 16 * 16)
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device='cuda')
    r = torch.full((Z, Y, X), -7, dtype=torch.int32, device='cuda') if r is None else r
    nv.call('iunet_rec_init', nv.ptr(markerd), nv.ptr(maskd), Z, Y, X, h, int(erosion), nv.ptr(r), nv.ptr(ws), ws_bytes, nv.stream())
    return r, maskd, ws, ws_bytes, (Z, Y, X)


def _relax(state, conn, erosion=False, rounds=8, limit=5000):
    """Calls of `rounds` rounds until no tile changes; the number of rounds."""
    from interactive_unet import _native as nv
    r, maskd, ws, ws_bytes, (Z, Y, X) = state
    changed = torch.full((1,), -3, dtype=torch.int32, device='cuda')
    done = 0
    while True:
        nv.call('iunet_rec_relax', nv.ptr(r), nv.ptr(maskd), Z, Y, X, conn, int(erosion), rounds, nv.ptr(changed), nv.ptr(ws), ws_bytes, nv.stream())
        done += rounds
        n = int(changed.item())
        assert 0 <= n <= _tiles(Z, Y, X) and done <= limit
        if n == 0:
            return done


def _rest(markerd, maskd, conn, erosion=False, h=0, rounds=8):
    state = _init(markerd, maskd, h, erosion)
    _relax(state, conn, erosion, rounds)
    return state[0].cpu().numpy()


@pytest.mark.parametrize('h', HEIGHTS)
@pytest.mark.parametrize('erosion', (False, True))
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', SHAPE_NAMES)
def test_reconstruction_of_random_landscapes(name, kind, erosion, h):
    marker, mask = _maps(kind, name)
    markerd, maskd = torch.tensor(marker).cuda(), torch.tensor(mask).cuda()
    state = _init(markerd, maskd, h, erosion)
    assert np.array_equal(state[0].cpu().numpy(), rr.first_state(marker, mask, h, erosion))
    n, part = _tiles(*mask.shape), state[3] // 2
    flags = state[2].cpu().numpy()
    for half in (flags[:part], flags[part:]):                              # every flag set, the padding behind them untouched
        assert (half[:4 * n].view(np.int32) == 1).all() and (half[4 * n:] == 0xA5).all()
    for conn in ((6, 18, 26) if name == 'ragged' else (6, 26)):
        got = _rest(markerd, maskd, conn, erosion, h)
        assert np.array_equal(got, _want(kind, name, conn, erosion, h)), (name, kind, conn, erosion, h)
    assert np.array_equal(markerd.cpu().numpy(), marker) and np.array_equal(maskd.cpu().numpy(), mask)


@pytest.mark.parametrize('name', ('ragged', 'flat', 'one voxel'))
def test_marker_may_be_mask(name):
    for kind in KINDS:
        mask = _maps(kind, name)[1]
        maskd = torch.tensor(mask).cuda()
        for erosion in (False, True):
            for h in (1, 2):
                assert np.array_equal(_rest(maskd, maskd, 26, erosion, h), _want(kind, name, 26, erosion, h, alias=True)), (name, kind, erosion, h)
        assert np.array_equal(_rest(maskd, maskd, 6, False, 0), mask)
        assert np.array_equal(maskd.cpu().numpy(), mask)


def _corridor(perm):
    """The serpentine corridor of 5 x 40 x 150, its axes permuted: (a uint8, path)."""
    a, path = serpentine((5, 40, 150))
    return np.ascontiguousarray(np.transpose(a, perm)), path[:, list(perm)]


@pytest.mark.parametrize('perm', ((0, 1, 2), (2, 0, 1), (1, 2, 0)))
def test_the_serpentine_corridor(perm):
    """About 3000 steps that cross and re-enter tiles many times: more than one round; R is the plateau on the whole corridor."""
    from interactive_unet import reconstruction
    a, path = _corridor(perm)
    assert len(path) == 20 * 150 + 19 and a.shape == tuple(np.array((5, 40, 150))[list(perm)])
    mask = np.where(a == 1, 7, LOW).astype(np.int32)
    marker = np.full(a.shape, LOW, np.int32)
    marker[tuple(path[0])] = 7
    markerd, maskd = torch.tensor(marker).cuda(), torch.tensor(mask).cuda()
    state = _init(markerd, maskd)
    rounds = _relax(state, 6, rounds=1)
    assert rounds > 2                                                       # the last round only finds that nothing changes
    assert np.array_equal(state[0].cpu().numpy(), mask)
    assert np.array_equal(_rest(markerd, maskd, 26), mask)
    # the dual: a pit of -8 in a corridor whose walls are 2^31 - 1
    got = _rest(torch.tensor(~marker).cuda(), torch.tensor(~mask).cuda(), 6, erosion=True)
    assert np.array_equal(got, ~mask)
    with pytest.raises(RuntimeError, match='max_rounds'):
        reconstruction.reconstruct(markerd, maskd, max_rounds=1)
    assert np.array_equal(reconstruction.reconstruct(markerd, maskd).cpu().numpy(), mask)


def _at(axis, a, u, v):
    index = [u, v]
    index.insert(axis, a)
    return tuple(index)


def test_a_plateau_and_a_crack_across_a_tile_seam():
    for axis, n, wall in ((2, 80, 64), (1, 20, 8), (0, 20, 8)):
        shape = [5, 6, 7]
        shape[axis] = n
        behind = [slice(None)] * 3
        behind[axis] = slice(wall + 1, None)
        behind = tuple(behind)
        marker = np.full(shape, LOW, np.int32)
        marker[_at(axis, 1, 2, 2)] = 9
        md = torch.tensor(marker).cuda()
        # a plateau of 4 over both tiles: one marker voxel lifts all of it
        mask = np.full(shape, 4, np.int32)
        for conn in (6, 18, 26):
            assert np.array_equal(_rest(md, torch.tensor(mask).cuda(), conn), mask), (axis, conn)
        # a wall on the first plane of the second tile: nothing behind it rises
        plane = [slice(None)] * 3
        plane[axis] = wall
        mask[tuple(plane)] = LOW
        for conn in (6, 26):
            got = _rest(md, torch.tensor(mask).cuda(), conn)
            assert np.array_equal(got, rr.reconstruct(marker, mask, conn)) and (got[behind] == LOW).all() and got[_at(axis, wall - 1, 0, 0)] == 4
        # a one-voxel crack in the wall: a face step passes it
        mask[_at(axis, wall, 3, 3)] = 4
        for conn in (6, 26):
            got = _rest(md, torch.tensor(mask).cuda(), conn)
            assert np.array_equal(got, rr.reconstruct(marker, mask, conn)) and np.array_equal(got, mask), (axis, conn)
        # a crack that the front side touches by a vertex step only: crossed at connectivity 26 and not at 18
        mask[_at(axis, wall, 3, 3)] = LOW
        mask[_at(axis, wall, 0, 0)] = 4
        for u, v in ((0, 0), (1, 0), (0, 1)):
            mask[_at(axis, wall - 1, u, v)] = LOW
        for conn in (6, 18, 26):
            got = _rest(md, torch.tensor(mask).cuda(), conn)
            assert np.array_equal(got, rr.reconstruct(marker, mask, conn)), (axis, conn)
            assert (got[behind] == (4 if conn == 26 else LOW)).all() and got[_at(axis, wall, 0, 0)] == (4 if conn == 26 else LOW), (axis, conn)


def test_rounds_one_at_a_time_in_batches_and_after_rest_give_the_same_bytes():
    from interactive_unet import _native as nv
    for kind, name, conn, erosion, h in (('small', 'ragged', 26, False, 1), ('full', 'long x', 6, True, 0), ('small', 'flat', 18, False, 0)):
        marker, mask = _maps(kind, name)
        markerd, maskd = torch.tensor(marker).cuda(), torch.tensor(mask).cuda()
        one, eight = _init(markerd, maskd, h, erosion), _init(markerd, maskd, h, erosion)
        assert torch.equal(one[0], eight[0]) and torch.equal(one[2], eight[2])
        r1, r8 = _relax(one, conn, erosion, rounds=1), _relax(eight, conn, erosion, rounds=8)
        assert r1 >= 1 and r8 % 8 == 0 and torch.equal(one[0], eight[0]), (name, r1, r8)
        assert np.array_equal(one[0].cpu().numpy(), _want(kind, name, conn, erosion, h))
        # at rest: a further call reports 0 and leaves every byte
        before, flags = one[0].clone(), one[2].clone()
        changed = torch.full((1,), -3, dtype=torch.int32, device='cuda')
        for rounds in (1, 3):
            nv.call('iunet_rec_relax', nv.ptr(one[0]), nv.ptr(maskd), *one[4], conn, int(erosion), rounds, nv.ptr(changed), nv.ptr(one[2]), one[3], nv.stream())
            assert int(changed.item()) == 0 and torch.equal(one[0], before) and torch.equal(one[2], flags)
        # a second stream
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            other = _init(markerd, maskd, h, erosion)
            _relax(other, conn, erosion, rounds=8)
        side.synchronize()
        assert torch.equal(other[0], one[0])


@pytest.mark.parametrize('shape', ((1, 1, 3), (1, 5, 821), (37, 41, 150)))
def test_the_streaming_passes_at_any_alignment(shape):
    """N = 3 and N = 4096 + 9: the voxels past the last whole step; a map 4 bytes off 16: the one-voxel path."""
    from interactive_unet import _native as nv
    rng = np.random.default_rng(int(np.prod(shape)))
    marker, mask = (rng.integers(-6, 7, shape).astype(np.int32) for _ in range(2))
    a, b = (rng.integers(LOW, HIGH + 1, shape).astype(np.int32) for _ in range(2))
    md, kd, ad, bd = (torch.tensor(x).cuda() for x in (marker, mask, a, b))
    Z, Y, X = shape
    for erosion, h in ((False, 2), (True, 1)):
        first, want = rr.first_state(marker, mask, h, erosion), rr.reconstruct(marker, mask, 26, erosion, h)
        for by_m, by_k, by_r in ((0, 0, 0), (4, 0, 0), (0, 4, 0), (0, 0, 4), (4, 4, 4), (8, 12, 4)):
            r = offset_copy(torch.full(shape, -7, dtype=torch.int32, device='cuda'), by_r)
            state = _init(offset_copy(md, by_m), offset_copy(kd, by_k), h, erosion, r=r)
            assert np.array_equal(r.cpu().numpy(), first), (by_m, by_k, by_r, erosion)
            _relax(state, 26, erosion)
            assert np.array_equal(r.cpu().numpy(), want), (by_m, by_k, by_r, erosion)
    for by_a, by_b, by_o in ((0, 0, 0), (4, 0, 0), (0, 8, 0), (0, 0, 1), (12, 4, 3)):
        for t, value in ((1, 1), (0, 255), (HIGH, 7), (LOW, 9), (-5, 0)):
            out, ao, bo = offset_copy(torch.full(shape, 0xA5, dtype=torch.uint8, device='cuda'), by_o), offset_copy(ad, by_a), offset_copy(bd, by_b)
            nv.call('iunet_rec_select', nv.ptr(ao), nv.ptr(bo), Z, Y, X, t, value, nv.ptr(out), nv.stream())
            assert np.array_equal(out.cpu().numpy(), rr.select(a, b, t, value)), (by_a, by_b, by_o, t, value)
    pool = np.concatenate([rng.integers(1, HIGH, 500), [1, 2, 3, HIGH]])      # few enough values for the restatement's math.isqrt
    d2 = np.where(rng.random(shape) < 0.3, 0, pool[rng.integers(0, len(pool), shape)]).astype(np.int32)
    for scale, off in ((4, LOW), (256, -1)):
        want = rr.landscape_of(d2, scale, off)
        for by_d, by_f in ((0, 0), (4, 0), (0, 4), (8, 8)):
            f, dd = offset_copy(torch.full(shape, -7, dtype=torch.int32, device='cuda'), by_f), offset_copy(torch.tensor(d2).cuda(), by_d)
            nv.call('iunet_rec_landscape', nv.ptr(dd), Z, Y, X, scale, off, nv.ptr(f), nv.stream())
            assert np.array_equal(f.cpu().numpy(), want), (by_d, by_f, scale)


def test_the_landscape_in_place_and_out_of_place():
    from interactive_unet import _native as nv
    d2 = landscape_values()
    Z, Y, X = d2.shape
    for scale in (1, 4, 256):
        want = rr.landscape_of(d2, scale)
        src = torch.tensor(d2).cuda()
        f = torch.full(d2.shape, -7, dtype=torch.int32, device='cuda')
        nv.call('iunet_rec_landscape', nv.ptr(src), Z, Y, X, scale, LOW, nv.ptr(f), nv.stream())
        assert np.array_equal(f.cpu().numpy(), want) and np.array_equal(src.cpu().numpy(), d2), scale
        nv.call('iunet_rec_landscape', nv.ptr(src), Z, Y, X, scale, LOW, nv.ptr(src), nv.stream())
        assert np.array_equal(src.cpu().numpy(), want), scale


def test_select_takes_the_difference_in_64_bits():
    from interactive_unet import _native as nv
    a = np.array([HIGH, LOW, HIGH, LOW, 0, -1, 5], np.int32).reshape(1, 1, -1)
    b = np.array([LOW, HIGH, HIGH, LOW, 0, 0, 4], np.int32).reshape(1, 1, -1)
    ad, bd = torch.tensor(a).cuda(), torch.tensor(b).cuda()
    for t in (LOW, -1, 0, 1, 2, HIGH):
        out = torch.full(a.shape, 0xA5, dtype=torch.uint8, device='cuda')
        nv.call('iunet_rec_select', nv.ptr(ad), nv.ptr(bd), 1, 1, a.shape[2], t, 200, nv.ptr(out), nv.stream())
        want = [200 if int(x) - int(y) >= t else 0 for x, y in zip(a.reshape(-1), b.reshape(-1))]
        assert out.cpu().numpy().reshape(-1).tolist() == want == rr.select(a, b, t, 200).reshape(-1).tolist(), t
    assert rr.select(a, b, 1, 200).reshape(-1).tolist() == [200, 0, 0, 0, 0, 0, 200]


@functools.lru_cache(maxsize=None)
def _volumes():
    return (('planted', planted(), 1), ('blobs', blobs((19, 23, 70), 0.5, 2), 1), ('blobs, class 0', blobs((20, 24, 40), 0.7, 7), 0),
            ('predicted', random_pred(SHAPES['flat'], 5, 32), 0), ('one voxel', np.ones((1, 1, 1), np.uint8), 1),
            ('everything', np.ones((9, 10, 70), np.uint8), 1), ('nothing', np.zeros(SHAPES['flat'], np.uint8), 1))


@functools.lru_cache(maxsize=None)
def _split_want(what, h, conn, metric):
    v, target = next((v, t) for w, v, t in _volumes() if w == what)
    return rr.hmax_markers(v, target, h, conn), rr.split_touching(v, target, h, conn, metric)


@pytest.mark.parametrize('conn', (6, 26))
@pytest.mark.parametrize('h', (0, 1.5, 25))
def test_markers_and_split_touching_on_resident_volumes(h, conn):
    from interactive_unet import reconstruction
    for what, v, target in _volumes():
        vd = torch.tensor(v).cuda()
        if h == 0:
            for scale in (1, 4):
                f = reconstruction.distance_landscape(vd, target, scale)
                assert f.is_cuda and f.dtype == torch.int32 and np.array_equal(f.cpu().numpy(), rr.distance_landscape(v, target, scale)), (what, scale)
        for metric in ('chamfer',) if h != 1.5 else ('chamfer', 6):
            (wm, km), (want, k) = _split_want(what, h, conn, metric)
            markers, count = reconstruction.hmax_markers(vd, target, h, conn)
            assert markers.is_cuda and markers.dtype == torch.int32 and isinstance(count, int)
            assert count == km and np.array_equal(markers.cpu().numpy(), wm), (what, h, conn)
            labels, count = reconstruction.split_touching(vd, target, h, conn, metric)
            assert labels.is_cuda and labels.dtype == torch.int32 and isinstance(count, int)
            assert count == k and np.array_equal(labels.cpu().numpy(), want), (what, h, conn, metric)
        assert np.array_equal(vd.cpu().numpy(), v)
    if h == 1.5 and conn == 6:
        vd = torch.tensor(planted()).cuda()
        for hh, n in ((0.25, 3), (3, 3), (3.25, 2), (20, 2)):
            assert reconstruction.hmax_markers(vd, 1, hh)[1] == n, hh
        labels, count = reconstruction.split_touching(vd, 1, 2)
        assert count == 3 and torch.bincount(labels.reshape(-1))[1:].tolist() == [123, 3013, 3013]


def test_the_map_functions_on_resident_tensors():
    from interactive_unet import reconstruction as m
    for kind, name in (('small', 'ragged'), ('full', 'flat'), ('small', 'one voxel'), ('small', 'row')):
        marker, mask = _maps(kind, name)
        markerd, maskd = torch.tensor(marker).cuda(), torch.tensor(mask).cuda()
        for conn in (6, 26):
            for method in m.METHODS:
                got = m.reconstruct(markerd, maskd, conn, method, 1)
                assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), _want(kind, name, conn, method == 'erosion', 1))
            for fn, h in (('hmaxima', 2), ('hminima', 2), ('extended_maxima', 1), ('extended_minima', 1), ('extended_maxima', 0)):
                got = getattr(m, fn)(maskd, h, conn)
                want = getattr(rr, fn)(mask, h, conn)
                assert got.is_cuda and got.cpu().numpy().dtype == want.dtype and np.array_equal(got.cpu().numpy(), want), (kind, name, conn, fn)
            for fn in ('regional_maxima', 'regional_minima'):
                got = getattr(m, fn)(maskd, conn)
                assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), getattr(rr, fn)(mask, conn)), (kind, name, conn, fn)
        assert np.array_equal(m.reconstruct(markerd, maskd).cpu().numpy(), _want(kind, name, 6, False, 0))
        assert np.array_equal(markerd.cpu().numpy(), marker) and np.array_equal(maskd.cpu().numpy(), mask)


def test_host_refusals_on_resident_tensors():
    from interactive_unet import reconstruction as m
    fd = torch.zeros(SHAPES['flat'], dtype=torch.int32, device='cuda')
    vd = torch.zeros(SHAPES['flat'], dtype=torch.uint8, device='cuda')
    for bad in (fd.to(torch.int64), fd[0], fd[:, :, ::2], fd.cpu(), fd.cpu().numpy(), fd[:, :, :64].contiguous(), None):
        with pytest.raises(ValueError, match='marker'):
            m.reconstruct(bad, fd)
    for bad in (fd.to(torch.int64), fd[0], fd[:, :, ::2], fd.cpu(), None):
        for call in (lambda x: m.reconstruct(fd, x), lambda x: m.hmaxima(x, 1), lambda x: m.regional_minima(x), lambda x: m.extended_maxima(x, 1)):
            with pytest.raises(ValueError):
                call(bad)
    for bad in (vd[:, :, ::2], vd.to(torch.int32), vd.cpu()):
        for call in (lambda x: m.distance_landscape(x), lambda x: m.hmax_markers(x, 1, 1), lambda x: m.split_touching(x, 1, 1)):
            with pytest.raises(ValueError):
                call(bad)
    for call, word in ((lambda: m.reconstruct(fd, fd, 7), 'connectivity'), (lambda: m.reconstruct(fd, fd, 6, 'opening'), 'method'),
                       (lambda: m.reconstruct(fd, fd, h=-1), 'h '), (lambda: m.hmaxima(fd, 1.5), 'h '), (lambda: m.reconstruct(fd, fd, max_rounds=0), 'max_rounds'),
                       (lambda: m.hmax_markers(vd, 1, -1), 'h '), (lambda: m.hmax_markers(vd, 1, 2 ** 30), 'h '), (lambda: m.split_touching(vd, 1, 1, 7), 'connectivity'),
                       (lambda: m.split_touching(vd, 1, 1, 6, 'euclid'), 'metric'), (lambda: m.split_touching(vd, 1, 1, scale=0), 'scale'),
                       (lambda: m.distance_landscape(vd, 256), 'target'), (lambda: m.split_touching(vd, 1, 1, max_rounds=0), 'max_rounds')):
        with pytest.raises(ValueError, match=word):
            call()


def test_split_touching_of_a_real_prediction():
    from interactive_unet import predict, reconstruction
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
        for h in (0.5, 2):
            labels, count = reconstruction.split_touching(pd, target, h)
            want, k = reconstruction.split_touching(pred, target, h)
            assert labels.is_cuda and count == k and np.array_equal(labels.cpu().numpy(), want), (target, h)
            ref = rr.split_touching(pred, target, h)
            assert k == ref[1] and np.array_equal(want, ref[0]), (target, h)
