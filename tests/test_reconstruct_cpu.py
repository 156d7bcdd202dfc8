"""Grayscale reconstruction and the h-maxima markers without a GPU: the definition tests/reconstruct_ref.py against
its level-set form (scipy.ndimage.label per level), the erosion against the bitwise-NOT dual, the saturation of h, the properties of
hmaxima, the landscape's integer square root against math.isqrt, the planted case count by count beside the erosion cores it is the
answer to, the invariants of the markers and the split on random blobs, the host layer's numpy path against the definition, the host
refusals, and the limits and the entry points' argument checks through the built library."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import reconstruct_ref as rr
from tests.reconstruct_inputs import blobs, landscape_values, planted
from tests.volume_inputs import random_pred

CONNS = (6, 18, 26)
LOW, HIGH = -2 ** 31, 2 ** 31 - 1


def random_pair(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-8, 8, shape).astype(np.int32), rng.integers(-5, 6, shape).astype(np.int32)


def by_levels(r0, mask, connectivity):
    """The level-set form: R[v] >= t iff v's component of {mask >= t} under the connectivity holds a voxel with r0 >= t."""
    from scipy import ndimage
    structure = ndimage.generate_binary_structure(3, rr.RANK[connectivity])
    out = np.full(mask.shape, min(int(r0.min()), int(mask.min())), np.int64)
    for t in np.union1d(r0, mask).tolist():                              # ascending: the sets shrink, the last level that holds v stays
        lab, _ = ndimage.label(mask >= t, structure=structure)
        out[np.isin(lab, np.unique(lab[r0 >= t])) & (lab > 0)] = t
    return out.astype(np.int32)


@pytest.mark.parametrize('conn', CONNS)
@pytest.mark.parametrize('shape', ((5, 6, 7), (1, 1, 20), (4, 1, 9)))
def test_the_sweep_form_is_the_level_set_form(shape, conn):
    """The restatement and, on its own, the module's numpy path against the independent definition."""
    from interactive_unet import reconstruction as m
    for trial in range(4):
        marker, mask = random_pair(shape, 10 * trial + sum(shape))
        for h in (0, 1, 3):
            r0 = rr.first_state(marker, mask, h)
            assert (r0 <= mask).all() and np.array_equal(r0, np.minimum(marker - h, mask))
            got = rr.reconstruct(marker, mask, conn, False, h)
            assert got.dtype == np.int32 and np.array_equal(got, by_levels(r0, mask, conn)), (shape, conn, trial, h)
            assert (got >= r0).all() and (got <= mask).all()
            assert np.array_equal(m.reconstruct(marker, mask, conn, 'dilation', h), by_levels(r0, mask, conn)), (shape, conn, trial, h)
            assert np.array_equal(rr.relax(got, mask, conn)[0], got)      # at rest


@pytest.mark.parametrize('conn', CONNS)
def test_erosion_is_the_bitwise_not_dual(conn):
    from interactive_unet import reconstruction as m
    for shape in ((5, 6, 7), (1, 1, 20)):
        marker, mask = random_pair(shape, 3)
        for h in (0, 2):
            assert np.array_equal(rr.reconstruct(marker, mask, conn, True, h), ~rr.reconstruct(~marker, ~mask, conn, False, h)), (shape, conn, h)
    rng = np.random.default_rng(4)
    marker, mask = (rng.integers(LOW, HIGH + 1, (4, 5, 6)).astype(np.int32) for _ in range(2))
    for h in (0, 1, HIGH):
        assert np.array_equal(rr.reconstruct(marker, mask, conn, True, h), ~rr.reconstruct(~marker, ~mask, conn, False, h)), (conn, h)
        assert np.array_equal(m.reconstruct(marker, mask, conn, 'erosion', h), ~m.reconstruct(~marker, ~mask, conn, 'dilation', h)), (conn, h)


def test_h_saturates_and_the_lowest_value_is_never_a_maximum():
    from interactive_unet import reconstruction as m
    marker = np.array([LOW, LOW + 5, -1, 0, HIGH], np.int32).reshape(1, 1, 5)
    mask = np.full((1, 1, 5), HIGH, np.int32)
    assert rr.first_state(marker, mask, HIGH).reshape(-1).tolist() == [LOW, LOW, LOW, LOW + 1, 0]
    assert rr.first_state(marker, mask, 10).reshape(-1).tolist() == [LOW, LOW, -11, -10, HIGH - 10]
    assert rr.first_state(marker, np.full((1, 1, 5), LOW, np.int32), HIGH, True).reshape(-1).tolist() == [-1, 4, HIGH - 1, HIGH, HIGH]
    f = np.full((3, 4, 9), LOW, np.int32)
    assert not rr.regional_maxima(f).any() and not rr.regional_minima(~f).any()
    assert not m.regional_maxima(f).any() and not m.regional_minima(~f).any()
    assert (m.reconstruct(marker, mask, h=HIGH) == 0).all() and (rr.reconstruct(marker, mask, h=HIGH) == 0).all()      # the line floods to its highest r0
    f[1, 1, 2:5] = 7
    f[1, 2, 7] = LOW + 1
    for conn in CONNS:
        assert np.array_equal(rr.regional_maxima(f, conn), (f > LOW).astype(np.uint8))
        assert np.array_equal(rr.regional_minima(~f, conn), (f > LOW).astype(np.uint8))
        assert np.array_equal(m.regional_maxima(f, conn), (f > LOW).astype(np.uint8)) and np.array_equal(m.regional_minima(~f, conn), (f > LOW).astype(np.uint8))
    assert rr.select(np.int32([HIGH]), np.int32([LOW]), HIGH).tolist() == [1] and rr.select(np.int32([LOW]), np.int32([HIGH]), LOW).tolist() == [0]


@pytest.mark.parametrize('conn', CONNS)
def test_the_properties_of_hmaxima(conn):
    from interactive_unet import reconstruction as m
    rng = np.random.default_rng(conn)
    f = rng.integers(-20, 21, (5, 6, 7)).astype(np.int32)
    assert np.array_equal(rr.hmaxima(f, 0, conn), f) and np.array_equal(rr.hminima(f, 0, conn), f)
    last = f
    for h in (1, 2, 5, 11):
        g = rr.hmaxima(f, h, conn)
        assert (g <= last).all() and (g >= f - h).all()                   # below f, falling with h, never by more than h
        assert (rr.hminima(f, h, conn) >= f).all()
        last = g
    span = int(f.max() - f.min())
    assert (rr.hmaxima(f, span, conn) == f.min()).all() and (rr.hmaxima(f, span + 7, conn) == f.max() - span - 7).all()
    assert len(np.unique(rr.hmaxima(f, span - 1, conn))) > 1
    assert np.array_equal(m.hmaxima(f, 0, conn), f) and np.array_equal(m.hminima(f, 0, conn), f) and (m.hmaxima(f, 5, conn) <= f).all()
    assert (m.hmaxima(f, span, conn) == f.min()).all() and len(np.unique(m.hmaxima(f, span - 1, conn))) > 1
    # a peak of dynamic d is an extended maximum for h < d and stops being one at h = d: two peaks of 9 and 6 over a saddle of 4; above
    # every peak the whole line is one plateau
    line = np.array([0, 9, 4, 6, 0], np.int32).reshape(1, 1, 5)
    assert [int(rr.extended_maxima(line, h, conn).sum()) for h in (0, 1, 2, 3, 50)] == [2, 2, 1, 1, 5]
    assert rr.extended_maxima(line, 1, conn).reshape(-1).tolist() == [0, 1, 0, 1, 0] and rr.extended_maxima(line, 2, conn).reshape(-1).tolist() == [0, 1, 0, 0, 0]
    assert [int(rr.extended_minima(~line, h, conn).sum()) for h in (0, 1, 2, 3, 50)] == [2, 2, 1, 1, 5]
    assert [int(m.extended_maxima(line, h, conn).sum()) for h in (0, 1, 2, 3, 50)] == [2, 2, 1, 1, 5]
    assert [int(m.extended_minima(~line, h, conn).sum()) for h in (0, 1, 2, 3, 50)] == [2, 2, 1, 1, 5]


def test_the_landscape_is_the_exact_integer_square_root():
    from interactive_unet import reconstruction
    d2 = landscape_values()
    for scale in (1, 4, 256):
        got = reconstruction._host_landscape(d2, scale)
        want = rr.landscape_of(d2, scale)
        assert got.dtype == np.int32 and np.array_equal(got, want), scale
        for d in (1, 2, 3, 46340 ** 2 - 1, 46340 ** 2, HIGH):
            assert want[d2 == d][0] == math.isqrt(scale * scale * d)
        assert (want[d2 == 0] == LOW).all() and (want[d2 > 0] >= scale).all()


def test_the_planted_case():
    """Count by count, on the restatement and on the module's numpy path."""
    from interactive_unet import reconstruction as m
    v = planted()
    a = v == 1
    assert a.sum() == 6149 and rr.components_of(a, 6)[1] == 2
    # the contrast: no radius of a plain erosion gives the three grains
    d_out = rr.feature_of(~a)[0]
    assert [rr.components_of(d_out > r * r, 6)[1] for r in (3, 4, 5, 6)] == [2, 1, 1, 2]
    for h in (0.25, 0.5, 1, 2, 3):
        assert rr.hmax_markers(v, 1, h)[1] == 3 and m.hmax_markers(v, 1, h)[1] == 3, h
    for h in (3.25, 4, 20):
        assert rr.hmax_markers(v, 1, h)[1] == 2 and m.hmax_markers(v, 1, h)[1] == 2, h
    labels, k, km, ka = rr.split_touching(v, 1, 2, 6, 'chamfer', parts=True)
    assert (k, km, ka) == (3, 3, 2) and np.bincount(labels.reshape(-1))[1:].tolist() == [123, 3013, 3013]
    assert np.array_equal(labels > 0, a) and labels[8, 8, 40] == 1 and labels[24, 24, 14] == 2 and labels[24, 24, 29] == 3
    got, count = m.split_touching(v, 1, 2, 6, 'chamfer')
    assert count == 3 and np.bincount(got.reshape(-1))[1:].tolist() == [123, 3013, 3013] and np.array_equal(got, labels)


@pytest.mark.parametrize('conn', (6, 26))
@pytest.mark.parametrize('density', (0.5, 0.7))
def test_the_invariants_on_random_blobs(density, conn):
    """On the restatement; the module's numpy path gives the same maps, so the invariants hold for it too."""
    from interactive_unet import reconstruction as m
    v = blobs((20, 24, 40), density, int(density * 10))
    a = v == 1
    objects, ka = rr.components_of(a, conn)
    assert ka >= 1
    for h in (0, 0.5, 1.5, 25):
        markers, km = rr.hmax_markers(v, 1, h, conn)
        assert not markers[~a].any()
        assert len(np.unique(objects[markers > 0])) == ka                 # every component of A holds a marker
        assert km >= ka
        labels, k = rr.split_touching(v, 1, h, conn)
        assert labels.dtype == np.int32 and np.array_equal(labels > 0, a) # labels > 0 exactly on A
        pairs = np.unique(np.stack([labels[a], objects[a]]), axis=1)      # no label spans two components of A
        assert len(np.unique(pairs[0])) == pairs.shape[1] == k == km
        got = m.hmax_markers(v, 1, h, conn)
        assert got[1] == km and got[0].dtype == np.int32 and np.array_equal(got[0], markers), (density, conn, h)
        got = m.split_touching(v, 1, h, conn)
        assert got[1] == k and got[0].dtype == np.int32 and np.array_equal(got[0], labels), (density, conn, h)
        if h == 25:                                                       # above every peak: one marker per component, components.label's numbering
            assert km == ka and np.array_equal(markers, objects) and np.array_equal(labels, objects)


def _maps():
    rng = np.random.default_rng(8)
    yield tuple(rng.integers(-6, 7, (6, 7, 9)).astype(np.int32) for _ in range(2))
    yield tuple(rng.integers(LOW, HIGH + 1, (4, 5, 6)).astype(np.int32) for _ in range(2))
    yield np.zeros((1, 1, 1), np.int32), np.ones((1, 1, 1), np.int32)
    yield tuple(rng.integers(-2, 3, (1, 1, 30)).astype(np.int32) for _ in range(2))


def test_the_numpy_path_is_the_definition():
    """Function by function against the restatement.  The module's sweeps are written like the restatement's (the same offsets in the
    same order, in place), so for `reconstruct` this compares two texts of one form; what holds either of them to an independent
    definition is the level-set test above, which runs both."""
    from interactive_unet import reconstruction as m
    assert m.OFF == rr.OFF == LOW and m.METHODS == ('dilation', 'erosion')
    for marker, mask in _maps():
        keep = marker.copy(), mask.copy()
        for conn in CONNS:
            for h in (0, 1, 3, HIGH):
                for method in m.METHODS:
                    got = m.reconstruct(marker, mask, conn, method, h)
                    assert got.dtype == np.int32 and np.array_equal(got, rr.reconstruct(marker, mask, conn, method == 'erosion', h)), (conn, h, method)
                if h < HIGH:
                    for name in ('hmaxima', 'hminima', 'extended_maxima', 'extended_minima'):
                        got = getattr(m, name)(mask, h, conn)
                        assert got.dtype == getattr(rr, name)(mask, h, conn).dtype and np.array_equal(got, getattr(rr, name)(mask, h, conn)), (name, conn, h)
            for name in ('regional_maxima', 'regional_minima'):
                got = getattr(m, name)(mask, conn)
                assert got.dtype == np.uint8 and np.array_equal(got, getattr(rr, name)(mask, conn)), (name, conn)
        assert np.array_equal(marker, keep[0]) and np.array_equal(mask, keep[1])
    assert np.array_equal(m.reconstruct(*list(_maps())[0]), rr.reconstruct(*list(_maps())[0]))      # the defaults
    for v, target in ((np.ascontiguousarray(planted()[16:34, 14:34, :]), 1), (blobs((9, 14, 30), 0.5, 3), 1), (random_pred((7, 9, 12), 3, 1), 0), (random_pred((7, 9, 12), 2, 4), 1),
                      (np.zeros((3, 4, 5), np.uint8), 1), (np.ones((2, 3, 4), np.uint8), 1), (np.ones((1, 1, 1), np.uint8), 1)):
        for scale in (1, 4):
            f = m.distance_landscape(v, target, scale)
            assert f.dtype == np.int32 and np.array_equal(f, rr.distance_landscape(v, target, scale))
        for conn in CONNS:
            for h in (0, 0.5, 2):
                labels, k = m.hmax_markers(v, target, h, conn)
                want, kw = rr.hmax_markers(v, target, h, conn)
                assert labels.dtype == np.int32 and k == kw and np.array_equal(labels, want), (v.shape, target, conn, h)
                for metric in ('chamfer', 6):
                    labels, k = m.split_touching(v, target, h, conn, metric)
                    want, kw = rr.split_touching(v, target, h, conn, metric)
                    assert labels.dtype == np.int32 and k == kw and np.array_equal(labels, want), (v.shape, target, conn, h, metric)
    v = planted()
    labels, k = m.split_touching(v, 1, 2)
    assert k == 3 and np.bincount(labels.reshape(-1))[1:].tolist() == [123, 3013, 3013]
    assert m.hmax_markers(v, 1, 3)[1] == 3 and m.hmax_markers(v, 1, 3.25)[1] == 2
    # max_rounds: a corridor of plateau takes as many sweeps as it is long
    mask = np.full((1, 1, 40), 5, np.int32)
    marker = np.full((1, 1, 40), LOW, np.int32)
    marker[0, 0, -1] = 5                                                  # against the sweeps' own direction: one voxel a sweep
    with pytest.raises(RuntimeError, match='max_rounds'):
        m.reconstruct(marker, mask, max_rounds=5)
    assert (m.reconstruct(marker, mask, max_rounds=41) == 5).all()


def test_host_refusals_need_no_device():
    from interactive_unet import reconstruction as m
    f = np.zeros((4, 5, 6), np.int32)
    v = np.zeros((4, 5, 6), np.uint8)
    bad_maps = (f.astype(np.uint8), f.astype(np.int64), f[0], f[None], f[:, :, ::2], np.zeros((0, 5, 6), np.int32), torch.from_numpy(f), f.tolist(), None,
                np.empty((1291, 1291, 1291), np.int32))                   # more than 2^31 - 1 voxels (never touched)
    for bad in bad_maps:
        for call in (lambda x: m.reconstruct(f, x), lambda x: m.hmaxima(x, 1), lambda x: m.hminima(x, 1), lambda x: m.regional_maxima(x),
                     lambda x: m.regional_minima(x), lambda x: m.extended_maxima(x, 1), lambda x: m.extended_minima(x, 1)):
            with pytest.raises(ValueError):
                call(bad)
    for bad in bad_maps[:-1] + (np.zeros((4, 5, 7), np.int32), np.zeros((5, 4, 6), np.int32)):
        with pytest.raises(ValueError, match='marker'):
            m.reconstruct(bad, f)
    for bad in (v.astype(np.int32), v[0], np.zeros((4, 5, 6, 1), np.uint8), np.zeros((4, 5, 6, 17), np.uint8), v[:, :, ::2], np.zeros((0, 5, 6), np.uint8),
                torch.from_numpy(v), v.tolist(), None, np.empty((1291, 1291, 1291), np.uint8)):
        for call in (lambda x: m.distance_landscape(x), lambda x: m.hmax_markers(x, 1, 1), lambda x: m.split_touching(x, 1, 1)):
            with pytest.raises(ValueError):
                call(bad)
    with pytest.raises(ValueError, match='diagonal'):
        m.split_touching(np.empty((46342, 1, 1), np.uint8), 1, 1)         # the landscape is a Euclidean distance
    for conn in (0, 4, 8, 27, None):
        for call in (lambda: m.reconstruct(f, f, conn), lambda: m.hmaxima(f, 1, conn), lambda: m.regional_minima(f, conn), lambda: m.extended_maxima(f, 1, conn),
                     lambda: m.hmax_markers(v, 1, 1, conn), lambda: m.split_touching(v, 1, 1, conn)):
            with pytest.raises(ValueError, match='connectivity'):
                call()
    for method in ('dilate', 0, None, True):
        with pytest.raises(ValueError, match='method'):
            m.reconstruct(f, f, 6, method)
    for h in (-1, 1.0, 2 ** 31, True, 'a', None):
        for call in (lambda: m.reconstruct(f, f, h=h), lambda: m.hmaxima(f, h), lambda: m.hminima(f, h), lambda: m.extended_maxima(f, h), lambda: m.extended_minima(f, h)):
            with pytest.raises(ValueError, match='h '):
                call()
    for h, scale in ((-1, 4), (-0.5, 4), (float('nan'), 4), (float('inf'), 4), ('a', 4), (None, 4), (True, 4), (2 ** 29, 4), ((2 ** 31 - 1) / 4, 4), (2 ** 31 - 1, 1)):
        for call in (lambda: m.hmax_markers(v, 1, h, 6, scale), lambda: m.split_touching(v, 1, h, 6, 'chamfer', scale)):
            with pytest.raises(ValueError, match='h '):
                call()
    assert m._height_voxels(2 ** 31 - 2, 1) == 2 ** 31 - 2 and m._height_voxels((2 ** 31 - 2) / 4, 4) == 2 ** 31 - 2 and m._height_voxels(0.124, 4) == 0
    assert m._height_voxels(0.125, 4) == 1 and m._height_voxels(3.25, 4) == 13 and rr.h_int(0.125, 4) == 1 and rr.h_int(3.25, 4) == 13
    for scale in (0, 257, -1, 1.0, True, None):
        for call in (lambda: m.distance_landscape(v, 1, scale), lambda: m.hmax_markers(v, 1, 1, 6, scale), lambda: m.split_touching(v, 1, 1, 6, 'chamfer', scale)):
            with pytest.raises(ValueError, match='scale'):
                call()
    for target in (-1, 256, 1.0, True, 'a'):
        for call in (lambda: m.distance_landscape(v, target), lambda: m.hmax_markers(v, target, 1), lambda: m.split_touching(v, target, 1)):
            with pytest.raises(ValueError, match='target'):
                call()
    for metric in (0, 7, 'euclid', None, (1, 1), (0, 1, 1), (256, 0, 0)):
        with pytest.raises(ValueError, match='metric'):
            m.split_touching(v, 1, 1, 6, metric)
    with pytest.raises(TypeError):
        m.hmax_markers(v, 1, 1, max_rounds=3)                             # the markers take no max_rounds
    for rounds in (0, -1, 1.5, True, 'a'):
        for call in (lambda: m.reconstruct(f, f, max_rounds=rounds), lambda: m.hmaxima(f, 1, max_rounds=rounds), lambda: m.regional_maxima(f, max_rounds=rounds),
                     lambda: m.extended_minima(f, 1, max_rounds=rounds),
                     lambda: m.split_touching(v, 1, 1, max_rounds=rounds)):
            with pytest.raises(ValueError, match='max_rounds'):
                call()
    with pytest.raises(ValueError, match='2\\^31 - 2'):                   # the growth's overflow limit: a chamfer run of 1024 x 1024 x 1000 (never touched)
        m.split_touching(np.empty((1000, 1024, 1024), np.uint8), 1, 1)


def test_the_module_goes_with_the_overlay():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import install_overlay
    assert 'reconstruction' in install_overlay.ADDED


def test_limits_and_refusals_through_the_library_without_a_gpu():
    """Argument validation precedes every HIP call."""
    from interactive_unet import _native as nv
    if not os.path.isfile(nv.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    l = nv.lib()
    need = l.iunet_rec_ws_bytes
    a16 = lambda n: (n + 15) // 16 * 16
    tiles = lambda Z, Y, X: ((Z + 7) // 8) * ((Y + 7) // 8) * ((X + 63) // 64)
    want = lambda Z, Y, X: 2 * a16(4 * tiles(Z, Y, X))
    assert need(1, 1, 1) == 32 and need(37, 41, 150) == want(37, 41, 150) == 2 * a16(4 * 5 * 6 * 3)
    for shape in ((8, 8, 64), (9, 8, 64), (8, 9, 65), (1, 1, 300), (2100, 3, 5), (1024, 1024, 1024), (2047, 1024, 1024), (2 ** 31 - 1, 1, 1), (1, 2 ** 31 - 1, 1),
                  (1, 1, 2 ** 31 - 1), (46342, 1, 1)):
        assert need(*shape) == want(*shape) > 0, shape
    assert need(0, 4, 4) == 0 and need(4, -1, 4) == 0 and need(4, 4, 0) == 0
    assert need(2048, 1024, 1024) == 0 and need(2 ** 16, 2 ** 15, 1) == 0 and need(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1) == 0      # Z Y X = 2^31 and far past it

    mem = (ctypes.c_double * 64)()
    at = lambda n: ctypes.c_void_p(ctypes.addressof(mem) + n)                          # never dereferenced: every call below stops before its launch
    M = 1 << 20
    buf, far, further, fourth, odd, odd8 = at(0), at(M), at(2 * M), at(3 * M), at(2), at(8)
    n8 = need(8, 8, 8)
    assert n8 == 32
    big = dict(Z=2048, Y=1024, X=1024)

    def landscape(d2=far, Z=8, Y=8, X=8, scale=4, off=LOW, f=further):
        return l.iunet_rec_landscape(d2, Z, Y, X, scale, off, f, None), l.iunet_last_error()
    for kw, word in ((dict(d2=None), b'null'), (dict(f=None), b'null'), (dict(Z=0), b'dimension'), (dict(Y=-3), b'dimension'), (dict(X=0), b'dimension'),
                     (big, b'voxels'), (dict(scale=0), b'scale'), (dict(scale=257), b'scale'), (dict(scale=-4), b'scale'),
                     (dict(d2=at(M + 2)), b'aligned'), (dict(f=at(2 * M + 1)), b'aligned'),
                     (dict(f=at(M + 4)), b'overlap'), (dict(f=at(M + 4 * 511)), b'overlap'), (dict(f=at(M - 4)), b'overlap')):
        rc, msg = landscape(**kw)
        assert rc < 0 and word in msg and msg.startswith(b'rec_landscape:'), (kw, msg)

    def init(marker=far, mask=further, Z=8, Y=8, X=8, h=0, erosion=0, r=fourth, ws=buf, ws_bytes=None):
        ws_bytes = need(Z, Y, X) if ws_bytes is None else ws_bytes
        return l.iunet_rec_init(marker, mask, Z, Y, X, h, erosion, r, ws, ws_bytes, None), l.iunet_last_error()
    for kw, word in ((dict(marker=None), b'null'), (dict(mask=None), b'null'), (dict(r=None), b'null'), (dict(ws=None), b'null'),
                     (dict(Z=0), b'dimension'), (dict(X=-1), b'dimension'), (dict(ws_bytes=1 << 40, **big), b'voxels'),
                     (dict(h=-1), b'h '), (dict(h=LOW), b'h '), (dict(erosion=2), b'erosion'), (dict(erosion=-1), b'erosion'),
                     (dict(ws_bytes=n8 - 1), b'workspace'), (dict(ws_bytes=0), b'workspace'), (dict(ws=odd8), b'aligned'), (dict(ws=odd), b'aligned'),
                     (dict(marker=at(M + 2)), b'aligned'), (dict(mask=at(2 * M + 2)), b'aligned'), (dict(r=at(3 * M + 2)), b'aligned'),
                     (dict(r=far), b'overlap'), (dict(r=further), b'overlap'), (dict(r=at(M + 4 * 511)), b'overlap'), (dict(r=at(2 * M - 4)), b'overlap'),
                     (dict(r=at(16)), b'overlap'), (dict(r=at(-2044)), b'overlap')):
        rc, msg = init(**kw)
        assert rc < 0 and word in msg and msg.startswith(b'rec_init:'), (kw, msg)
    # what is allowed gets as far as the workspace: marker is mask, the largest h, the largest volume
    for kw in (dict(marker=further), dict(h=HIGH), dict(erosion=1), dict(Z=2047, Y=1024, X=1024), dict(Z=2 ** 31 - 1, Y=1, X=1)):
        rc, msg = init(ws_bytes=0, **kw)
        assert rc < 0 and b'workspace' in msg, (kw, msg)

    def relax(r=far, mask=further, Z=8, Y=8, X=8, conn=6, erosion=0, rounds=1, changed=fourth, ws=buf, ws_bytes=None):
        ws_bytes = need(Z, Y, X) if ws_bytes is None else ws_bytes
        return l.iunet_rec_relax(r, mask, Z, Y, X, conn, erosion, rounds, changed, ws, ws_bytes, None), l.iunet_last_error()
    for kw, word in ((dict(r=None), b'null'), (dict(mask=None), b'null'), (dict(changed=None), b'null'), (dict(ws=None), b'null'),
                     (dict(Y=0), b'dimension'), (dict(ws_bytes=1 << 40, **big), b'voxels'),
                     (dict(conn=0), b'connectivity'), (dict(conn=8), b'connectivity'), (dict(conn=27), b'connectivity'), (dict(conn=-6), b'connectivity'),
                     (dict(erosion=2), b'erosion'), (dict(erosion=-1), b'erosion'),
                     (dict(rounds=0), b'rounds'), (dict(rounds=-1), b'rounds'), (dict(rounds=1025), b'rounds'),
                     (dict(ws_bytes=n8 - 1), b'workspace'), (dict(ws=odd8), b'aligned'), (dict(r=at(M + 2)), b'aligned'), (dict(mask=at(2 * M + 2)), b'aligned'),
                     (dict(changed=at(3 * M + 2)), b'aligned'),
                     (dict(changed=buf), b'overlap'), (dict(changed=at(n8 - 4)), b'overlap'), (dict(changed=far), b'overlap'), (dict(changed=at(M + 4 * 511)), b'overlap'),
                     (dict(r=further), b'overlap'), (dict(mask=at(M + 4 * 511)), b'overlap'), (dict(r=at(16)), b'overlap'), (dict(r=at(-2044)), b'overlap')):
        rc, msg = relax(**kw)
        assert rc < 0 and word in msg and msg.startswith(b'rec_relax:'), (kw, msg)
    for kw in (dict(conn=18), dict(conn=26, erosion=1), dict(rounds=1024), dict(Z=2047, Y=1024, X=1024), dict(Z=1, Y=1, X=2 ** 31 - 1)):
        rc, msg = relax(ws_bytes=0, **kw)
        assert rc < 0 and b'workspace' in msg, (kw, msg)

    def select(a=far, b=further, Z=8, Y=8, X=8, t=1, value=1, out=fourth):
        return l.iunet_rec_select(a, b, Z, Y, X, t, value, out, None), l.iunet_last_error()
    for kw, word in ((dict(a=None), b'null'), (dict(b=None), b'null'), (dict(out=None), b'null'), (dict(Z=0), b'dimension'), (big, b'voxels'),
                     (dict(value=-1), b'value'), (dict(value=256), b'value'), (dict(a=at(M + 2)), b'aligned'), (dict(b=at(2 * M + 1)), b'aligned'),
                     (dict(out=far), b'overlap'), (dict(out=at(M + 2047)), b'overlap'), (dict(out=at(M - 1)), b'overlap'), (dict(out=further), b'overlap'),
                     (dict(out=at(2 * M + 5)), b'overlap')):
        rc, msg = select(**kw)
        assert rc < 0 and word in msg and msg.startswith(b'rec_select:'), (kw, msg)
