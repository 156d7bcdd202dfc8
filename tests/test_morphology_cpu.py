"""Distance transform and ball morphology without a GPU: the definition tests/morphology_ref.py against a brute-force
minimum, closed forms and scipy's binary operators; the host layer's numpy path against the definition; the host refusals; the limits and
the entry points' argument checks through the built library; and the two facts tests/test_gpu_morphology.py leans on (the condition of its
sparse input, the crop argument of its volume-scale case)."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import morphology_ref as mr
from tests.volume_inputs import random_pred

CONN = (6, 18, 26)
RADII = (0, 1, 1.5, 2, 3)


def blobs(shape, seed):
    """A planted class map: balls of classes 1 and 2 on background 0, one-voxel bridges between some of them, pin-holes knocked out."""
    rng = np.random.default_rng(seed)
    Z, Y, X = shape
    zz, yy, xx = np.indices(shape)
    v = np.zeros(shape, np.uint8)
    centres = []
    for k in range(max(3, int(np.prod(shape)) // 4000)):
        c = (int(rng.integers(0, Z)), int(rng.integers(0, Y)), int(rng.integers(0, X)))
        r = float(rng.integers(2, 7))
        v[(zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= r * r] = 1 if k % 3 else 2
        centres.append(c)
    for a, b in zip(centres[::2], centres[1::2]):                              # a bridge along x, then a thin wall piece along y
        v[a[0], a[1], min(a[2], b[2]):max(a[2], b[2]) + 1] = 1
        v[a[0], min(a[1], b[1]):max(a[1], b[1]) + 1, b[2]] = 1
    v[rng.random(shape) < 0.01] = 0                                            # pin-holes
    return v


def ball(r2):
    R = int(math.isqrt(r2))
    g = np.arange(-R, R + 1)
    return (g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2) <= r2


def holes_volume():
    """Class 1 shells on background 0: a closed hollow box; one open to the face x = 0 (not filled); one whose hole holds a voxel of a third
    class (filled); one with a corner voxel missing, open under the 26-neighbourhood only."""
    v = np.zeros((12, 16, 30), np.uint8)

    def shell(z, y, x, n=6):
        v[z:z + n, y:y + n, x:x + n] = 1
        v[z + 1:z + n - 1, y + 1:y + n - 1, x + 1:x + n - 1] = 0
    shell(2, 2, 2)
    shell(2, 9, 0)
    v[3:7, 10:14, 0] = 0
    shell(2, 2, 12)
    v[4, 4, 14] = 2
    shell(2, 2, 22)
    v[2, 2, 22] = 0
    return v


def lattice_axis(n, step):
    """bool [n]: the multiples of `step` and the axis' last index -- the lattice of the volume-scale test along one axis, closed at the far
    face so that no index is further than step // 2 from it."""
    on = np.arange(n) % step == 0
    on[-1] = True
    return on


def sparse_input():
    return np.random.default_rng(40).random((37, 41, 150)) < 0.0005


def _brute(seeds):
    at = np.argwhere(seeds).astype(np.int64)
    pos = np.stack(np.indices(seeds.shape), axis=-1).reshape(-1, 1, 3).astype(np.int64)
    if len(at) == 0:
        return np.full(seeds.shape, mr.INF, np.int32)
    return ((pos - at[None]) ** 2).sum(-1).min(axis=1).reshape(seeds.shape).astype(np.int32)


@pytest.mark.parametrize('shape', ((9, 11, 23), (1, 1, 40), (7, 1, 5), (1, 1, 1)))
def test_the_definition_is_the_brute_force_minimum(shape):
    rng = np.random.default_rng(sum(shape))
    for p in (0.5, 0.05, 0.005):
        v = (rng.random(shape) < p).astype(np.uint8)
        for target, invert in ((1, False), (1, True), (0, False)):
            a = v == target
            got = mr.distance_sq(v, target, invert)
            assert got.dtype == np.int32 and np.array_equal(got, _brute(~a if invert else a)), (shape, p, target, invert)
    pred = random_pred(shape, 3, 1)
    has, cls = pred.max(-1) > 0, pred.argmax(-1)
    for target in (0, 1, 5):
        a = has & (cls == target)
        assert np.array_equal(mr.distance_sq(pred, target, False), _brute(a)) and np.array_equal(mr.distance_sq(pred, target, True), _brute(~a))


def test_no_seed_all_seeds_and_one_seed_at_the_origin():
    shape = (9, 11, 23)
    assert (mr.distance_sq(np.zeros(shape, np.uint8), 1) == mr.INF).all() and mr.INF == 2 ** 31 - 1
    assert not mr.distance_sq(np.ones(shape, np.uint8), 1).any()
    v = np.zeros(shape, np.uint8)
    v[0, 0, 0] = 1
    z, y, x = np.indices(shape)
    assert np.array_equal(mr.distance_sq(v, 1), z * z + y * y + x * x)
    assert (mr.distance_sq(np.zeros(shape + (3,), np.uint8), 0) == mr.INF).all()      # never predicted: no member of class 0
    assert not mr.distance_sq(np.zeros(shape + (3,), np.uint8), 0, True).any()
    assert mr.radius_sq(1.5) == 2 and mr.radius_sq(0) == 0 and mr.radius_sq(3) == 9 and mr.radius_sq(46340.9) == 2147479012


@pytest.mark.parametrize('radius', RADII)
def test_ball_morphology_is_scipys_binary_operators(radius):
    r2 = mr.radius_sq(radius)
    st = ball(r2)
    for shape, seed in (((20, 24, 40), 0), ((9, 30, 31), 1), ((1, 25, 40), 2)):
        v = blobs(shape, seed)
        a = v == 1
        assert a.any() and (v == 2).any() and not a.all()
        d = ndimage.binary_dilation(a, st)
        e = ndimage.binary_erosion(a, st, border_value=1)
        o = ndimage.binary_dilation(e, st)
        c = ndimage.binary_erosion(d, st, border_value=1)
        assert np.array_equal(mr.dilate(v, 1, radius), np.where(d, 1, v))
        assert np.array_equal(mr.erode(v, 1, radius, 7), np.where(a & ~e, 7, v))
        assert np.array_equal(mr.opening(v, 1, radius, 7), np.where(a & ~o, 7, v))
        assert np.array_equal(mr.closing(v, 1, radius), np.where(c, 1, v))
        assert not (o & ~a).any() and not (a & ~c).any()
        if radius == 0:
            for got in (mr.dilate(v, 1, 0), mr.erode(v, 1, 0, 7), mr.opening(v, 1, 0, 7), mr.closing(v, 1, 0)):
                assert np.array_equal(got, v)
        elif shape[0] > 1:
            assert (e != a).any() and (d != a).any() and (o != a).any() and (c != a).any()     # the blobs do have bridges and pin-holes


@pytest.mark.parametrize('conn', CONN)
def test_fill_holes_is_scipys(conn):
    v = holes_volume()
    a = v == 1
    want = ndimage.binary_fill_holes(a, structure=ndimage.generate_binary_structure(3, mr.RANK[conn]))
    got = mr.fill_holes(v, 1, conn)
    assert np.array_equal(got, np.where(want, 1, v))
    assert (got[3:7, 3:7, 3:7] == 1).all()                       # the closed box
    assert not got[3:7, 10:14, 0:5].any()                        # the one open to a face
    assert (got[3:7, 3:7, 13:17] == 1).all() and v[4, 4, 14] == 2   # the hole with a voxel of a third class
    assert (got[3:7, 3:7, 23:27] == 1).all() == (conn != 26)     # the missing corner opens it at 26 only


def _host_cases():
    yield blobs((9, 14, 30), 3)
    yield random_pred((7, 9, 12), 2, 4)
    yield random_pred((7, 9, 12), 5, 5)
    yield np.zeros((3, 4, 5), np.uint8)
    yield np.ones((1, 1, 1), np.uint8)


def test_the_numpy_path_is_the_definition():
    from interactive_unet import morphology
    for v in _host_cases():
        assert np.array_equal(morphology.class_map(v), mr.class_map(v)[0]) and morphology.class_map(v).dtype == np.uint8
        for target in (0, 1, 3):
            for invert in (False, True):
                got = morphology.distance_sq(v, target, invert)
                assert got.dtype == np.int32 and np.array_equal(got, mr.distance_sq(v, target, invert))
            for radius in (0, 1, 1.5, 3):
                for got, want in ((morphology.dilate(v, target, radius), mr.dilate(v, target, radius)),
                                  (morphology.erode(v, target, radius, 7), mr.erode(v, target, radius, 7)),
                                  (morphology.opening(v, target, radius, 7), mr.opening(v, target, radius, 7)),
                                  (morphology.closing(v, target, radius), mr.closing(v, target, radius))):
                    assert got.dtype == np.uint8 and np.array_equal(got, want), (v.shape, target, radius)
            for conn in CONN:
                assert np.array_equal(morphology.fill_holes(v, target, conn), mr.fill_holes(v, target, conn))
    for conn in CONN:
        assert np.array_equal(morphology.fill_holes(holes_volume(), 1, conn), mr.fill_holes(holes_volume(), 1, conn))
    assert morphology.INF == mr.INF


def test_host_refusals_need_no_device():
    from interactive_unet import morphology as m
    v = np.zeros((4, 5, 6), np.uint8)
    pred = np.zeros((4, 5, 6, 3), np.uint8)
    calls = (lambda s: m.distance_sq(s), lambda s: m.class_map(s), lambda s: m.dilate(s, 1, 1), lambda s: m.erode(s, 1, 1),
             lambda s: m.opening(s, 1, 1), lambda s: m.closing(s, 1, 1), lambda s: m.fill_holes(s, 1))
    for bad in (v.astype(np.int32), v[0], pred[..., :1], np.zeros((4, 5, 6, 17), np.uint8), v[:, :, ::2], np.zeros((0, 5, 6), np.uint8),
                torch.from_numpy(v), v.tolist(), None,
                np.empty((46342, 1, 1), np.uint8),                              # the squared diagonal
                np.empty((1291, 1291, 1291), np.uint8)):                        # more than 2^31 - 1 voxels (never touched)
        for call in calls:
            with pytest.raises(ValueError):
                call(bad)
    assert m.class_map(np.zeros((46341, 1, 1), np.uint8)).shape == (46341, 1, 1)
    for target in (-1, 256, 1.0, True, 'a'):
        for call in (lambda: m.distance_sq(v, target), lambda: m.dilate(v, target, 1), lambda: m.erode(v, target, 1),
                     lambda: m.opening(v, target, 1), lambda: m.closing(v, target, 1), lambda: m.fill_holes(v, target)):
            with pytest.raises(ValueError, match='target'):
                call()
    for fill in (-1, 256, 1.5):
        with pytest.raises(ValueError, match='fill'):
            m.erode(v, 1, 1, fill)
        with pytest.raises(ValueError, match='fill'):
            m.opening(v, 1, 1, fill)
    for radius in (-1, -0.5, float('nan'), float('inf'), 46341, 'r', None, True):
        for call in (lambda: m.dilate(v, 1, radius), lambda: m.erode(v, 1, radius), lambda: m.opening(v, 1, radius), lambda: m.closing(v, 1, radius)):
            with pytest.raises(ValueError, match='radius'):
                call()
    for conn in (0, 4, 8, 27):
        with pytest.raises(ValueError, match='connectivity'):
            m.fill_holes(v, 1, conn)


def test_limits_and_refusals_through_the_library_without_a_gpu():
    """Argument validation precedes every HIP call."""
    from interactive_unet import _native as nv
    if not os.path.isfile(nv.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    l = nv.lib()
    need = l.iunet_edt_ws_bytes
    a16 = lambda n: (n + 15) // 16 * 16
    assert need(46341, 1, 1) > 0 and need(1, 1, 1) == 16 and need(37, 41, 150) == a16(8 * 227550)
    assert need(1030, 1024, 1024) == 8 * 1030 * 2 ** 20 and need(32768, 32768, 1) > 0 and need(2047, 1024, 1024) > 0
    assert need(46342, 1, 1) == 0 and need(0, 4, 4) == 0 and need(4, -1, 4) == 0 and need(4, 4, 0) == 0
    assert need(2048, 1024, 1024) == 0 and need(2 ** 16, 2 ** 15, 1) == 0                    # Z Y X = 2^31
    assert need(32769, 32769, 1) == 0                                                         # the squared diagonal: 2 * 32768^2 = 2^31

    mem = (ctypes.c_double * 64)()
    buf = ctypes.c_void_p(ctypes.addressof(mem))                                      # never dereferenced: every call below stops before its launch
    far = ctypes.c_void_p(ctypes.addressof(mem) + 4096 * 4)
    odd = ctypes.c_void_p(ctypes.addressof(mem) + 2)

    def sq(src=buf, Z=8, Y=8, X=8, C=1, target=1, invert=0, d2=buf, cls=None, ws=buf, ws_bytes=None):
        ws_bytes = need(Z, Y, X) if ws_bytes is None else ws_bytes
        return l.iunet_edt_sq(src, Z, Y, X, C, target, invert, d2, cls, ws, ws_bytes, None), l.iunet_last_error()
    for kw, word in ((dict(src=None), b'null'), (dict(d2=None), b'null'), (dict(ws=None), b'null'), (dict(Z=0), b'dimension'),
                     (dict(Y=-3), b'dimension'), (dict(X=0), b'dimension'), (dict(Z=2048, Y=1024, X=1024, ws_bytes=1 << 40), b'voxels'),
                     (dict(Z=46342, Y=1, X=1, ws_bytes=1 << 40), b'diagonal'), (dict(C=0), b'classes'), (dict(C=17), b'classes'),
                     (dict(target=-1), b'target'), (dict(target=256), b'target'), (dict(invert=2), b'invert'), (dict(invert=-1), b'invert'),
                     (dict(ws_bytes=need(8, 8, 8) - 1), b'workspace'), (dict(ws_bytes=0), b'workspace'), (dict(d2=odd), b'aligned'),
                     (dict(ws=odd), b'aligned')):
        rc, msg = sq(**kw)
        assert rc < 0 and word in msg, (kw, msg)
    assert b'null' in sq(None, 0, 0, 0, 0, 0, 0, None, None, None, 0)[1]

    def mask(prev=buf, Z=8, Y=8, X=8, r2=4, above=1, d2=far, ws=buf, ws_bytes=None):
        ws_bytes = need(Z, Y, X) if ws_bytes is None else ws_bytes
        return l.iunet_edt_sq_mask(prev, Z, Y, X, r2, above, d2, ws, ws_bytes, None), l.iunet_last_error()
    for kw, word in ((dict(prev=None), b'null'), (dict(d2=None), b'null'), (dict(ws=None), b'null'), (dict(Z=0), b'dimension'),
                     (dict(Z=2048, Y=1024, X=1024, ws_bytes=1 << 40), b'voxels'), (dict(r2=-1), b'r2'), (dict(r2=2 ** 31 - 1), b'r2'),
                     (dict(above=2), b'above'), (dict(ws_bytes=need(8, 8, 8) - 1), b'workspace'), (dict(prev=odd), b'aligned'),
                     (dict(d2=buf), b'overlap'), (dict(d2=ctypes.c_void_p(ctypes.addressof(mem) + 4 * 511)), b'overlap')):
        rc, msg = mask(**kw)
        assert rc < 0 and word in msg, (kw, msg)
    assert b'null' in mask(None, 0, 0, 0, 0, 0, None, None, 0)[1]

    def sel(d2=buf, cls=buf, Z=8, Y=8, X=8, r2=4, above=0, only=-1, value=1, out=buf):
        return l.iunet_edt_select(d2, cls, Z, Y, X, r2, above, only, value, out, None), l.iunet_last_error()
    for kw, word in ((dict(d2=None), b'null'), (dict(cls=None), b'null'), (dict(out=None), b'null'), (dict(Y=0), b'dimension'),
                     (dict(Z=2048, Y=1024, X=1024), b'voxels'), (dict(r2=-1), b'r2'), (dict(r2=2 ** 31 - 1), b'r2'), (dict(above=-1), b'above'),
                     (dict(only=-2), b'only'), (dict(only=256), b'only'), (dict(value=-1), b'value'), (dict(value=256), b'value'),
                     (dict(d2=odd), b'aligned')):
        rc, msg = sel(**kw)
        assert rc < 0 and word in msg, (kw, msg)
    assert b'null' in sel(None, None, 0, 0, 0, 0, 0, 0, 0, None)[1]


def test_the_sparse_gpu_input_has_seedless_rows_and_a_seedless_plane():
    s = sparse_input()
    seeds, rows, planes = int(s.sum()), int((~s.any(axis=2)).sum()), int((~s.any(axis=(1, 2))).sum())
    print(f'sparse input: {seeds} seeds, {rows} seedless rows, {planes} seedless planes')
    assert seeds >= 1 and rows >= 1 and planes >= 1


def test_a_crop_extended_by_the_distance_bound_defines_its_interior():
    """Where every voxel has a seed within squared distance B, the nearest seed of a voxel of a crop lies in the crop extended by
    ceil(sqrt(B)) voxels: the definition on the extended crop (clipped to the volume) equals the volume's on the crop."""
    B = 3 ** 2 + 2 ** 2 + 4 ** 2
    # the bound needs the lattice closed at the far faces: the far corner of the volume-scale shape, 1030 x 1024 x 1024, with and without
    big = (1030, 1024, 1024)
    start = [(m - 20) // step * step for m, step in zip(big, (7, 5, 9))]                # the corner begins on a lattice plane of each axis
    closed = [lattice_axis(m, step)[lo:] for m, step, lo in zip(big, (7, 5, 9), start)]
    opened = [(np.arange(m) % step == 0)[lo:] for m, step, lo in zip(big, (7, 5, 9), start)]
    corner = lambda ax: mr.distance_sq_of(ax[0][:, None, None] & ax[1][None, :, None] & ax[2][None, None, :])
    assert corner(closed).max() <= B and corner(opened).max() == 3 ** 2 + 3 ** 2 + 6 ** 2 == 54
    shape = (30, 28, 40)
    s = (lattice_axis(30, 7)[:, None, None] & lattice_axis(28, 5)[None, :, None] & lattice_axis(40, 9)[None, None, :]) \
        | (np.random.default_rng(6).random(shape) < 0.01)
    whole = mr.distance_sq_of(s)
    assert whole.max() <= B
    m = math.ceil(math.sqrt(B))
    assert m == 6
    for lo in ((0, 0, 0), (9, 8, 13), (18, 16, 28)):
        hi = tuple(a + 12 for a in lo)
        elo = tuple(max(0, a - m) for a in lo)
        ehi = tuple(min(n, b + m) for n, b in zip(shape, hi))
        ext = mr.distance_sq_of(s[elo[0]:ehi[0], elo[1]:ehi[1], elo[2]:ehi[2]])
        inner = ext[lo[0] - elo[0]:hi[0] - elo[0], lo[1] - elo[1]:hi[1] - elo[1], lo[2] - elo[2]:hi[2] - elo[2]]
        assert np.array_equal(inner, whole[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]), lo
    # and an extension short of the bound does not: the argument is needed
    short = mr.distance_sq_of(s[9:21, 8:20, 13:25])
    assert not np.array_equal(short, whole[9:21, 8:20, 13:25])
