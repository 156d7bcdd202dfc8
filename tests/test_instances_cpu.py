"""Nearest-seed feature transform and instance splitting without a GPU: the definition tests/instances_ref.py against
a brute-force minimum over all seeds in raster order, two planted volumes checked voxel count by voxel count, the invariants of
split_touching, expand_labels against a brute force; the host layer's numpy path against the definition; the host refusals; the limits and
the entry points' argument checks through the built library."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import instances_ref as ir
from tests import morphology_ref as mr
from tests.volume_inputs import random_pred


def brute(seeds):
    """(d2, idx): the minimum over all seeds, listed in raster order, and the first of them that attains it."""
    seeds = np.asarray(seeds, dtype=bool)
    at = np.argwhere(seeds).astype(np.int64)                                   # raster order
    if len(at) == 0:
        return np.full(seeds.shape, ir.INF, np.int32), np.full(seeds.shape, -1, np.int32)
    pos = np.stack(np.indices(seeds.shape), axis=-1).reshape(-1, 1, 3).astype(np.int64)
    sq = ((pos - at[None]) ** 2).sum(-1)
    first = sq.argmin(axis=1)                                                  # the first of equal minima: the smallest raster index
    raster = np.flatnonzero(seeds.reshape(-1))
    return sq.min(axis=1).reshape(seeds.shape).astype(np.int32), raster[first].reshape(seeds.shape).astype(np.int32)


def ball(shape, c, r):
    z, y, x = np.indices(shape)
    return (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= r * r


def planted_split():
    """21 x 23 x 60: two touching balls, a small ball, a ball with a thin arm towards the small one.  Three objects."""
    shape = (21, 23, 60)
    a = ball(shape, (10, 10, 8), 6) | ball(shape, (10, 10, 18), 6) | ball(shape, (10, 10, 30), 2) | ball(shape, (10, 10, 50), 6)
    a[10, 10, 36:44] = True
    return a.astype(np.uint8)


def planted_leak():
    """21 x 21 x 50: a ball with a long thin arm whose tip is nearer to the core of a second ball.  Two objects."""
    shape = (21, 21, 50)
    a = ball(shape, (10, 10, 6), 5) | ball(shape, (10, 10, 37), 6)
    a[10, 10, 11:30] = True
    return a.astype(np.uint8)


def grains(shape, seed, p_hole=0.0):
    """Random overlapping balls of class 1 (touching objects), a few of class 2, on background 0."""
    rng = np.random.default_rng(seed)
    v = np.zeros(shape, np.uint8)
    for k in range(max(4, int(np.prod(shape)) // 400)):
        c = [int(rng.integers(0, n)) for n in shape]
        v[ball(shape, c, float(rng.integers(1, 6)))] = 2 if k % 5 == 4 else 1
    if p_hole:
        v[rng.random(shape) < p_hole] = 0
    return v


def check_same(got, want, where):
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[0].flags['C_CONTIGUOUS'] and got[1].flags['C_CONTIGUOUS'], where
    assert np.array_equal(got[0], want[0]), ('d2', where)
    assert np.array_equal(got[1], want[1]), ('idx', where)


@pytest.mark.parametrize('shape', ((9, 11, 23), (5, 7, 6), (1, 1, 30), (4, 1, 9)))
def test_the_definition_is_the_brute_force_minimum_and_its_first_seed(shape):
    rng = np.random.default_rng(sum(shape))
    for p in (0.5, 0.05, 0.01):
        s = rng.random(shape) < p
        check_same(ir.feature_of(s), brute(s), (shape, p))
        v = s.astype(np.uint8)
        check_same(ir.feature(v, 1, True), brute(~s), (shape, p, 'invert'))
        check_same(ir.feature(v, 0, False), brute(~s), (shape, p, 'target 0'))


def test_the_definition_on_a_lattice_of_ties():
    s = np.zeros((9, 10, 12), bool)
    s[::4, ::3, ::5] = True
    d2, idx = ir.feature_of(s)
    check_same((d2, idx), brute(s), 'lattice')
    # more than a fifth of the voxels have several nearest seeds, along every axis
    at = np.argwhere(s).astype(np.int64)
    pos = np.stack(np.indices(s.shape), axis=-1).reshape(-1, 1, 3).astype(np.int64)
    sq = ((pos - at[None]) ** 2).sum(-1)
    assert ((sq == sq.min(axis=1, keepdims=True)).sum(axis=1) > 1).mean() > 0.2


def test_the_definition_on_a_predicted_volume_with_never_predicted_voxels():
    pred = random_pred((7, 9, 12), 3, 1)
    has, cls = pred.max(-1) > 0, pred.argmax(-1)
    assert (~has).any()
    for target in (0, 1, 5):
        a = has & (cls == target)
        check_same(ir.feature(pred, target, False), brute(a), target)
        check_same(ir.feature(pred, target, True), brute(~a), (target, 'invert'))


def test_no_seed_and_all_seeds():
    shape = (5, 6, 7)
    d2, idx = ir.feature_of(np.zeros(shape, bool))
    assert (d2 == ir.INF).all() and (idx == -1).all() and ir.INF == 2 ** 31 - 1
    d2, idx = ir.feature_of(np.ones(shape, bool))
    assert not d2.any() and np.array_equal(idx.reshape(-1), np.arange(5 * 6 * 7))
    s = np.random.default_rng(0).random(shape) < 0.2
    d2, idx = ir.feature_of(s)
    own = np.arange(s.size).reshape(shape)
    assert np.array_equal(idx[s], own[s]) and s.reshape(-1)[idx.reshape(-1)].all()
    assert np.array_equal(ir.feature_mask(d2, 0, False)[0], d2) and np.array_equal(ir.feature_mask(d2, 0, True)[1], brute(~s)[1])


def test_the_planted_split():
    from interactive_unet import components
    v = planted_split()
    a = v == 1
    assert components.label(v)[1] == 3
    labels, k, ke, ka = ir.split_touching(v, 1, 4, 6, parts=True)
    assert (ke, ka, k) == (3, 3, 4)
    assert np.bincount(labels.reshape(-1))[1:].tolist() == [924, 887, 933, 33]
    assert np.array_equal(labels > 0, a)
    assert labels[10, 10, 8] == 1 and labels[10, 10, 18] == 2                   # the two touching balls are separated ...
    assert (labels[:, :, :13][a[:, :, :13]] == 1).all() and (labels[:, :, 14:25][a[:, :, 14:25]] == 2).all()
    assert (labels[ball(a.shape, (10, 10, 30), 2)] == 4).all() and (labels == 4).sum() == 33      # ... the small ball is its own instance
    assert (labels[10, 10, 36:44] == 3).all() and labels[10, 10, 50] == 3       # the arm stays with its ball
    objects = components.label(v)[0]
    for i in range(1, k + 1):                                                   # no voxel outside its own object's cores
        assert len(np.unique(objects[labels == i])) == 1


@pytest.mark.parametrize('radius', (2, 3))
def test_the_leak_case(radius):
    from interactive_unet import components
    v = planted_leak()
    assert components.label(v)[1] == 2
    labels, k, ke, ka = ir.split_touching(v, 1, radius, 6, parts=True)
    assert (ke, ka, k) == (2, 2, 3)
    assert np.bincount(labels.reshape(-1))[1:].tolist() == [925, 525, 8]
    tip = labels == 3                                                           # the remainder of the first object, not part of the second
    assert tip[10, 10, 29] and tip.sum() == tip[10, 10, 11:30].sum() == 8
    assert labels[10, 10, 37] == 1 and labels[10, 10, 6] == 2 and labels[10, 10, 12] == 2
    # and the plain nearest core would have leaked: the tip's nearest core is the second ball's
    a = v == 1
    e = ir.feature_of(~a)[0] > ir.radius_sq(radius)
    _, idx = ir.feature_of(e)
    assert (idx[tip] % 50 > 30).all()


@pytest.mark.parametrize('conn', (6, 26))
def test_the_invariants_of_split_touching(conn):
    for v, target in ((grains((14, 20, 31), 1), 1), (grains((14, 20, 31), 2, 0.02), 1), (planted_split(), 1), (random_pred((7, 9, 12), 3, 1), 0)):
        a = ir.members(v, target)
        objects, ka = ir.components_of(a, conn)
        for radius in (0, 1, 1.5, 3):
            labels, k, ke, ka2 = ir.split_touching(v, target, radius, conn, parts=True)
            assert labels.dtype == np.int32 and ka2 == ka and ka <= k <= ke + ka
            assert np.array_equal(labels > 0, a)                               # labels > 0 exactly on A
            pairs = np.unique(np.stack([labels[a], objects[a]]), axis=1)       # two voxels of different objects never share a label
            assert len(np.unique(pairs[0])) == pairs.shape[1] == k
            firsts = [np.flatnonzero(labels.reshape(-1) == i)[0] for i in range(1, k + 1)]
            assert firsts == sorted(firsts)                                    # numbered in order of the first voxel
    # radius 0 on a volume without one-voxel necks: every object is its own core, the numbering is components.label's
    from interactive_unet import components
    v = grains((14, 20, 31), 1)
    labels, k = ir.split_touching(v, 1, 0, conn)
    want, kw, _ = components.label((v == 1).astype(np.uint8), conn)
    assert k == kw and np.array_equal(labels, want)


def test_split_touching_does_split_the_grains():
    v = grains((14, 20, 31), 1)
    ka = ir.components_of(v == 1, 6)[1]
    assert ir.split_touching(v, 1, 1.5, 6)[1] > ka


def label_map(shape, seed, p):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < p, rng.integers(1, 9, shape), 0).astype(np.int32)


@pytest.mark.parametrize('distance', (0, 1, 1.5, 3))
def test_expand_labels_is_the_brute_force(distance):
    for shape, seed, p in (((6, 9, 14), 0, 0.03), ((1, 1, 25), 1, 0.2), ((5, 4, 6), 2, 0.3)):
        lab = label_map(shape, seed, p)
        d2, idx = brute(lab > 0)
        want = np.where(d2 <= ir.radius_sq(distance), lab.reshape(-1)[idx], 0)
        got = ir.expand_labels(lab, distance)
        assert got.dtype == np.int32 and np.array_equal(got, want), (shape, distance)
        assert np.array_equal(got[lab > 0], lab[lab > 0])                      # a labelled voxel keeps its label
        if distance == 0:
            assert np.array_equal(got, lab)
    assert not ir.expand_labels(np.zeros((3, 4, 5), np.int32), distance).any()


def test_assign_and_remap_follow_their_rules():
    rng = np.random.default_rng(3)
    shape = (4, 5, 6)
    s = rng.random(shape) < 0.1
    d2, idx = ir.feature_of(s)
    seed_labels = np.where(s, rng.integers(1, 5, shape), 0).astype(np.int32)
    group = rng.integers(0, 3, shape).astype(np.int32)
    for r2 in (0, 2, ir.MAX_SQ):
        out = ir.assign(idx, d2, seed_labels, r2)
        for v in np.ndindex(shape):
            assert out[v] == (seed_labels.reshape(-1)[idx[v]] if d2[v] <= r2 else 0)
        out = ir.assign(idx, d2, seed_labels, r2, group=group, offset=10)
        for v in np.ndindex(shape):
            own = d2[v] <= r2 and group.reshape(-1)[idx[v]] == group[v]
            assert out[v] == (0 if group[v] == 0 else seed_labels.reshape(-1)[idx[v]] if own else 10 + group[v])
    none = np.full(shape, -1, np.int32)
    assert not ir.assign(none, np.full(shape, ir.INF, np.int32), seed_labels, ir.MAX_SQ).any()
    assert np.array_equal(ir.assign(none, np.full(shape, ir.INF, np.int32), seed_labels, ir.MAX_SQ, group=group, offset=7), np.where(group > 0, 7 + group, 0))
    lab = np.array([[[0, 1, 2, 3, 9, -4]]], np.int32)
    assert ir.remap(lab, np.array([0, 5, 0, 6], np.int32)).tolist() == [[[0, 5, 0, 6, 9, -4]]]


def _host_cases():
    yield grains((9, 14, 30), 3)
    yield planted_leak()
    yield random_pred((7, 9, 12), 2, 4)
    yield random_pred((7, 9, 12), 5, 5)
    yield np.zeros((3, 4, 5), np.uint8)
    yield np.ones((1, 1, 1), np.uint8)
    yield np.ones((2, 3, 4), np.uint8)


def test_the_numpy_path_is_the_definition():
    from interactive_unet import instances
    assert instances.INF == ir.INF and instances.MAX_SQ == ir.MAX_SQ
    for v in _host_cases():
        for target in (0, 1, 3):
            for invert in (False, True):
                check_same(instances.nearest(v, target, invert), ir.feature(v, target, invert), (v.shape, target, invert))
            for radius in (0, 1.5, 3):
                for conn in (6, 18, 26):
                    labels, k = instances.split_touching(v, target, radius, conn)
                    want, kw = ir.split_touching(v, target, radius, conn)
                    assert labels.dtype == np.int32 and k == kw and np.array_equal(labels, want), (v.shape, target, radius, conn)
            sizes, first = instances.instance_table(labels, k)
            assert sizes.dtype == np.int32 and first.dtype == np.int32 and sizes[0] == 0 and first[0] == -1
            assert np.array_equal(sizes[1:], np.bincount(labels.reshape(-1), minlength=k + 1)[1:])
            assert first[1:].tolist() == [np.flatnonzero(labels.reshape(-1) == i)[0] for i in range(1, k + 1)]
    for shape, seed, p in (((6, 9, 14), 0, 0.03), ((1, 1, 25), 1, 0.2), ((3, 4, 5), 2, 0.0)):
        lab = label_map(shape, seed, p)
        check_same(instances.nearest_labelled(lab), ir.feature_of(lab > 0), shape)
        for distance in (0, 1, 1.5, 3):
            got = instances.expand_labels(lab, distance)
            assert got.dtype == np.int32 and np.array_equal(got, ir.expand_labels(lab, distance)), (shape, distance)


def test_host_refusals_need_no_device():
    from interactive_unet import instances as m
    v = np.zeros((4, 5, 6), np.uint8)
    pred = np.zeros((4, 5, 6, 3), np.uint8)
    calls = (lambda s: m.nearest(s), lambda s: m.split_touching(s, 1, 1))
    for bad in (v.astype(np.int32), v[0], pred[..., :1], np.zeros((4, 5, 6, 17), np.uint8), v[:, :, ::2], np.zeros((0, 5, 6), np.uint8),
                torch.from_numpy(v), v.tolist(), None,
                np.empty((46342, 1, 1), np.uint8),                              # the squared diagonal
                np.empty((1291, 1291, 1291), np.uint8)):                        # more than 2^31 - 1 voxels (never touched)
        for call in calls:
            with pytest.raises(ValueError):
                call(bad)
    lab = np.zeros((4, 5, 6), np.int32)
    calls = (lambda s: m.nearest_labelled(s), lambda s: m.expand_labels(s, 1), lambda s: m.instance_table(s, 0))
    for bad in (lab.astype(np.uint8), lab.astype(np.int64), lab[0], lab[None], lab[:, :, ::2], np.zeros((0, 5, 6), np.int32),
                torch.from_numpy(lab), lab.tolist(), None,
                np.empty((46342, 1, 1), np.int32), np.empty((1291, 1291, 1291), np.int32)):
        for call in calls:
            with pytest.raises(ValueError):
                call(bad)
    for target in (-1, 256, 1.0, True, 'a'):
        for call in (lambda: m.nearest(v, target), lambda: m.split_touching(v, target, 1)):
            with pytest.raises(ValueError, match='target'):
                call()
    for radius in (-1, -0.5, float('nan'), float('inf'), 46341, 'r', None, True):
        with pytest.raises(ValueError, match='radius'):
            m.split_touching(v, 1, radius)
        with pytest.raises(ValueError, match='distance'):
            m.expand_labels(lab, radius)
    for conn in (0, 4, 8, 27):
        with pytest.raises(ValueError, match='connectivity'):
            m.split_touching(v, 1, 1, conn)
    for count in (-1, 1.0, True, None):
        with pytest.raises(ValueError, match='count'):
            m.instance_table(lab, count)


def test_limits_and_refusals_through_the_library_without_a_gpu():
    """Argument validation precedes every HIP call."""
    from interactive_unet import _native as nv
    if not os.path.isfile(nv.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    l = nv.lib()
    need = l.iunet_edt_feature_ws_bytes
    a16 = lambda n: (n + 15) // 16 * 16
    assert need(46341, 1, 1) > 0 and need(1, 1, 1) == 32 and need(37, 41, 150) == a16(8 * 227550) + a16(4 * 227550)
    assert need(1030, 1024, 1024) == 12 * 1030 * 2 ** 20 and need(32768, 32768, 1) > 0 and need(2047, 1024, 1024) > 0
    assert need(46342, 1, 1) == 0 and need(0, 4, 4) == 0 and need(4, -1, 4) == 0 and need(4, 4, 0) == 0
    assert need(2048, 1024, 1024) == 0 and need(2 ** 16, 2 ** 15, 1) == 0                    # Z Y X = 2^31
    assert need(32769, 32769, 1) == 0                                                         # the squared diagonal
    for Z, Y, X in ((46341, 1, 1), (46342, 1, 1), (0, 4, 4), (2048, 1024, 1024), (37, 41, 150)):
        assert (need(Z, Y, X) == 0) == (l.iunet_edt_ws_bytes(Z, Y, X) == 0) == (not mr.limits_ok(Z, Y, X))

    mem = (ctypes.c_double * 64)()
    at = lambda n: ctypes.c_void_p(ctypes.addressof(mem) + n)                          # never dereferenced: every call below stops before its launch
    buf, far, further, odd = at(0), at(4096 * 4), at(8192 * 4), at(2)

    def feat(src=buf, Z=8, Y=8, X=8, C=1, target=1, invert=0, d2=buf, idx=far, cls=None, ws=buf, ws_bytes=None):
        ws_bytes = need(Z, Y, X) if ws_bytes is None else ws_bytes
        return l.iunet_edt_feature(src, Z, Y, X, C, target, invert, d2, idx, cls, ws, ws_bytes, None), l.iunet_last_error()
    for kw, word in ((dict(src=None), b'null'), (dict(d2=None), b'null'), (dict(idx=None), b'null'), (dict(ws=None), b'null'),
                     (dict(Z=0), b'dimension'), (dict(Y=-3), b'dimension'), (dict(X=0), b'dimension'),
                     (dict(Z=2048, Y=1024, X=1024, ws_bytes=1 << 40), b'voxels'), (dict(Z=46342, Y=1, X=1, ws_bytes=1 << 40), b'diagonal'),
                     (dict(C=0), b'classes'), (dict(C=17), b'classes'), (dict(target=-1), b'target'), (dict(target=256), b'target'),
                     (dict(invert=2), b'invert'), (dict(ws_bytes=need(8, 8, 8) - 1), b'workspace'), (dict(ws_bytes=0), b'workspace'),
                     (dict(ws_bytes=l.iunet_edt_ws_bytes(8, 8, 8)), b'workspace'), (dict(d2=odd), b'aligned'), (dict(idx=odd), b'aligned'),
                     (dict(ws=odd), b'aligned'), (dict(idx=buf), b'overlap'), (dict(idx=at(4 * 511)), b'overlap')):
        rc, msg = feat(**kw)
        assert rc < 0 and word in msg, (kw, msg)
    assert feat(Z=46341, Y=1, X=1, d2=None)[1].startswith(b'edt_feature: null')        # the accepted limit gets as far as the pointers

    def mask(prev=buf, Z=8, Y=8, X=8, r2=4, above=1, d2=far, idx=further, ws=buf, ws_bytes=None):
        ws_bytes = need(Z, Y, X) if ws_bytes is None else ws_bytes
        return l.iunet_edt_feature_mask(prev, Z, Y, X, r2, above, d2, idx, ws, ws_bytes, None), l.iunet_last_error()
    for kw, word in ((dict(prev=None), b'null'), (dict(d2=None), b'null'), (dict(idx=None), b'null'), (dict(ws=None), b'null'),
                     (dict(Z=0), b'dimension'), (dict(Z=2048, Y=1024, X=1024, ws_bytes=1 << 40), b'voxels'),
                     (dict(Z=46342, Y=1, X=1, ws_bytes=1 << 40), b'diagonal'), (dict(r2=-1), b'r2'), (dict(r2=2 ** 31 - 1), b'r2'),
                     (dict(above=2), b'above'), (dict(ws_bytes=need(8, 8, 8) - 1), b'workspace'), (dict(prev=odd), b'aligned'),
                     (dict(idx=odd), b'aligned'), (dict(d2=buf), b'overlap'), (dict(idx=buf), b'overlap'), (dict(idx=far), b'overlap'),
                     (dict(idx=at(4 * 4096 + 4 * 511)), b'overlap')):
        rc, msg = mask(**kw)
        assert rc < 0 and word in msg, (kw, msg)

    def assign(idx=buf, d2=far, seed=further, group=None, offset=0, Z=8, Y=8, X=8, r2=4, out=at(12288 * 4)):
        return l.iunet_edt_assign(idx, d2, seed, group, offset, Z, Y, X, r2, out, None), l.iunet_last_error()
    for kw, word in ((dict(idx=None), b'null'), (dict(d2=None), b'null'), (dict(seed=None), b'null'), (dict(out=None), b'null'),
                     (dict(Y=0), b'dimension'), (dict(Z=2048, Y=1024, X=1024), b'voxels'), (dict(Z=46342, Y=1, X=1, idx=None), b'null'),
                     (dict(r2=-1), b'r2'), (dict(r2=2 ** 31 - 1), b'r2'), (dict(offset=-1), b'offset'), (dict(idx=odd), b'aligned'),
                     (dict(group=odd), b'aligned'), (dict(out=odd), b'aligned'), (dict(out=buf), b'overlap'), (dict(out=further), b'overlap'),
                     (dict(out=at(8192 * 4 + 4 * 511)), b'overlap'), (dict(group=at(16384 * 4), out=at(16384 * 4)), b'overlap')):
        rc, msg = assign(**kw)
        assert rc < 0 and word in msg, (kw, msg)

    def remap(labels=buf, Z=8, Y=8, X=8, K=3, table=far):
        return l.iunet_label_remap(labels, Z, Y, X, K, table, None), l.iunet_last_error()
    for kw, word in ((dict(labels=None), b'null'), (dict(table=None), b'null'), (dict(X=0), b'dimension'), (dict(Z=2048, Y=1024, X=1024), b'voxels'),
                     (dict(Z=46342, Y=1, X=1, labels=None), b'null'), (dict(K=-1), b'labels'),
                     (dict(labels=odd), b'aligned'), (dict(table=odd), b'aligned')):
        rc, msg = remap(**kw)
        assert rc < 0 and word in msg, (kw, msg)
