"""Geodesic seeded growth without a GPU: the definition tests/geodesic_ref.py against multi-source Dijkstra and a
brute-force smallest label over the seeds at that distance, against closed forms in free space, on a tie, a sealed pocket, seeds off the
domain, no seed and a serpentine corridor; the two planted volumes voxel count by voxel count and the invariants of split_touching; the
host layer's numpy path against the definition; the host refusals; the limits and the entry points' argument checks through the built
library."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import geodesic_ref as gr
from tests.volume_inputs import random_pred

METRIC_NAMES = (6, 18, 26, 'chamfer')


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
    """21 x 21 x 50: a ball with a long thin arm whose tip is nearer, in a straight line, to the core of a second ball.  Two objects."""
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


def random_case(shape, density, seed, p_seed=0.05):
    """(a bool, seeds int32): a random domain, and labels 1 .. 8 on about p_seed of ALL voxels (some of them off the domain)."""
    rng = np.random.default_rng(seed)
    a = rng.random(shape) < density
    seeds = np.where(rng.random(shape) < p_seed, rng.integers(1, 9, shape), 0).astype(np.int32)
    return a, seeds


def serpentine(shape, z=None):
    """(a uint8 [Z, Y, X], path int [n, 3]): a corridor of one voxel's width in the plane z: the rows of even y, joined at alternating ends
    through the odd rows; path lists its voxels from one end to the other."""
    Z, Y, X = shape
    z = Z // 2 if z is None else z
    path = []
    for k, y in enumerate(range(0, Y, 2)):
        xs = range(X) if k % 2 == 0 else range(X - 1, -1, -1)
        path += [(z, y, x) for x in xs]
        if y + 2 < Y:
            path.append((z, y + 1, path[-1][2]))
    path = np.array(path)
    a = np.zeros(shape, np.uint8)
    a[tuple(path.T)] = 1
    assert a.sum() == len(path)
    return a, path


def dijkstra(a, seeds, weights):
    """(labels, g) by scipy's Dijkstra from every seed on its own: g the minimum over the seeds, the label the smallest among the seeds
    that attain it."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import dijkstra as sp_dijkstra
    shape = a.shape
    node = np.arange(a.size).reshape(shape)
    rows, cols, vals = [], [], []
    for dz, dy, dx in gr.OFFSETS:
        w = weights[abs(dz) + abs(dy) + abs(dx) - 1]
        if w == 0:
            continue
        lo = [max(0, -d) for d in (dz, dy, dx)]
        hi = [n - max(0, d) for n, d in zip(shape, (dz, dy, dx))]
        src = tuple(slice(l, h) for l, h in zip(lo, hi))
        dst = tuple(slice(l + d, h + d) for l, h, d in zip(lo, hi, (dz, dy, dx)))
        both = a[src] & a[dst]
        rows.append(node[src][both]); cols.append(node[dst][both]); vals.append(np.full(int(both.sum()), w, np.float64))
    graph = coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(a.size, a.size)).tocsr()
    at = np.flatnonzero((a & (seeds > 0)).reshape(-1))
    labels, g = np.zeros(a.size, np.int32), np.full(a.size, gr.INF, np.int32)
    if len(at):
        dist = sp_dijkstra(graph, directed=True, indices=at)             # [seed, voxel]
        best = dist.min(axis=0)
        lab = seeds.reshape(-1)[at].astype(np.int64)
        smallest = np.where(dist == best[None], lab[:, None], np.int64(1) << 40).min(axis=0)
        reached = np.isfinite(best)
        g[reached] = best[reached].astype(np.int32)
        labels[reached] = smallest[reached].astype(np.int32)
    return labels.reshape(shape), g.reshape(shape)


def check_same(got, want, where):
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32, where
    assert np.array_equal(got[1], want[1]), ('g', where)
    assert np.array_equal(got[0], want[0]), ('labels', where)


@pytest.mark.parametrize('metric', METRIC_NAMES)
@pytest.mark.parametrize('shape', ((5, 6, 7), (1, 1, 20), (4, 1, 9)))
def test_the_definition_is_dijkstra_and_the_smallest_label_at_that_distance(shape, metric):
    for density in (0.6, 0.8):
        for trial in range(3):
            a, seeds = random_case(shape, density, 100 * trial + sum(shape), 0.05 if trial < 2 else 0.2)
            got = gr.grow_in(a, seeds, metric)
            check_same(got, dijkstra(a, seeds, gr.METRICS[metric]), (shape, metric, density, trial))
            assert (got[1][~a] == gr.INF).all() and not got[0][~a].any()
            on = a & (seeds > 0)
            assert not got[1][on].any() and np.array_equal(got[0][on], seeds[on])
            assert ((got[1] == gr.INF) == (got[0] == 0)).all()


def test_the_definition_with_weights_that_leave_a_rank_out():
    for weights in ((2, 0, 3), (5, 7, 0), (255, 255, 255), (1, 3, 2)):
        a, seeds = random_case((5, 6, 7), 0.7, 11)
        check_same(gr.grow_in(a, seeds, weights), dijkstra(a, seeds, weights), weights)


def test_one_seed_in_free_space_against_the_closed_forms():
    shape = (7, 9, 11)
    for at in ((0, 0, 0), (3, 4, 5), (6, 8, 10), (6, 0, 5)):
        seeds = np.zeros(shape, np.int32)
        seeds[at] = 5
        off = np.sort(np.stack([np.abs(i - c) for i, c in zip(np.indices(shape), at)]), axis=0)
        c, b, a = off                                                     # a >= b >= c
        for metric, want in ((6, a + b + c), (26, a), (18, np.maximum(a, (a + b + c + 1) // 2)), ('chamfer', 3 * (a - b) + 4 * (b - c) + 5 * c)):
            labels, g = gr.grow_in(np.ones(shape, bool), seeds, metric)
            assert np.array_equal(g, want) and (labels == 5).all(), (at, metric)


def test_of_two_seeds_at_the_same_distance_the_smaller_label_wins():
    seeds = np.zeros((1, 1, 5), np.int32)
    seeds[0, 0, 0], seeds[0, 0, 4] = 7, 3                                 # the lower raster index carries the larger label
    for metric in METRIC_NAMES:
        labels, g = gr.grow_in(np.ones((1, 1, 5), bool), seeds, metric)
        w = gr.METRICS[metric][0]
        assert g.reshape(-1).tolist() == [0, w, 2 * w, w, 0] and labels.reshape(-1).tolist() == [7, 7, 3, 3, 3], metric
    seeds = np.zeros((3, 3, 3), np.int32)                                 # along a diagonal too
    seeds[0, 0, 0], seeds[2, 2, 2] = 9, 2
    labels, g = gr.grow_in(np.ones((3, 3, 3), bool), seeds, 'chamfer')
    assert g[1, 1, 1] == 5 and labels[1, 1, 1] == 2 and labels[0, 0, 1] == 9 and labels[2, 2, 1] == 2
    assert labels[0, 2, 1] == 2 and g[0, 2, 1] == 7                       # (0, 2, 1): an edge and a face step from either seed


def sealed_pocket(shape=(5, 6, 9)):
    """(a, seeds, pocket): free space cut by a wall of background at x = 4; the seed is on the left, the pocket is the right side."""
    a = np.ones(shape, bool)
    a[:, :, 4] = False
    seeds = np.zeros(shape, np.int32)
    seeds[2, 2, 1] = 4
    pocket = np.zeros(shape, bool)
    pocket[:, :, 5:] = True
    return a, seeds, pocket


def test_a_sealed_pocket_seeds_off_the_domain_and_no_seed():
    a, seeds, pocket = sealed_pocket()
    for metric in METRIC_NAMES:
        labels, g = gr.grow_in(a, seeds, metric)
        assert (g[pocket] == gr.INF).all() and not labels[pocket].any() and (labels[a & ~pocket] == 4).all() and (g[a & ~pocket] < gr.INF).all()
        key = gr.grow_keys(a, seeds, metric)[0]
        fb = np.full(a.shape, 6, np.int32)
        with_fb = gr.finish(key, fallback=fb, offset=10)[0]
        assert (with_fb[pocket] == 16).all() and np.array_equal(with_fb[~pocket], labels[~pocket])      # the wall stays 0
        # a positive entry off A is ignored, on the wall and anywhere else: the same result
        more = seeds.copy()
        more[:, :, 4] = 8
        check_same(gr.grow_in(a, more, metric), (labels, g), metric)
        # a diagonal crack in the wall is a way through for the metrics with that step only
        b = a.copy()
        b[0, 0, 4], b[0, 0, 3], b[0, 1, 3], b[1, 0, 3] = True, False, False, False      # (0, 0, 4) touches the left side at (1, 1, 3) only: a vertex step
        reached = gr.grow_in(b, seeds, metric)[1][0, 0, 5] < gr.INF
        assert reached == (gr.METRICS[metric][2] > 0), metric
        labels, g = gr.grow_in(a, np.zeros(a.shape, np.int32), metric)
        assert (g == gr.INF).all() and not labels.any()
        labels, g = gr.grow_in(a, np.where(a, 0, 3).astype(np.int32), metric)      # seeds off A only
        assert (g == gr.INF).all() and not labels.any()
    labels, g = gr.grow_in(np.zeros((2, 3, 4), bool), np.ones((2, 3, 4), np.int32))
    assert (g == gr.INF).all() and not labels.any()
    labels, g = gr.grow_in(np.ones((2, 3, 4), bool), np.full((2, 3, 4), 6, np.int32))
    assert not g.any() and (labels == 6).all()


def test_along_a_serpentine_corridor_g_is_the_position():
    a, path = serpentine((3, 9, 12))
    assert len(path) == 5 * 12 + 4
    seeds = np.zeros(a.shape, np.int32)
    seeds[tuple(path[0])] = 3
    for metric, w1 in ((6, 1), ((3, 0, 0), 3), ((7, 0, 0), 7)):
        key, sweeps = gr.grow_keys(a == 1, seeds, metric)
        labels, g = gr.split_keys(key)
        assert np.array_equal(g[tuple(path.T)], w1 * np.arange(len(path))) and (labels[a == 1] == 3).all() and sweeps == len(path) - 1
        check_same(gr.grow(a, seeds, 1, metric), (labels, g), metric)
    check_same(gr.grow_in(a == 1, seeds, 'chamfer'), dijkstra(a == 1, seeds, (3, 4, 5)), 'chamfer')      # it cuts the corners
    # a seed at each end: the midpoint tie goes to the smaller label
    a, path = serpentine((3, 9, 13))                                      # an odd number of voxels: one midpoint at the same distance of both
    n = len(path)
    assert n % 2 == 1
    seeds = np.zeros(a.shape, np.int32)
    seeds[tuple(path[0])], seeds[tuple(path[-1])] = 9, 2
    labels, g = gr.grow_in(a == 1, seeds, 6)
    pos = np.arange(n)
    assert np.array_equal(g[tuple(path.T)], np.minimum(pos, n - 1 - pos))
    assert np.array_equal(labels[tuple(path.T)], np.where(pos < n // 2, 9, 2)) and labels[tuple(path[n // 2])] == 2


def test_the_class_rule_of_a_predicted_volume():
    pred = random_pred((7, 9, 12), 3, 1)
    has, cls = pred.max(-1) > 0, pred.argmax(-1)
    assert (~has).any()
    _, seeds = random_case((7, 9, 12), 1.0, 5)
    for target in (0, 1, 5):
        check_same(gr.grow(pred, seeds, target, 26), gr.grow_in(has & (cls == target), seeds, 26), target)
    cm = cls.astype(np.uint8)
    check_same(gr.grow(cm, seeds, 0, 6), gr.grow_in(cm == 0, seeds, 6), 'class map')     # a class map: every voxel counts as predicted


def test_the_planted_split():
    from interactive_unet import components
    v = planted_split()
    a = v == 1
    assert components.label(v)[1] == 3
    labels, k, ke, ka = gr.split_touching(v, 1, 4, 6, parts=True)
    assert (ke, ka, k) == (3, 3, 4)
    assert np.bincount(labels.reshape(-1))[1:].tolist() == [924, 887, 933, 33]
    assert np.array_equal(labels > 0, a)
    assert labels[10, 10, 8] == 1 and labels[10, 10, 18] == 2
    assert (labels[ball(a.shape, (10, 10, 30), 2)] == 4).all() and (labels[10, 10, 36:44] == 3).all() and labels[10, 10, 50] == 3


@pytest.mark.parametrize('radius', (2, 3))
def test_the_leak_case_has_no_remainder(radius):
    from interactive_unet import components
    v = planted_leak()
    assert components.label(v)[1] == 2
    labels, k, ke, ka = gr.split_touching(v, 1, radius, 6, parts=True)
    assert (ke, ka, k) == (2, 2, 2)
    assert np.bincount(labels.reshape(-1))[1:].tolist() == [925, 533]
    assert (labels[10, 10, 11:30] == 2).all() and labels[10, 10, 6] == 2 and labels[10, 10, 37] == 1    # the arm's tip stays with its own ball
    objects = components.label(v)[0]
    assert np.array_equal(labels > 0, v == 1) and all(len(np.unique(objects[labels == i])) == 1 for i in (1, 2))


def _check_invariants(v, target, conn, metric, radii=(0, 1, 1.5, 3)):
    a = gr.members(v, target)
    objects, ka = gr.components_of(a, conn)
    for radius in radii:
        labels, k, ke, ka2 = gr.split_touching(v, target, radius, conn, metric, parts=True)
        assert labels.dtype == np.int32 and ka2 == ka
        assert np.array_equal(labels > 0, a)                               # labels > 0 exactly on A
        pairs = np.unique(np.stack([labels[a], objects[a]]), axis=1)       # no label spans two components of A
        assert len(np.unique(pairs[0])) == pairs.shape[1] == k
        cores = gr.feature_of(~a)[0] > gr.radius_sq(radius)
        without = ka - len(np.unique(objects[cores]))
        assert k == ke + without, (conn, metric, radius)                   # the cores, and one instance per object without a core
        firsts = [np.flatnonzero(labels.reshape(-1) == i)[0] for i in range(1, k + 1)]
        assert firsts == sorted(firsts)                                    # numbered in order of the first voxel


@pytest.mark.parametrize('conn', (6, 26))
def test_the_invariants_of_split_touching(conn):
    from interactive_unet import components
    for v, target in ((grains((14, 20, 31), 1), 1), (grains((14, 20, 31), 2, 0.02), 1), (planted_split(), 1), (random_pred((7, 9, 12), 3, 1), 0)):
        _check_invariants(v, target, conn, 'chamfer')
        _check_invariants(v, target, conn, conn, radii=(1.5,))
        # radius 0: every object is its own core (all of it), the numbering is components.label's
        labels, k = gr.split_touching(v, target, 0, conn)
        want, kw, _ = components.label(gr.members(v, target).astype(np.uint8), conn)
        assert k == kw and np.array_equal(labels, want)
    # the steps follow the connectivity: under 6 the chamfer metric keeps its face steps only, and no diagonal step joins two objects
    assert gr.split_weights('chamfer', 6) == (3, 0, 0) and gr.split_weights('chamfer', 18) == (3, 4, 0) and gr.split_weights(26, 26) == (1, 1, 1)
    assert gr.split_weights(6, 26) == (1, 0, 0)
    v = np.zeros((1, 2, 2), np.uint8)
    v[0, 0, 0] = v[0, 1, 1] = 1
    assert gr.split_touching(v, 1, 0, 6)[1] == 2 and gr.split_touching(v, 1, 0, 26)[1] == 1


def _host_cases():
    yield grains((9, 14, 30), 3)
    yield planted_leak()
    yield random_pred((7, 9, 12), 2, 4)
    yield random_pred((7, 9, 12), 5, 5)
    yield np.zeros((3, 4, 5), np.uint8)
    yield np.ones((1, 1, 1), np.uint8)
    yield np.ones((2, 3, 4), np.uint8)


def test_the_numpy_path_is_the_definition():
    from interactive_unet import geodesic
    assert geodesic.INF == gr.INF and geodesic.METRICS == gr.METRICS
    for n, v in enumerate(_host_cases()):
        shape = v.shape[:3]
        _, seeds = random_case(shape, 1.0, n, 0.03)
        for target in (0, 1, 3):
            for metric in METRIC_NAMES + ((2, 0, 5),):
                check_same(geodesic.grow(v, seeds, target, metric), gr.grow(v, seeds, target, metric), (shape, target, metric))
            for radius in (0, 1.5, 3):
                for conn in (6, 18, 26):
                    for metric in ('chamfer', 6):
                        labels, k = geodesic.split_touching(v, target, radius, conn, metric)
                        want, kw = gr.split_touching(v, target, radius, conn, metric)
                        assert labels.dtype == np.int32 and k == kw and np.array_equal(labels, want), (shape, target, radius, conn, metric)
        dom = np.where(gr.members(v, 1), 7, -2).astype(np.int32)
        for metric in METRIC_NAMES:
            check_same(geodesic.grow_in(dom, seeds, metric), gr.grow_in(dom, seeds, metric), (shape, metric))
    check_same(geodesic.grow(np.ones((2, 3, 4), np.uint8), np.zeros((2, 3, 4), np.int32)), gr.grow(np.ones((2, 3, 4), np.uint8), np.zeros((2, 3, 4), np.int32)), 'defaults')
    a, path = serpentine((3, 9, 12))
    seeds = np.zeros(a.shape, np.int32)
    seeds[tuple(path[0])] = 1
    with pytest.raises(RuntimeError, match='max_rounds'):
        geodesic.grow(a, seeds, 1, 6, max_rounds=5)
    assert np.array_equal(geodesic.grow(a, seeds, 1, 6, max_rounds=len(path))[1], gr.grow(a, seeds, 1, 6)[1])


def test_host_refusals_need_no_device():
    from interactive_unet import geodesic as m
    v = np.zeros((4, 5, 6), np.uint8)
    s = np.zeros((4, 5, 6), np.int32)
    pred = np.zeros((4, 5, 6, 3), np.uint8)
    for bad in (v.astype(np.int32), v[0], pred[..., :1], np.zeros((4, 5, 6, 17), np.uint8), v[:, :, ::2], np.zeros((0, 5, 6), np.uint8),
                torch.from_numpy(v), v.tolist(), None,
                np.empty((1291, 1291, 1291), np.uint8)):                        # more than 2^31 - 1 voxels (never touched)
        for call in (lambda x: m.grow(x, s), lambda x: m.split_touching(x, 1, 1)):
            with pytest.raises(ValueError):
                call(bad)
    with pytest.raises(ValueError, match='diagonal'):
        m.split_touching(np.empty((46342, 1, 1), np.uint8), 1, 1)               # the split measures Euclidean distances too
    for bad in (s.astype(np.uint8), s.astype(np.int64), s[0], s[None], s[:, :, ::2], np.zeros((0, 5, 6), np.int32), torch.from_numpy(s),
                s.tolist(), None, np.empty((1291, 1291, 1291), np.int32)):
        with pytest.raises(ValueError):
            m.grow_in(bad, s)
    for bad in (s.astype(np.uint8), s.astype(np.int64), s[0], s[None], s[:, :, ::2], np.zeros((4, 5, 7), np.int32), np.zeros((5, 4, 6), np.int32),
                torch.from_numpy(s), s.tolist(), None):                          # a seeds map of the wrong kind, shape or side
        for call in (lambda x: m.grow(v, x), lambda x: m.grow(pred, x), lambda x: m.grow_in(s, x)):
            with pytest.raises(ValueError, match='seeds'):
                call(bad)
    for target in (-1, 256, 1.0, True, 'a'):
        for call in (lambda: m.grow(v, s, target), lambda: m.split_touching(v, target, 1)):
            with pytest.raises(ValueError, match='target'):
                call()
    for metric in (0, 7, 4, 'euclid', None, True, 1.0, (1, 1), (1, 1, 1, 1), (0, 1, 1), (256, 0, 0), (1, -1, 0), (1, 0, 256), (1.0, 0, 0), (True, 0, 0)):
        for call in (lambda: m.grow(v, s, 1, metric), lambda: m.grow_in(s, s, metric), lambda: m.split_touching(v, 1, 1, 6, metric)):
            with pytest.raises(ValueError, match='metric'):
                call()
    for radius in (-1, -0.5, float('nan'), float('inf'), 46341, 'r', None, True):
        with pytest.raises(ValueError, match='radius'):
            m.split_touching(v, 1, radius)
    for conn in (0, 4, 8, 27):
        with pytest.raises(ValueError, match='connectivity'):
            m.split_touching(v, 1, 1, conn)
    for rounds in (0, -1, 1.5, True, 'a'):
        for call in (lambda: m.grow(v, s, max_rounds=rounds), lambda: m.grow_in(s, s, max_rounds=rounds), lambda: m.split_touching(v, 1, 1, max_rounds=rounds)):
            with pytest.raises(ValueError, match='max_rounds'):
                call()
    # Z Y X max(w) <= 2^31 - 2: a chamfer run of 1024^3 is refused, a unit-step run is not refused for its size (never touched)
    big, bigs = np.empty((1024, 1024, 1024), np.uint8), np.empty((1024, 1024, 1024), np.int32)
    for call in (lambda: m.grow(big, bigs), lambda: m.grow_in(bigs, bigs, 'chamfer'), lambda: m.grow(big, bigs, 1, (2, 0, 0)),
                 lambda: m.split_touching(big, 1, 1, 26, 'chamfer')):
        with pytest.raises(ValueError, match='2\\^31 - 2'):
            call()
    assert gr.limits_ok(1024, 1024, 1024, (1, 1, 1)) and not gr.limits_ok(1024, 1024, 1024, (3, 4, 5)) and not gr.limits_ok(1024, 1024, 1024, (2, 0, 0))
    assert gr.limits_ok(2 ** 31 - 2, 1, 1) and not gr.limits_ok(2 ** 31 - 1, 1, 1) and gr.limits_ok(715827882, 1, 1, (3, 0, 0)) and not gr.limits_ok(715827883, 1, 1, (3, 0, 0))


def test_the_module_goes_with_the_overlay():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import install_overlay
    assert 'geodesic' in install_overlay.ADDED


def test_limits_and_refusals_through_the_library_without_a_gpu():
    """Argument validation precedes every HIP call."""
    from interactive_unet import _native as nv
    if not os.path.isfile(nv.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    l = nv.lib()
    need = l.iunet_geo_ws_bytes
    a16 = lambda n: (n + 15) // 16 * 16
    tiles = lambda Z, Y, X: ((Z + 7) // 8) * ((Y + 7) // 8) * ((X + 63) // 64)
    want = lambda Z, Y, X: a16(8 * Z * Y * X) + 2 * a16(4 * tiles(Z, Y, X))
    assert need(1, 1, 1) == 16 + 2 * 16 and need(37, 41, 150) == want(37, 41, 150) == 8 * 227550 + 2 * a16(4 * 5 * 6 * 3)
    for shape in ((8, 8, 64), (9, 8, 64), (8, 9, 65), (1, 1, 300), (2100, 3, 5), (1024, 1024, 1024), (2047, 1024, 1024), (2 ** 31 - 1, 1, 1), (46342, 1, 1)):
        assert need(*shape) == want(*shape) > 0, shape
    assert need(0, 4, 4) == 0 and need(4, -1, 4) == 0 and need(4, 4, 0) == 0
    assert need(2048, 1024, 1024) == 0 and need(2 ** 16, 2 ** 15, 1) == 0                    # Z Y X = 2^31

    mem = (ctypes.c_double * 64)()
    at = lambda n: ctypes.c_void_p(ctypes.addressof(mem) + n)                          # never dereferenced: every call below stops before its launch
    buf, far, further, odd, odd8 = at(0), at(1 << 20), at(2 << 20), at(2), at(8)
    n8 = need(8, 8, 8)

    def init(src=far, Z=8, Y=8, X=8, C=1, target=1, seeds=further, ws=buf, ws_bytes=None):
        ws_bytes = need(Z, Y, X) if ws_bytes is None else ws_bytes
        return l.iunet_geo_init(src, Z, Y, X, C, target, seeds, ws, ws_bytes, None), l.iunet_last_error()
    for kw, word in ((dict(src=None), b'null'), (dict(seeds=None), b'null'), (dict(ws=None), b'null'),
                     (dict(Z=0), b'dimension'), (dict(Y=-3), b'dimension'), (dict(X=0), b'dimension'),
                     (dict(Z=2048, Y=1024, X=1024, ws_bytes=1 << 40), b'voxels'), (dict(C=0), b'classes'), (dict(C=17), b'classes'),
                     (dict(target=-1), b'target'), (dict(target=256), b'target'), (dict(ws_bytes=n8 - 1), b'workspace'), (dict(ws_bytes=0), b'workspace'),
                     (dict(ws=odd), b'aligned'), (dict(ws=odd8), b'aligned'), (dict(seeds=odd), b'aligned')):
        rc, msg = init(**kw)
        assert rc < 0 and word in msg and msg.startswith(b'geo_init:'), (kw, msg)

    def mask(dom=far, Z=8, Y=8, X=8, seeds=further, ws=buf, ws_bytes=None):
        ws_bytes = need(Z, Y, X) if ws_bytes is None else ws_bytes
        return l.iunet_geo_init_mask(dom, Z, Y, X, seeds, ws, ws_bytes, None), l.iunet_last_error()
    for kw, word in ((dict(dom=None), b'null'), (dict(seeds=None), b'null'), (dict(ws=None), b'null'), (dict(Z=0), b'dimension'),
                     (dict(Z=2048, Y=1024, X=1024, ws_bytes=1 << 40), b'voxels'), (dict(ws_bytes=n8 - 1), b'workspace'),
                     (dict(ws=odd8), b'aligned'), (dict(dom=odd), b'aligned'), (dict(seeds=odd), b'aligned')):
        rc, msg = mask(**kw)
        assert rc < 0 and word in msg and msg.startswith(b'geo_init_mask:'), (kw, msg)

    def relax(ws=buf, ws_bytes=None, Z=8, Y=8, X=8, w=(3, 4, 5), rounds=1, changed=far):
        ws_bytes = need(Z, Y, X) if ws_bytes is None else ws_bytes
        return l.iunet_geo_relax(ws, ws_bytes, Z, Y, X, w[0], w[1], w[2], rounds, changed, None), l.iunet_last_error()
    for kw, word in ((dict(ws=None), b'null'), (dict(changed=None), b'null'), (dict(X=0), b'dimension'),
                     (dict(Z=2048, Y=1024, X=1024, ws_bytes=1 << 40), b'voxels'),
                     (dict(w=(0, 1, 1)), b'weights'), (dict(w=(256, 0, 0)), b'weights'), (dict(w=(1, -1, 0)), b'weights'), (dict(w=(1, 256, 0)), b'weights'),
                     (dict(w=(1, 0, -1)), b'weights'), (dict(w=(1, 0, 256)), b'weights'),
                     (dict(Z=1024, Y=1024, X=1024, ws_bytes=1 << 40), b'overflow'),                  # chamfer at 1024^3
                     (dict(Z=1024, Y=1024, X=1024, w=(2, 0, 0), ws_bytes=1 << 40), b'overflow'),
                     (dict(Z=715827883, Y=1, X=1, w=(1, 3, 0), ws_bytes=1 << 40), b'overflow'),       # 3 N = 2^31 + 1
                     (dict(Z=2 ** 31 - 1, Y=1, X=1, w=(1, 0, 0), ws_bytes=1 << 40), b'overflow'),     # N = 2^31 - 1 itself
                     (dict(rounds=0), b'rounds'), (dict(rounds=-1), b'rounds'), (dict(rounds=1025), b'rounds'),
                     (dict(ws_bytes=n8 - 1), b'workspace'), (dict(ws=odd8), b'aligned'), (dict(changed=at((1 << 20) + 2)), b'aligned'),
                     (dict(changed=buf), b'overlap'), (dict(changed=at(n8 - 4)), b'overlap')):
        rc, msg = relax(**kw)
        assert rc < 0 and word in msg and msg.startswith(b'geo_relax:'), (kw, msg)
    # the accepted limits get as far as the workspace
    for kw in (dict(Z=1024, Y=1024, X=1024, w=(1, 1, 1)), dict(Z=715827882, Y=1, X=1, w=(3, 0, 0)), dict(Z=2 ** 31 - 2, Y=1, X=1, w=(1, 0, 0)),
               dict(w=(255, 255, 255)), dict(rounds=1024)):
        rc, msg = relax(ws_bytes=0, **kw)
        assert rc < 0 and b'workspace' in msg, (kw, msg)

    def finish(ws=buf, ws_bytes=None, Z=8, Y=8, X=8, labels=far, g=further, fallback=None, offset=0):
        ws_bytes = need(Z, Y, X) if ws_bytes is None else ws_bytes
        return l.iunet_geo_finish(ws, ws_bytes, Z, Y, X, labels, g, fallback, offset, None), l.iunet_last_error()
    fb = at(3 << 20)
    for kw, word in ((dict(ws=None), b'null'), (dict(labels=None), b'null'), (dict(Y=0), b'dimension'),
                     (dict(Z=2048, Y=1024, X=1024, ws_bytes=1 << 40), b'voxels'), (dict(offset=-1), b'offset'),
                     (dict(ws_bytes=n8 - 1), b'workspace'), (dict(ws=odd8), b'aligned'), (dict(labels=at((1 << 20) + 2)), b'aligned'),
                     (dict(g=at((2 << 20) + 2)), b'aligned'), (dict(fallback=at((3 << 20) + 2)), b'aligned'),
                     (dict(labels=buf), b'overlap'), (dict(labels=at(n8 - 4)), b'overlap'), (dict(g=buf), b'overlap'), (dict(g=at(n8 - 4)), b'overlap'),
                     (dict(g=far), b'overlap'), (dict(g=at((1 << 20) + 4 * 511)), b'overlap'),
                     (dict(fallback=far), b'overlap'), (dict(fallback=further), b'overlap'), (dict(fallback=fb, labels=at((3 << 20) + 4 * 511)), b'overlap'),
                     (dict(g=None, fallback=far), b'overlap')):
        rc, msg = finish(**kw)
        assert rc < 0 and word in msg and msg.startswith(b'geo_finish:'), (kw, msg)
