"""The definition of the geodesic seeded growth and of the instance split built on it: what iunet_geo_init,
iunet_geo_init_mask, iunet_geo_relax and iunet_geo_finish compute, and what interactive_unet/geodesic.py builds on them, restated with
numpy.  Nothing here imports the package.

Domain A: the member set of a target class of a uint8 src (tests/morphology_ref.py's rule: a class map [Z, Y, X], or a predicted volume
[Z, Y, X, C] whose class is the first largest byte and whose all-zero voxels belong to no class), or {dom > 0} of an int32 map.
Seeds: the voxels of A with seeds[v] > 0 (int32 [Z, Y, X]); the label is seeds[v]; a positive entry off A is ignored.
Metric: integer weights (w1, w2, w3) of a step to a face, edge and vertex neighbour; 0: that kind of step does not exist; w1 >= 1, all
<= 255.  METRICS names four of them.
g[v] (int32): the least total weight of a path from v to a seed whose every voxel lies in A; 0 on a seed; INF = 2^31 - 1 off A and where
no seed can be reached.  label[v] (int32): the smallest label among the seeds at distance exactly g[v] along such paths; 0 where g[v] = INF.
So (g, label), ordered lexicographically, is the one fixed point of
    key[v] = min(key[v], min over the neighbours u in A with g[u] < INF of (g[u] + w(u, v), label[u]))
that is reached from (0, label) on the seeds and (INF, 0) on the rest of A: written here as whole-volume Jacobi sweeps over shifted arrays
until nothing changes.  A pair is held as one uint64, g in the high word and the label in the low one, so that the order of the integers
is the order of the pairs.  Size limits: every dimension >= 1, Z Y X <= 2^31 - 1, and Z Y X max(w) <= 2^31 - 2 (no path is longer)."""
import numpy as np

from tests.instances_ref import class_map, components_of, feature_of, members, radius_sq, renumber  # noqa: F401 (the shared rules)

INF = 2 ** 31 - 1
MAX_SQ = 2 ** 31 - 2
METRICS = {6: (1, 0, 0), 18: (1, 1, 0), 26: (1, 1, 1), 'chamfer': (3, 4, 5)}
_UNREACHED = np.uint64(INF << 32)                                     # (INF, 0)
_OFF = np.uint64(2 ** 64 - 1)                                         # off A: above every pair (the workspace's own bytes)
_FAR = np.uint64(1 << 63)                                             # what a sweep reads for a neighbour that offers nothing
OFFSETS = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy, dx) != (0, 0, 0)]


def weights_of(metric):
    if isinstance(metric, (tuple, list)):
        w = tuple(int(x) for x in metric)
    else:
        w = METRICS[metric]
    assert len(w) == 3 and 1 <= w[0] <= 255 and 0 <= w[1] <= 255 and 0 <= w[2] <= 255
    return w


def limits_ok(Z, Y, X, weights=(1, 0, 0)):
    return min(Z, Y, X) >= 1 and Z * Y * X <= 2 ** 31 - 1 and Z * Y * X * max(weights) <= 2 ** 31 - 2


def keys_of(a, seeds):
    """The initial state, uint64 [Z, Y, X]."""
    a, seeds = np.asarray(a, dtype=bool), np.asarray(seeds)
    assert a.ndim == 3 and seeds.shape == a.shape
    return np.where(a, np.where(seeds > 0, np.maximum(seeds, 0).astype(np.uint64), _UNREACHED), _OFF)


def sweep(key, weights):
    """One Jacobi sweep: every voxel of A against the state of all its neighbours before the sweep.  A neighbour off A, outside the volume
    or not reached reads as _FAR: with any step added it stays above (INF, 0), the most a voxel of A holds, and below 2^64."""
    Z, Y, X = key.shape
    pad = np.full((Z + 2, Y + 2, X + 2), _FAR, np.uint64)
    pad[1:-1, 1:-1, 1:-1] = np.where(key < _UNREACHED, key, _FAR)
    best, cand = key.copy(), np.empty_like(key)
    for dz, dy, dx in OFFSETS:
        w = weights[abs(dz) + abs(dy) + abs(dx) - 1]
        if w == 0:
            continue
        np.add(pad[1 + dz:1 + dz + Z, 1 + dy:1 + dy + Y, 1 + dx:1 + dx + X], np.uint64(w << 32), out=cand)
        np.minimum(best, cand, out=best)
    return np.where(key == _OFF, _OFF, best)


def split_keys(key):
    """(labels int32, g int32) of a state."""
    reached = key < _UNREACHED
    return (np.where(reached, key & np.uint64(0xffffffff), np.uint64(0)).astype(np.int32),
            np.where(reached, key >> np.uint64(32), np.uint64(INF)).astype(np.int32))


def device_keys(key):
    """The state as the workspace holds it, read as int64: off A all ones."""
    return key.view(np.int64)


def grow_keys(a, seeds, metric='chamfer'):
    """The fixed point as uint64 keys, and the number of sweeps that changed something.  A sweep is a whole-volume Jacobi sweep; it is
    evaluated on the planes next to one that changed in the sweep before only, since no other voxel can change: the same states, sooner."""
    weights = weights_of(metric)
    key = keys_of(a, seeds)
    assert limits_ok(*key.shape, weights)
    Z = key.shape[0]
    sweeps, lo, hi = 0, 0, Z
    while True:
        z0, z1 = max(lo - 1, 0), min(hi + 1, Z)                       # the planes that can change
        h0, h1 = max(z0 - 1, 0), min(z1 + 1, Z)                       # and the planes they read
        nxt = sweep(key[h0:h1], weights)[z0 - h0:z1 - h0]
        differ = np.flatnonzero((nxt != key[z0:z1]).any(axis=(1, 2)))
        if len(differ) == 0:
            return key, sweeps
        key[z0:z1] = nxt
        sweeps, lo, hi = sweeps + 1, z0 + int(differ[0]), z0 + int(differ[-1]) + 1


def grow_in(dom, seeds, metric='chamfer'):
    """(labels int32, g int32) [Z, Y, X]: the seeds grown through A = {dom > 0} (a boolean map: A itself)."""
    return split_keys(grow_keys(np.asarray(dom) > 0, seeds, metric)[0])


def grow(src, seeds, target=1, metric='chamfer'):
    return grow_in(members(src, target), seeds, metric)


def finish(key, fallback=None, offset=0):
    """(labels, g) of a state; with fallback: labels[v] = offset + fallback[v] on the voxels of A no seed reaches."""
    labels, g = split_keys(key)
    if fallback is not None:
        labels = np.where(key == _UNREACHED, offset + np.asarray(fallback, dtype=np.int64), labels).astype(np.int32)
    return labels, g


# ---- the instance split: A, the distance to its outside, the cores, the components and the renumbering are section 26's ----
def split_weights(metric, connectivity):
    """Inside objects of `connectivity` a step to a neighbour that the connectivity does not count as one does not exist: it could join two
    objects.  The weights above the connectivity's rank are 0."""
    rank = {6: 1, 18: 2, 26: 3}[connectivity]
    return tuple(w if k < rank else 0 for k, w in enumerate(weights_of(metric)))


def split_touching(src, target, radius, connectivity=6, metric='chamfer', parts=False):
    """(labels int32 [Z, Y, X], K): the cores are the components of the erosion E = {d2(v, outside A) > r2}; every voxel of A takes the
    geodesically nearest core, by steps between neighbours of `connectivity`; the voxels of an object (a component of A) that no core
    reaches form one instance per object.  parts: also (KE, KA)."""
    a, r2 = members(src, target), radius_sq(radius)
    e = feature_of(~a)[0] > r2                                       # the outside of the volume does not erode
    assert not (e & ~a).any()
    le, ke = components_of(e, connectivity)
    la, ka = components_of(a, connectivity)
    labels, k = renumber(finish(grow_keys(a, le, split_weights(metric, connectivity))[0], fallback=la, offset=ke)[0])
    return (labels, k, ke, ka) if parts else (labels, k)
