"""Geodesic seeded growth through a predicted volume (not in the reference; DESIGN.md section 27, defined by tests/geodesic_ref.py):
integer seed labels grow through a domain along the shortest path INSIDE the domain, and touching objects are split by such paths.

  grow(src, seeds, target, metric)             (labels, g) int32 [Z, Y, X]: through the voxels of class `target` of src
  grow_in(domain, seeds, metric)               the same through {domain > 0} of an int32 map
  split_touching(src, target, radius, conn, metric)
                                               (labels, count): instances.split_touching with geodesic cells -- every voxel of an object
                                               takes the core it reaches by the shortest path inside the class; no path leaves an object
  split_from_seeds(a, seeds, count, ...)       the tail of such a split (grow, fallback, renumber), for reconstruction.py's markers too

src is uint8 as in morphology.py: a class map [Z, Y, X] or a predicted volume [Z, Y, X, C].  seeds is an int32 [Z, Y, X] map: the voxels
of the domain with seeds > 0 are the seeds, the value is their label; an entry off the domain is ignored.  metric: 6, 18, 26 (unit steps
to face / face and edge / all neighbours), 'chamfer' (3, 4, 5), or three integer weights (w1, w2, w3) for a step to a face, edge and
vertex neighbour (0: no such step; 1 <= w1 <= 255, the others 0 .. 255).  g is the least weight of a path inside the domain to a seed:
0 on a seed, INF = 2^31 - 1 off the domain and where no seed can be reached.  labels holds the SMALLEST label among the seeds at that
distance (this is not instances.py's smallest-raster-index rule: it is what makes the result independent of the order of relaxation),
0 where g is INF.  Z Y X max(w) <= 2^31 - 2, so that no distance overflows.

Resident volumes (CUDA tensors) go through libiunet (iunet_geo_init, iunet_geo_init_mask, iunet_geo_relax, iunet_geo_finish; for the
split also iunet_edt_sq, iunet_cc_label, iunet_cc_table, iunet_label_remap) and stay on the device; numpy arrays take the numpy path
below, which yields the same integers.  A missing library is an error."""
import numpy as np
import torch

from . import components, instances, morphology, resident
from .morphology import INF, MAX_SQ

METRICS = {6: (1, 0, 0), 18: (1, 1, 0), 26: (1, 1, 1), 'chamfer': (3, 4, 5)}
MAX_DIST = 2 ** 31 - 2
ROUNDS_PER_CALL = 8                                                   # rounds between two reads of the 4-byte `changed`
_MAX_CALL = 1024                                                      # iunet_geo_relax's limit


def _weights(metric):
    """(w1, w2, w3) of a named metric or of three integer weights."""
    if isinstance(metric, (str, int, np.integer)) and not isinstance(metric, bool):
        if metric not in METRICS:
            raise ValueError(f"metric {metric!r}: one of 6, 18, 26, 'chamfer', or three weights (w1, w2, w3)")
        return METRICS[metric]
    if not isinstance(metric, (tuple, list)) or len(metric) != 3 or not all(resident.is_int(w) for w in metric):
        raise ValueError(f"metric {metric!r}: one of 6, 18, 26, 'chamfer', or three integer weights (w1, w2, w3)")
    w = tuple(int(x) for x in metric)
    if not (1 <= w[0] <= 255 and 0 <= w[1] <= 255 and 0 <= w[2] <= 255):
        raise ValueError(f'metric {metric!r}: w1 in 1 .. 255, w2 and w3 in 0 .. 255')
    return w


def _check_overflow(Z, Y, X, weights):
    if Z * Y * X * max(weights) > MAX_DIST:
        raise ValueError(f'volume {Z} x {Y} x {X} at step weight {max(weights)}: a distance could pass 2^31 - 2')


def _check_rounds(max_rounds, Z, Y, X):
    if max_rounds is None:
        return Z * Y * X + 1                                          # a proof bound: Bellman-Ford needs at most |A| sweeps
    if not resident.is_int(max_rounds) or max_rounds < 1:
        raise ValueError(f'max_rounds {max_rounds!r}: an int >= 1, or None')
    return int(max_rounds)


# ---- the device path ----
def _relax(ws, ws_bytes, Z, Y, X, weights, max_rounds):
    """Rounds of iunet_geo_relax until no tile changes; the 4-byte count is read back once per call."""
    from . import _native as nv
    changed = torch.empty(1, dtype=torch.int32, device=ws.device)
    done = 0
    while done < max_rounds:
        rounds = min(ROUNDS_PER_CALL, _MAX_CALL, max_rounds - done)
        nv.call('iunet_geo_relax', nv.ptr(ws), ws_bytes, Z, Y, X, weights[0], weights[1], weights[2], rounds, nv.ptr(changed), nv.stream())
        done += rounds
        if int(changed.item()) == 0:
            return done
    raise RuntimeError(f'geodesic growth: still changing after {done} rounds (max_rounds)')


def _grow_device(src, dom, seeds, Z, Y, X, C, target, weights, max_rounds, want_g=True, fallback=None, offset=0):
    from . import _native as nv
    device = seeds.device
    ws_bytes = nv.lib().iunet_geo_ws_bytes(Z, Y, X)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    labels = torch.empty((Z, Y, X), dtype=torch.int32, device=device)
    g = torch.empty_like(labels) if want_g else None
    with torch.cuda.device(device):
        if dom is None:
            nv.call('iunet_geo_init', nv.ptr(src), Z, Y, X, C, target, nv.ptr(seeds), nv.ptr(ws), ws_bytes, nv.stream())
        else:
            nv.call('iunet_geo_init_mask', nv.ptr(dom), Z, Y, X, nv.ptr(seeds), nv.ptr(ws), ws_bytes, nv.stream())
        _relax(ws, ws_bytes, Z, Y, X, weights, max_rounds)
        nv.call('iunet_geo_finish', nv.ptr(ws), ws_bytes, Z, Y, X, nv.ptr(labels), nv.ptr(g) if want_g else None,
                nv.ptr(fallback) if fallback is not None else None, offset, nv.stream())
    return labels, g


# ---- the host path ----
_UNREACHED = np.int64(INF) << 32                                      # (INF, 0): a pair is one int64, g in the high word
_OFF = np.iinfo(np.int64).max


def _host_keys(a, seeds, weights, max_rounds):
    """The fixed point by whole-volume sweeps: every voxel of A against all its neighbours, until nothing changes."""
    Z, Y, X = a.shape
    key = np.where(a, np.where(seeds > 0, seeds.astype(np.int64), _UNREACHED), _OFF)
    steps = [((dz, dy, dx), np.int64(weights[abs(dz) + abs(dy) + abs(dx) - 1]) << 32) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
             if (dz, dy, dx) != (0, 0, 0) and weights[abs(dz) + abs(dy) + abs(dx) - 1]]
    pad = np.full((Z + 2, Y + 2, X + 2), _OFF, np.int64)
    for _ in range(max_rounds):
        pad[1:-1, 1:-1, 1:-1] = key
        best = key.copy()
        for (dz, dy, dx), w in steps:
            u = pad[1 + dz:1 + dz + Z, 1 + dy:1 + dy + Y, 1 + dx:1 + dx + X]
            np.minimum(best, np.where(u < _UNREACHED, u + w, _OFF), out=best)
        best[~a] = _OFF
        if np.array_equal(best, key):
            return key
        key = best
    raise RuntimeError(f'geodesic growth: still changing after {max_rounds} rounds (max_rounds)')


def _host_finish(key, fallback=None, offset=0):
    reached = key < _UNREACHED
    labels = np.where(reached, key & 0xffffffff, 0)
    if fallback is not None:
        labels = np.where(key == _UNREACHED, np.int64(offset) + fallback, labels)
    return labels.astype(np.int32), np.where(reached, key >> 32, INF).astype(np.int32)


# ---- the functions ----
def grow(src, seeds, target=1, metric='chamfer', max_rounds=None):
    """(labels, g) int32 [Z, Y, X]: the seeds grown through the voxels of class `target`.  max_rounds: a RuntimeError when the growth has
    not come to rest after that many rounds (default Z Y X + 1, which no input reaches)."""
    dev, Z, Y, X, C = resident.check_volume(src)
    target, weights = resident.check_byte(target, 'target'), _weights(metric)
    resident.check_map(seeds, 'seeds', (dev, Z, Y, X))
    _check_overflow(Z, Y, X, weights)
    max_rounds = _check_rounds(max_rounds, Z, Y, X)
    if dev:
        if seeds.device != src.device:
            raise ValueError(f'seeds on {seeds.device}, src on {src.device}')
        return _grow_device(src, None, seeds, Z, Y, X, C, target, weights, max_rounds)
    cls, has = resident.host_maps(src)
    return _host_finish(_host_keys(has & (cls == target), seeds, weights, max_rounds))


def grow_in(domain, seeds, metric='chamfer', max_rounds=None):
    """(labels, g) int32 [Z, Y, X]: the seeds grown through {domain > 0} of an int32 map (a label map: through its labelled voxels)."""
    dev, Z, Y, X = resident.check_map(domain, 'domain')
    weights = _weights(metric)
    resident.check_map(seeds, 'seeds', (dev, Z, Y, X))
    _check_overflow(Z, Y, X, weights)
    max_rounds = _check_rounds(max_rounds, Z, Y, X)
    if dev:
        if seeds.device != domain.device:
            raise ValueError(f'seeds on {seeds.device}, domain on {domain.device}')
        return _grow_device(None, domain, seeds, Z, Y, X, 1, 0, weights, max_rounds)
    return _host_finish(_host_keys(domain > 0, seeds, weights, max_rounds))


def split_weights(metric, connectivity):
    """The metric's weights inside objects of `connectivity`: a step to a neighbour the connectivity does not count as one does not exist
    (it would join two objects), so the weights above the connectivity's rank are 0."""
    rank = {6: 1, 18: 2, 26: 3}[connectivity]
    return tuple(w if k < rank else 0 for k, w in enumerate(_weights(metric)))


def split_from_seeds(a, seeds, count, connectivity, weights, max_rounds):
    """(labels int32 [Z, Y, X], instances): the tail of a split, written once for split_touching here and in reconstruction.py.  a: A as
    a resident uint8 map (1 on A) or a numpy bool map; seeds: a ONE-ELEMENT LIST holding the int32 map of labels 1 .. count on A
    (validated by the caller, as weights and max_rounds) -- the list is emptied here and the map released once it has grown, so a caller
    that keeps no other reference does not hold it through the table, sort and remap.  The seeds grow through A; the voxels of A none
    reaches take count + the label of their object (a component of A under `connectivity`); the labels that occur are renumbered in
    increasing order of their first voxels."""
    Z, Y, X = (int(n) for n in a.shape)
    seeds = seeds.pop()
    if torch.is_tensor(a):
        from . import _native as nv
        la, ka = instances._label(a, Z, Y, X, connectivity)
        raw, _ = _grow_device(a, None, seeds, Z, Y, X, 1, 1, weights, max_rounds, want_g=False, fallback=la, offset=count)
        del seeds, la
        K = min(count + ka, Z * Y * X)                                # instances.split_touching's bound: every label of raw is <= K
        sizes, first = instances._table(raw, a, Z, Y, X, K)
        # the K-entry plumbing: the labels that occur, in order of their first voxel
        there = sizes[1:] > 0
        order = torch.sort(torch.where(there, first[1:], torch.full_like(first[1:], INF)).to(torch.int64), stable=True).indices
        found = int(there.sum().item())
        number = torch.zeros(K + 1, dtype=torch.int32, device=a.device)
        number[order[:found] + 1] = torch.arange(1, found + 1, dtype=torch.int32, device=a.device)
        with torch.cuda.device(a.device):
            nv.call('iunet_label_remap', nv.ptr(raw), Z, Y, X, K, nv.ptr(number), nv.stream())
        return raw, found
    la, ka, _ = components.label(a.astype(np.uint8), connectivity)
    raw = _host_finish(_host_keys(a, seeds, weights, max_rounds), fallback=la, offset=count)[0]
    _, first = instances.instance_table(raw, count + ka)
    there = np.flatnonzero(first[1:] >= 0)
    number = np.zeros(count + ka + 1, dtype=np.int32)
    number[there[np.argsort(first[1:][there], kind='stable')] + 1] = np.arange(1, len(there) + 1, dtype=np.int32)
    return number[raw], len(there)


def split_touching(src, target, radius, connectivity=6, metric='chamfer', max_rounds=None):
    """(labels int32 [Z, Y, X], count): 0 off class `target`.  The cores are the components of the class eroded by the ball of `radius`
    (instances.split_touching's); every voxel of an object -- a component of the class -- takes the core nearest along paths inside the
    class, by steps between neighbours of `connectivity` (split_weights), the smallest core label among equally near ones; the voxels no
    core reaches form one instance per object.  Numbered in increasing order of the instances' first voxels.  CUDA src: count is read back
    as a Python int."""
    dev, Z, Y, X, C = resident.check_volume(src, MAX_SQ)
    target, r2 = resident.check_byte(target, 'target'), morphology._radius_sq(radius)
    connectivity = instances._connectivity(connectivity)
    weights = split_weights(metric, connectivity)
    _check_overflow(Z, Y, X, weights)
    max_rounds = _check_rounds(max_rounds, Z, Y, X)
    if dev:
        d_out = morphology._edt(src, Z, Y, X, C, target, True, want_cls=False)[0]      # the distance to the outside of A: > 0 exactly on A
        a = (d_out > 0).to(torch.uint8)
        le, ke = instances._label((d_out > r2).to(torch.uint8), Z, Y, X, connectivity)
        seeds = [le]
        del d_out, le
        return split_from_seeds(a, seeds, ke, connectivity, weights, max_rounds)
    cls, has = resident.host_maps(src)
    a = has & (cls == target)
    d_out = morphology._host_d2(~a)
    le, ke, _ = components.label((d_out > r2).astype(np.uint8), connectivity)
    return split_from_seeds(a, [le], ke, connectivity, weights, max_rounds)
