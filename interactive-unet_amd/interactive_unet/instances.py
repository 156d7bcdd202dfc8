"""Nearest-seed feature transform and instance labels of a predicted volume (not in the reference; DESIGN.md section 26, defined by
tests/instances_ref.py): touching objects split, each counted and measured on its own.

  nearest(src, target, invert)                 (d2, idx) int32 [Z, Y, X]: the squared distance to the nearest voxel of the target class
                                               (invert: outside it) and that voxel's raster index (z Y + y) X + x; of equally near ones the
                                               smallest index; INF = 2^31 - 1 and -1 everywhere when there is none
  nearest_labelled(labels)                     the same to the nearest voxel with a label > 0 of an int32 label map
  expand_labels(labels, distance)              int32 [Z, Y, X]: every voxel within `distance` of a labelled voxel takes the nearest one's label
  split_touching(src, target, radius, conn)    (labels, count): the objects of the target class, those that touch through a neck a ball of
                                               `radius` cannot pass split at it; numbered 1 .. count in order of their first voxel
  instance_table(labels, count)                (sizes, first) int32 [count + 1] of the labels 0 .. count

src is uint8 as in morphology.py: a class map [Z, Y, X] or a predicted volume [Z, Y, X, C].  The cells are Euclidean (the nearest core in a
straight line), not geodesic: this is no watershed.  Resident volumes (CUDA tensors) go through libiunet (iunet_edt_sq, iunet_cc_label,
iunet_edt_feature, iunet_edt_feature_mask, iunet_edt_assign, iunet_cc_table, iunet_label_remap) and stay on the device; numpy arrays take
the numpy / scipy path below, which yields the same integers.  A missing library is an error."""
import numpy as np
import torch

from . import components, morphology, resident
from .morphology import INF, MAX_SQ


def _check_labels(labels, name='labels'):
    """Validated (on_device, Z, Y, X) of an int32 map [Z, Y, X]."""
    dev = torch.is_tensor(labels)
    if not (dev or isinstance(labels, np.ndarray)):
        raise ValueError(f'{name} must be a CUDA int32 tensor or a numpy int32 array')
    if dev and not labels.is_cuda:
        raise ValueError(f'resident {name} must be a CUDA tensor (a host map goes in as a numpy array)')
    if labels.dtype != (torch.int32 if dev else np.int32):
        raise ValueError(f'{name} must be int32, got {labels.dtype}')
    if not (labels.is_contiguous() if dev else labels.flags['C_CONTIGUOUS']):
        raise ValueError(f'{name} must be contiguous')
    if labels.ndim != 3 or min(labels.shape) < 1:
        raise ValueError(f'{name} must be [Z, Y, X], got {tuple(labels.shape)}')
    Z, Y, X = (int(n) for n in labels.shape)
    if Z * Y * X > resident.MAX_VOXELS:
        raise ValueError(f'volume {Z} x {Y} x {X}: more than 2^31 - 1 voxels')
    if (Z - 1) ** 2 + (Y - 1) ** 2 + (X - 1) ** 2 > MAX_SQ:
        raise ValueError(f'volume {Z} x {Y} x {X}: its squared diagonal passes 2^31 - 2')
    return dev, Z, Y, X


def _bound_sq(value, name):
    """floor(value^2) of a radius or a distance: morphology's rule, under the argument's own name."""
    try:
        return morphology._radius_sq(value)
    except ValueError as e:
        raise ValueError(str(e).replace('radius', name, 1)) from None


def _connectivity(connectivity):
    if connectivity not in components.CONNECTIVITIES:
        raise ValueError(f'connectivity {connectivity}: one of {components.CONNECTIVITIES}')
    return int(connectivity)


# ---- the device path: one call each ----
def _feature_ws(Z, Y, X, device):
    from . import _native as nv
    ws_bytes = nv.lib().iunet_edt_feature_ws_bytes(Z, Y, X)
    return torch.empty(ws_bytes, dtype=torch.uint8, device=device), ws_bytes


def _feature(src, Z, Y, X, C, target, invert):
    from . import _native as nv
    d2 = torch.empty((Z, Y, X), dtype=torch.int32, device=src.device)
    idx = torch.empty_like(d2)
    ws, ws_bytes = _feature_ws(Z, Y, X, src.device)
    with torch.cuda.device(src.device):
        nv.call('iunet_edt_feature', nv.ptr(src), Z, Y, X, C, target, int(invert), nv.ptr(d2), nv.ptr(idx), None, nv.ptr(ws), ws_bytes, nv.stream())
    return d2, idx


def _feature_mask(prev, Z, Y, X, r2, above):
    from . import _native as nv
    d2, idx = torch.empty_like(prev), torch.empty_like(prev)
    ws, ws_bytes = _feature_ws(Z, Y, X, prev.device)
    with torch.cuda.device(prev.device):
        nv.call('iunet_edt_feature_mask', nv.ptr(prev), Z, Y, X, r2, int(above), nv.ptr(d2), nv.ptr(idx), nv.ptr(ws), ws_bytes, nv.stream())
    return d2, idx


def _assign(idx, d2, seed_labels, Z, Y, X, r2, group=None, offset=0):
    from . import _native as nv
    out = torch.empty_like(idx)
    with torch.cuda.device(idx.device):
        nv.call('iunet_edt_assign', nv.ptr(idx), nv.ptr(d2), nv.ptr(seed_labels), nv.ptr(group) if group is not None else None, offset,
                Z, Y, X, r2, nv.ptr(out), nv.stream())
    return out


def _label(mask, Z, Y, X, connectivity):
    """(labels, count) of a resident uint8 map's voxels above 0: iunet_cc_label without its class map."""
    from . import _native as nv
    labels = torch.empty((Z, Y, X), dtype=torch.int32, device=mask.device)
    count = torch.empty(1, dtype=torch.int32, device=mask.device)
    ws_bytes = nv.lib().iunet_cc_ws_bytes(Z, Y, X)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=mask.device)
    with torch.cuda.device(mask.device):
        nv.call('iunet_cc_label', nv.ptr(mask), Z, Y, X, 1, connectivity, 0, nv.ptr(labels), None, nv.ptr(count), nv.ptr(ws), ws_bytes, nv.stream())
    return labels, int(count.item())


def _table(labels, cls, Z, Y, X, K):
    """(sizes, first) of iunet_cc_table; cls: any map of one byte per voxel (the classes it yields are not kept)."""
    from . import _native as nv
    sizes = torch.empty(K + 1, dtype=torch.int32, device=labels.device)
    first = torch.empty(K + 1, dtype=torch.int32, device=labels.device)
    classes = torch.empty(K + 1, dtype=torch.uint8, device=labels.device)
    with torch.cuda.device(labels.device):
        nv.call('iunet_cc_table', nv.ptr(labels), nv.ptr(cls), Z, Y, X, K, nv.ptr(sizes), nv.ptr(classes), nv.ptr(first), nv.stream())
    return sizes, first


# ---- the host path ----
def _host_axis(f, at, axis):
    """One pass of the separable transform along `axis`: for every u the minimum of f(i) + (u - i)^2 and `at` of the first i attaining it."""
    n = f.shape[axis]
    f, at = np.moveaxis(f, axis, 0), np.moveaxis(at, axis, 0)
    g, to = np.empty_like(f), np.empty_like(at)
    pos = np.arange(n, dtype=np.int64).reshape((n,) + (1,) * (f.ndim - 1))
    for u in range(n):
        cost = f + (pos - u) ** 2
        first = cost.argmin(axis=0)[None]                             # the first of equal minima: the smallest i
        g[u], to[u] = np.take_along_axis(cost, first, 0)[0], np.take_along_axis(at, first, 0)[0]
    return np.moveaxis(g, 0, axis), np.moveaxis(to, 0, axis)


def _host_feature(seeds):
    big = np.int64(1) << 40
    f = np.where(seeds, np.int64(0), big)
    at = np.arange(seeds.size, dtype=np.int64).reshape(seeds.shape)
    for axis in (2, 1, 0):
        f, at = _host_axis(f, at, axis)
    none = f >= big
    # C order: the passes leave their axis last in memory, and numpy keeps that layout
    return np.ascontiguousarray(np.where(none, INF, f), dtype=np.int32), np.ascontiguousarray(np.where(none, -1, at), dtype=np.int32)


def _host_assign(idx, d2, seed_labels, r2, group=None, offset=0):
    reached = (idx >= 0) & (d2 <= r2)
    to = np.where(idx >= 0, idx, 0)
    if group is None:
        return np.where(reached, seed_labels.reshape(-1)[to], 0).astype(np.int32)
    own = reached & (group.reshape(-1)[to] == group)
    return np.where(group == 0, 0, np.where(own, seed_labels.reshape(-1)[to], offset + group)).astype(np.int32)


# ---- the functions ----
def nearest(src, target=1, invert=False):
    """(d2, idx) int32 [Z, Y, X] of the voxels of class `target` (invert: of the voxels outside it, the never-predicted ones included)."""
    dev, Z, Y, X, C = resident.check_volume(src, MAX_SQ)
    target = resident.check_byte(target, 'target')
    if dev:
        return _feature(src, Z, Y, X, C, target, bool(invert))
    cls, has = resident.host_maps(src)
    a = has & (cls == target)
    return _host_feature(~a if invert else a)


def nearest_labelled(labels):
    """(d2, idx) int32 [Z, Y, X] of the voxels whose label is above 0."""
    dev, Z, Y, X = _check_labels(labels)
    if dev:
        return _feature_mask(labels, Z, Y, X, 0, True)
    return _host_feature(labels > 0)


def expand_labels(labels, distance):
    """int32 [Z, Y, X]: every voxel within `distance` of a labelled voxel (label > 0) takes the label of the nearest one -- of equally near
    ones the one with the smallest raster index -- and the others 0; a labelled voxel keeps its label.  skimage.segmentation.expand_labels
    with the tie rule stated."""
    dev, Z, Y, X = _check_labels(labels)
    r2 = _bound_sq(distance, 'distance')
    if dev:
        d2, idx = _feature_mask(labels, Z, Y, X, 0, True)
        return _assign(idx, d2, labels, Z, Y, X, r2)
    d2, idx = _host_feature(labels > 0)
    return _host_assign(idx, d2, labels, r2)


def split_touching(src, target, radius, connectivity=6):
    """(labels int32 [Z, Y, X], count): 0 off class `target`.  The cores are the components of the class eroded by the ball of `radius`
    (the outside of the volume does not erode); every voxel of an object -- a component of the class -- takes the nearest core of its own
    object; an object too small to have a core, and the voxels of an object whose nearest core lies in another object, form one instance
    per object.  Numbered in increasing order of the instances' first voxels.  CUDA src: count is read back as a Python int."""
    dev, Z, Y, X, C = resident.check_volume(src, MAX_SQ)
    target, r2, connectivity = resident.check_byte(target, 'target'), morphology._radius_sq(radius), _connectivity(connectivity)
    if dev:
        from . import _native as nv
        d_out = morphology._edt(src, Z, Y, X, C, target, True, want_cls=False)[0]      # the distance to the outside of A: > 0 exactly on A
        a = (d_out > 0).to(torch.uint8)
        la, ka = _label(a, Z, Y, X, connectivity)
        le, ke = _label((d_out > r2).to(torch.uint8), Z, Y, X, connectivity)
        d2e, idx = _feature_mask(d_out, Z, Y, X, r2, True)
        del d_out
        raw = _assign(idx, d2e, le, Z, Y, X, MAX_SQ, group=la, offset=ke)
        del d2e, idx, le, la
        # ke + ka <= Z Y X + 1 (along a snake through the volume the objects are at most the runs of A: ka <= Z Y X - |A| + 1, and ke <= |A|),
        # with equality only where every voxel of A is a core and an object of its own: no remainder label occurs then, so the table of
        # the labels up to Z Y X, the most iunet_cc_table takes, still holds every label of raw
        K = min(ke + ka, Z * Y * X)
        sizes, first = _table(raw, a, Z, Y, X, K)
        # the K-entry plumbing: the labels that occur, in order of their first voxel
        there = sizes[1:] > 0
        order = torch.sort(torch.where(there, first[1:], torch.full_like(first[1:], INF)).to(torch.int64), stable=True).indices
        count = int(there.sum().item())
        number = torch.zeros(K + 1, dtype=torch.int32, device=src.device)
        number[order[:count] + 1] = torch.arange(1, count + 1, dtype=torch.int32, device=src.device)
        with torch.cuda.device(src.device):
            nv.call('iunet_label_remap', nv.ptr(raw), Z, Y, X, K, nv.ptr(number), nv.stream())
        return raw, count
    cls, has = resident.host_maps(src)
    a = has & (cls == target)
    d_out = morphology._host_d2(~a)
    la, ka, _ = components.label(a.astype(np.uint8), connectivity)
    le, ke, _ = components.label((d_out > r2).astype(np.uint8), connectivity)
    d2e, idx = _host_feature(d_out > r2)
    raw = _host_assign(idx, d2e, le, MAX_SQ, group=la, offset=ke)
    _, first = instance_table(raw, ke + ka)
    there = np.flatnonzero(first[1:] >= 0)
    number = np.zeros(ke + ka + 1, dtype=np.int32)
    number[there[np.argsort(first[1:][there], kind='stable')] + 1] = np.arange(1, len(there) + 1, dtype=np.int32)
    return number[raw], len(there)


def instance_table(labels, count):
    """(sizes int32 [count + 1], first int32 [count + 1]): the voxels and the raster index of the first voxel of each label 0 .. count;
    entry 0 (no instance) is (0, -1).  A thin call of iunet_cc_table."""
    dev, Z, Y, X = _check_labels(labels)
    K = resident.check_count(count, 'count', 'the number of instances, an int >= 0')
    if dev:
        # iunet_cc_table also reads a byte per voxel for the classes, which instances do not have: the labels' own first bytes serve
        return _table(labels, labels, Z, Y, X, K)
    flat = labels.reshape(-1)
    keep = (flat > 0) & (flat <= K)
    sizes = np.bincount(flat[keep], minlength=K + 1)[:K + 1].astype(np.int32)
    first = np.full(K + 1, -1, dtype=np.int32)
    at = np.flatnonzero(keep)
    found, where = np.unique(flat[at], return_index=True)
    first[found] = at[where]
    return sizes, first
