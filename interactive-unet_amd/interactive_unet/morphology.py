"""Exact distance transform and ball morphology of a predicted volume (not in the reference; DESIGN.md section 23, defined by
tests/morphology_ref.py): how far every voxel is from a class, a ragged boundary smoothed, thin bridges cut, pin-holes closed.

  distance_sq(src, target, invert)         int32 [Z, Y, X]: the squared distance to the nearest voxel of the target class (invert: to the
                                           nearest voxel outside it); INF = 2^31 - 1 everywhere when there is none
  class_map(src)                           uint8 [Z, Y, X]
  dilate / erode / opening / closing       the class map with the target class grown, shrunk, opened or closed by a ball of `radius`
  fill_holes(src, target, connectivity)    the class map with the holes of the target class filled

src is uint8: a class map [Z, Y, X], or a predicted volume [Z, Y, X, C], 2 <= C <= 16, whose voxels take the class of their largest byte
(the lowest index on a tie; a voxel whose bytes are all 0 was never predicted: it has no class, 0 in the class map, and is outside every
target).  A ball of radius r is {dz^2 + dy^2 + dx^2 <= floor(r r)}; the outside of the volume does not erode.  Resident volumes (CUDA uint8
tensors) go through libiunet (iunet_edt_sq, iunet_edt_sq_mask, iunet_edt_select) and stay on the device; numpy arrays take the scipy path
below, which yields the same integers.  A missing library is an error."""
import math

import numpy as np
import torch

from . import components, resident

INF = 2 ** 31 - 1
MAX_SQ = 2 ** 31 - 2              # the largest finite squared distance: the squared diagonal of the volume may not pass it


def _radius_sq(radius):
    if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)) or not math.isfinite(radius) or radius < 0:
        raise ValueError(f'radius {radius!r}: a finite number >= 0')
    r2 = int(math.floor(float(radius) * float(radius)))
    if r2 > MAX_SQ:
        raise ValueError(f'radius {radius!r}: its square passes 2^31 - 2')
    return r2


def _host_d2(seeds):
    from scipy import ndimage
    if not seeds.any():
        return np.full(seeds.shape, INF, dtype=np.int32)
    return np.rint(ndimage.distance_transform_edt(~seeds) ** 2).astype(np.int32)


def _edt(src, Z, Y, X, C, target, invert, want_d2=True, want_cls=True):
    """(d2, cls, ws, ws_bytes) of iunet_edt_sq on a resident src."""
    from . import _native as nv
    d2 = torch.empty((Z, Y, X), dtype=torch.int32, device=src.device) if want_d2 else None
    cls = torch.empty((Z, Y, X), dtype=torch.uint8, device=src.device) if want_cls else None
    ws_bytes = nv.lib().iunet_edt_ws_bytes(Z, Y, X) if want_d2 else 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=src.device) if want_d2 else None
    with torch.cuda.device(src.device):
        nv.call('iunet_edt_sq', nv.ptr(src), Z, Y, X, C, target, int(invert), nv.ptr(d2), nv.ptr(cls), nv.ptr(ws), ws_bytes, nv.stream())
    return d2, cls, ws, ws_bytes


def _edt_mask(prev, Z, Y, X, r2, above, ws, ws_bytes):
    from . import _native as nv
    d2 = torch.empty_like(prev)
    with torch.cuda.device(prev.device):
        nv.call('iunet_edt_sq_mask', nv.ptr(prev), Z, Y, X, r2, int(above), nv.ptr(d2), nv.ptr(ws), ws_bytes, nv.stream())
    return d2


def _select(d2, cls, Z, Y, X, r2, above, only, value):
    """In place on cls (which this module has just made)."""
    from . import _native as nv
    with torch.cuda.device(cls.device):
        nv.call('iunet_edt_select', nv.ptr(d2), nv.ptr(cls), Z, Y, X, r2, int(above), only, value, nv.ptr(cls), nv.stream())
    return cls


def _never_to_zero(out, src, C, target, fill):
    """A never-predicted voxel shows as 0 in the class map and is no member of class 0: where the target is 0 and `only` met it, it
    gets its 0 back (predicted volumes with target 0 and a fill other than 0 only)."""
    if C >= 2 and target == 0 and fill != 0:
        out[src.amax(dim=-1) == 0] = 0
    return out


def distance_sq(src, target=1, invert=False):
    """int32 [Z, Y, X]: the squared Euclidean distance of every voxel to the nearest voxel of class `target` (invert: to the nearest voxel
    that is not of that class, the never-predicted ones included); 0 on those voxels, INF = 2^31 - 1 everywhere when there is none."""
    dev, Z, Y, X, C = resident.check_volume(src, MAX_SQ)
    target = resident.check_byte(target, 'target')
    if dev:
        return _edt(src, Z, Y, X, C, target, bool(invert), want_cls=False)[0]
    cls, has = resident.host_maps(src)
    a = has & (cls == target)
    return _host_d2(~a if invert else a)


def class_map(src):
    """uint8 [Z, Y, X]: the class of every voxel, 0 for a voxel never predicted."""
    dev, Z, Y, X, C = resident.check_volume(src, MAX_SQ)
    if dev:
        return _edt(src, Z, Y, X, C, 0, False, want_d2=False)[1]
    return resident.host_maps(src)[0]


def dilate(src, target, radius):
    """The class map with every voxel within `radius` of class `target` set to it."""
    dev, Z, Y, X, C = resident.check_volume(src, MAX_SQ)
    target, r2 = resident.check_byte(target, 'target'), _radius_sq(radius)
    if dev:
        d2, cls, _, _ = _edt(src, Z, Y, X, C, target, False)
        return _select(d2, cls, Z, Y, X, r2, False, -1, target)
    cls, has = resident.host_maps(src)
    cls[_host_d2(has & (cls == target)) <= r2] = target
    return cls


def erode(src, target, radius, fill=0):
    """The class map with the voxels of class `target` within `radius` of a voxel outside it set to `fill`."""
    dev, Z, Y, X, C = resident.check_volume(src, MAX_SQ)
    target, fill, r2 = resident.check_byte(target, 'target'), resident.check_byte(fill, 'fill'), _radius_sq(radius)
    if dev:
        d2, cls, _, _ = _edt(src, Z, Y, X, C, target, True)
        return _never_to_zero(_select(d2, cls, Z, Y, X, r2, False, target, fill), src, C, target, fill)
    cls, has = resident.host_maps(src)
    a = has & (cls == target)
    cls[a & (_host_d2(~a) <= r2)] = fill
    return cls


def opening(src, target, radius, fill=0):
    """Erosion then dilation of class `target` by the ball: what the ball cannot enter -- thin bridges, a ragged rim -- is set to `fill`."""
    dev, Z, Y, X, C = resident.check_volume(src, MAX_SQ)
    target, fill, r2 = resident.check_byte(target, 'target'), resident.check_byte(fill, 'fill'), _radius_sq(radius)
    if dev:
        inner, cls, ws, ws_bytes = _edt(src, Z, Y, X, C, target, True)          # the distance to the outside of A: > r2 on the eroded set
        d2 = _edt_mask(inner, Z, Y, X, r2, True, ws, ws_bytes)                  # the distance to the eroded set
        return _never_to_zero(_select(d2, cls, Z, Y, X, r2, True, target, fill), src, C, target, fill)
    cls, has = resident.host_maps(src)
    a = has & (cls == target)
    cls[a & (_host_d2(_host_d2(~a) > r2) > r2)] = fill
    return cls


def closing(src, target, radius):
    """Dilation then erosion of class `target` by the ball: gaps and pin-holes the ball cannot enter take the target."""
    dev, Z, Y, X, C = resident.check_volume(src, MAX_SQ)
    target, r2 = resident.check_byte(target, 'target'), _radius_sq(radius)
    if dev:
        outer, cls, ws, ws_bytes = _edt(src, Z, Y, X, C, target, False)         # the distance to A: <= r2 on the dilated set
        d2 = _edt_mask(outer, Z, Y, X, r2, True, ws, ws_bytes)                  # the distance to the outside of the dilated set
        return _select(d2, cls, Z, Y, X, r2, True, -1, target)
    cls, has = resident.host_maps(src)
    cls[_host_d2(_host_d2(has & (cls == target)) > r2) > r2] = target
    return cls


def fill_holes(src, target, connectivity=6):
    """The class map with the holes of class `target` -- the components of its complement, under the 6-, 18- or 26-neighbourhood, that
    touch none of the six faces of the volume -- set to it.  No kernel of its own: the complement is labelled by components.label."""
    dev, Z, Y, X, C = resident.check_volume(src, MAX_SQ)
    target = resident.check_byte(target, 'target')
    if connectivity not in components.CONNECTIVITIES:
        raise ValueError(f'connectivity {connectivity}: one of {components.CONNECTIVITIES}')
    if dev:
        cls = class_map(src)
        outside = cls != target
        if C >= 2 and target == 0:
            outside |= src.amax(dim=-1) == 0                                    # never predicted: 0 in the class map, no member of class 0
        labels, K, _ = components.label(outside.to(torch.uint8), connectivity, background=0)
        keep = torch.zeros(K + 1, dtype=torch.uint8, device=src.device)
        for face in (labels[0], labels[-1], labels[:, 0], labels[:, -1], labels[:, :, 0], labels[:, :, -1]):
            keep[face.reshape(-1).long()] = 1
        return components.filter_components(labels, cls, K, keep, fill=target)
    from scipy import ndimage
    cls, has = resident.host_maps(src)
    a = has & (cls == target)
    cls[ndimage.binary_fill_holes(a, structure=ndimage.generate_binary_structure(3, components.CONNECTIVITIES.index(connectivity) + 1)) & ~a] = target
    return cls
