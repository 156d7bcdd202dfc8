"""The definition of the exact distance transform and the ball morphology built on it: what iunet_edt_sq,
iunet_edt_sq_mask and iunet_edt_select compute, and what interactive_unet/morphology.py builds on them, restated with numpy and
scipy.ndimage.  Nothing here imports the package.

Input src, uint8: a class map [Z][Y][X] (every voxel has the class of its byte), or a predicted volume [Z][Y][X][C], 2 <= C <= 16 -- a
voxel's class is the index of its largest byte, the lowest index on a tie; a voxel whose bytes are all 0 was never predicted: it has no
class, and 0 in the class map cls.
Member set of a target 0 .. 255: A = {v: v has a class and class(v) == target}.  Seeds: S = A (invert 0) or its complement (invert 1; the
never-predicted voxels are in it).  Voxels outside the volume are never seeds.
d2 int32 [Z][Y][X]: d2[v] = min over s in S of |v - s|^2; 0 on S; INF = 2^31 - 1 everywhere when S is empty.
Seeds from a distance map prev: S = {prev > r2} (above) or {prev <= r2}.
Select: out[v] = value where cond(d2[v]) and (only < 0 or cls[v] == only), cls[v] elsewhere; cond = d2 > r2 (above) or d2 <= r2.
Ball of radius r >= 0: r2 = floor(r * r) in float64; dilation, erosion, opening and closing are thresholds of d2 at r2 (below)."""
import math

import numpy as np
from scipy import ndimage

INF = 2 ** 31 - 1
RANK = {6: 1, 18: 2, 26: 3}


def class_map(src):
    """(cls uint8 [Z, Y, X], has bool [Z, Y, X]: the voxel has a class)."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim in (3, 4)
    if src.ndim == 3:
        return src.copy(), np.ones(src.shape, dtype=bool)
    assert 2 <= src.shape[3] <= 16
    return np.argmax(src, axis=-1).astype(np.uint8), src.max(axis=-1) > 0        # numpy's argmax returns the first of equal maxima


def members(src, target):
    cls, has = class_map(src)
    return has & (cls == target)


def limits_ok(Z, Y, X):
    return min(Z, Y, X) >= 1 and Z * Y * X <= 2 ** 31 - 1 and (Z - 1) ** 2 + (Y - 1) ** 2 + (X - 1) ** 2 <= 2 ** 31 - 2


def radius_sq(radius):
    return int(math.floor(float(radius) * float(radius)))


def distance_sq_of(seeds):
    """d2 of a boolean seed map."""
    seeds = np.asarray(seeds, dtype=bool)
    assert limits_ok(*seeds.shape)
    if not seeds.any():
        return np.full(seeds.shape, INF, dtype=np.int32)
    return np.rint(ndimage.distance_transform_edt(~seeds) ** 2).astype(np.int32)


def distance_sq(src, target=1, invert=False):
    a = members(src, target)
    return distance_sq_of(~a if invert else a)


def distance_sq_mask(prev, r2, above):
    prev = np.asarray(prev)
    return distance_sq_of(prev > r2 if above else prev <= r2)


def select(d2, cls, r2, above, only, value):
    cond = (d2 > r2) if above else (d2 <= r2)
    if only >= 0:
        cond = cond & (cls == only)
    out = np.asarray(cls).copy()
    out[cond] = value
    return out


def dilate(src, target, radius):
    cls, _ = class_map(src)
    out = cls.copy()
    out[distance_sq(src, target, False) <= radius_sq(radius)] = target
    return out


def erode(src, target, radius, fill=0):
    """The outside of the volume does not erode (scipy's border_value=1)."""
    cls, _ = class_map(src)
    a = members(src, target)
    out = cls.copy()
    out[a & (distance_sq_of(~a) <= radius_sq(radius))] = fill
    return out


def opening(src, target, radius, fill=0):
    cls, _ = class_map(src)
    a, r2 = members(src, target), radius_sq(radius)
    e = a & (distance_sq_of(~a) > r2)
    o = distance_sq_of(e) <= r2
    assert not (o & ~a).any()                                  # O is a subset of A
    out = cls.copy()
    out[a & ~o] = fill
    return out


def closing(src, target, radius):
    cls, _ = class_map(src)
    a, r2 = members(src, target), radius_sq(radius)
    d = distance_sq_of(a) <= r2
    c = distance_sq_of(~d) > r2
    assert not (a & ~c).any()                                  # Cl is a superset of A
    out = cls.copy()
    out[c] = target
    return out


def fill_holes(src, target, connectivity=6):
    """The voxels outside A in components of the complement of A that touch none of the six faces take the target."""
    cls, _ = class_map(src)
    a = members(src, target)
    lab, k = ndimage.label(~a, structure=ndimage.generate_binary_structure(3, RANK[connectivity]))
    faces = np.concatenate([lab[0].ravel(), lab[-1].ravel(), lab[:, 0].ravel(), lab[:, -1].ravel(), lab[:, :, 0].ravel(), lab[:, :, -1].ravel()])
    open_ = np.zeros(k + 1, dtype=bool)
    open_[faces] = True
    open_[0] = True                                            # label 0 is A itself
    out = cls.copy()
    out[~open_[lab]] = target
    return out
