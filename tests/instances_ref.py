"""The definition of the nearest-seed feature transform and of the instance labels built on it: what
iunet_edt_feature, iunet_edt_feature_mask, iunet_edt_assign and iunet_label_remap compute, and what interactive_unet/instances.py builds on
them, restated with numpy and scipy.ndimage.label.  Nothing here imports the package.

Input src, the class rule, the member set A of a target, invert, INF = 2^31 - 1 and the two size limits are those of
tests/morphology_ref.py.  The raster index of v = (z, y, x) is (z Y + y) X + x, int32 (Z Y X <= 2^31 - 1).
Feature transform of a seed set S: d2[v] = min over s in S of |v - s|^2 (INF everywhere when S is empty); idx[v] = the raster index of the
seed nearest to v -- of the seeds at the minimum distance the one with the smallest raster index; v's own index on S; -1 everywhere when S
is empty.  It is written here as three passes, X then Y then Z, each a minimum and a FIRST argmin of f(i) + (u - i)^2 along its axis: the Z
pass takes the smallest z' of the minimising planes, inside it the Y pass the smallest y', inside that row the X pass the left seed --
raster order is z-major, so that is the smallest raster index (tests/test_instances_cpu.py compares with a brute-force minimum over all
seeds in raster order).
Seeds from an int32 map prev: S = {prev > r2} (above) or {prev <= r2}.
Assign, remap, split_touching and expand_labels: at the functions below."""
import math

import numpy as np
from scipy import ndimage

INF = 2 ** 31 - 1
MAX_SQ = 2 ** 31 - 2
RANK = {6: 1, 18: 2, 26: 3}
_BIG = np.int64(1) << 40                                             # "no seed": above every finite f + (u - i)^2


def class_map(src):
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim in (3, 4)
    if src.ndim == 3:
        return src.copy(), np.ones(src.shape, dtype=bool)
    assert 2 <= src.shape[3] <= 16
    return np.argmax(src, axis=-1).astype(np.uint8), src.max(axis=-1) > 0


def members(src, target):
    cls, has = class_map(src)
    return has & (cls == target)


def limits_ok(Z, Y, X):
    return min(Z, Y, X) >= 1 and Z * Y * X <= 2 ** 31 - 1 and (Z - 1) ** 2 + (Y - 1) ** 2 + (X - 1) ** 2 <= 2 ** 31 - 2


def radius_sq(radius):
    return int(math.floor(float(radius) * float(radius)))


def _axis_pass(f, at, axis):
    """One pass along `axis`: (min over i of f(i) + (u - i)^2, at[the first i that attains it]) for every u, by broadcasting."""
    f, at = np.moveaxis(f, axis, -1), np.moveaxis(at, axis, -1)
    shape, n = f.shape, f.shape[-1]
    f, at = f.reshape(-1, n), at.reshape(-1, n)
    g, to = np.empty_like(f), np.empty_like(at)
    pos = np.arange(n, dtype=np.int64)
    sq = (pos[:, None] - pos[None, :]) ** 2                          # [u, i]
    rows = max(1, (1 << 22) // (n * n))                              # lines of the axis per step: the [rows, u, i] table stays small
    for lo in range(0, f.shape[0], rows):
        cost = f[lo:lo + rows, None, :] + sq[None]                   # [line, u, i]
        first = cost.argmin(axis=2)                                  # numpy's argmin returns the first of equal minima
        g[lo:lo + rows] = np.take_along_axis(cost, first[..., None], axis=2)[..., 0]
        to[lo:lo + rows] = np.take_along_axis(at[lo:lo + rows], first, axis=1)
    return np.moveaxis(g.reshape(shape), -1, axis), np.moveaxis(to.reshape(shape), -1, axis)


def feature_of(seeds):
    """(d2 int32, idx int32) of a boolean seed map."""
    seeds = np.asarray(seeds, dtype=bool)
    assert seeds.ndim == 3 and limits_ok(*seeds.shape)
    f = np.where(seeds, np.int64(0), _BIG)
    at = np.arange(seeds.size, dtype=np.int64).reshape(seeds.shape)  # on S, v's own index
    for axis in (2, 1, 0):
        f, at = _axis_pass(f, at, axis)
    none = f >= _BIG
    # C order: the passes leave their axis last in memory, and numpy keeps that layout
    return np.ascontiguousarray(np.where(none, INF, f), dtype=np.int32), np.ascontiguousarray(np.where(none, -1, at), dtype=np.int32)


def feature(src, target=1, invert=False):
    a = members(src, target)
    return feature_of(~a if invert else a)


def feature_mask(prev, r2, above):
    prev = np.asarray(prev)
    return feature_of(prev > r2 if above else prev <= r2)


def assign(idx, d2, seed_labels, r2, group=None, offset=0):
    """Without group: out[v] = seed_labels[idx[v]] where idx[v] >= 0 and d2[v] <= r2, 0 elsewhere.  With group: 0 where group[v] == 0;
    seed_labels[idx[v]] where idx[v] >= 0, d2[v] <= r2 and group[idx[v]] == group[v]; offset + group[v] otherwise."""
    idx, d2, flat = np.asarray(idx), np.asarray(d2), np.asarray(seed_labels).reshape(-1)
    reached = (idx >= 0) & (d2 <= r2)
    to = np.where(idx >= 0, idx, 0)
    if group is None:
        return np.where(reached, flat[to], 0).astype(np.int32)
    group = np.asarray(group)
    own = reached & (group.reshape(-1)[to] == group)
    return np.where(group == 0, 0, np.where(own, flat[to], offset + group)).astype(np.int32)


def remap(labels, table):
    """labels[v] <- table[labels[v]]; a label outside 0 .. K = len(table) - 1 is left as it is."""
    labels, table = np.asarray(labels), np.asarray(table)
    inside = (labels >= 0) & (labels < len(table))
    return np.where(inside, table[np.where(inside, labels, 0)], labels).astype(np.int32)


def renumber(raw):
    """The labels that occur in raw (0 is none), renumbered 1 .. K in increasing order of their first voxel."""
    flat = np.asarray(raw).reshape(-1)
    at = np.flatnonzero(flat)
    found, where = np.unique(flat[at], return_index=True)            # first occurrence = the smallest raster index
    order = np.argsort(at[where], kind='stable')
    out = np.zeros(flat.shape, np.int32)
    for k, label in enumerate(found[order]):
        out[flat == label] = k + 1
    return out.reshape(np.shape(raw)), len(found)


def components_of(mask, connectivity):
    """(labels int32, count) of a boolean map: numbered in increasing order of the components' first voxels (section 22's rule)."""
    lab, _ = ndimage.label(mask, structure=ndimage.generate_binary_structure(3, RANK[connectivity]))
    return renumber(lab)


def split_touching(src, target, radius, connectivity=6, parts=False):
    """(labels int32 [Z, Y, X], K): every voxel of an object (a component of A) takes the nearest core of its own object, the cores being
    the components of the erosion E = {d2(v, outside A) > r2}; an object without a core, and the voxels of an object whose nearest core
    lies in another object, form one instance per object.  parts: also (KE, KA)."""
    a, r2 = members(src, target), radius_sq(radius)
    d_out, _ = feature_of(~a)                                        # the outside of the volume does not erode
    e = d_out > r2
    assert not (e & ~a).any()
    le, ke = components_of(e, connectivity)
    la, ka = components_of(a, connectivity)
    d2e, idx = feature_of(e)
    raw = assign(idx, d2e, le, MAX_SQ, group=la, offset=ke)
    labels, k = renumber(raw)
    return (labels, k, ke, ka) if parts else (labels, k)


def expand_labels(labels, distance):
    """Every voxel within `distance` of a labelled voxel takes the label of the nearest one (the tie rule above), the others 0."""
    labels = np.asarray(labels)
    d2, idx = feature_of(labels > 0)
    return assign(idx, d2, labels, radius_sq(distance))
