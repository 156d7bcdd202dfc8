"""The definition of the oblique slab: what iunet_slab_gather and iunet_slab_paste compute, restated in
numpy float64 with the operation order the kernels keep.  Nothing here imports the package: geometry goes in as four float64
vectors (a, b, n, origin) -- slicer_geometry() reads them off a Slicer.

Gather: sample (k, i, j) lies at c = ((a r_i + b r_j) + n r_k) + origin, r_i = start + i, r_j = start + j, r_k = start_k + k, every
product and sum rounded on its own (numpy evaluates one ufunc at a time: no fused multiply-add); the slab is
scipy.ndimage.map_coordinates(volume, c, order, mode='constant', cval=0) on the WHOLE volume.
Paste: voxel p of the box [lo, lo + len) has d = p - origin, t_v = (d_0 v_0 + d_1 v_1) + d_2 v_2 for v in (n, a, b), k = rint(t_n) -
start_k, i = rint(t_a) - start, j = rint(t_b) - start (np.rint: ties to even); it becomes quantize(probs[k, i, j]) iff k_lo <= k < k_hi
and border <= i, j < sw - border, and keeps its value otherwise."""
import numpy as np
from scipy import ndimage


def default_start(n):
    return int(-np.floor(n / 2))


def slicer_geometry(slicer, axis):
    """(a, b, n, origin): the plane vectors of `axis` (slicer.py: get_interpolation_coords) and the remaining one of (u, v, w)."""
    u, v, w = (np.asarray(t, dtype=np.float64) for t in (slicer.u, slicer.v, slicer.w))
    a, b = ((v, w), (u, w), (u, v))[axis]
    return a, b, (u, v, w)[axis], np.asarray(slicer.origin, dtype=np.float64)


def coords(geom, T, sw, start=None, start_k=None):
    """float64 [3, T, sw, sw]."""
    a, b, n, o = (np.asarray(t, dtype=np.float64) for t in geom)
    start = default_start(sw) if start is None else start
    start_k = default_start(T) if start_k is None else start_k
    ri = (start + np.arange(sw)).astype(np.float64)[None, None, :, None]
    rj = (start + np.arange(sw)).astype(np.float64)[None, None, None, :]
    rk = (start_k + np.arange(T)).astype(np.float64)[None, :, None, None]
    col = lambda t: t[:, None, None, None]
    t1 = col(a) * ri
    t2 = col(b) * rj
    t3 = col(n) * rk
    s = t1 + t2
    q = s + t3
    return q + col(o)


def gather(volume, geom, T, sw, order, start=None, start_k=None):
    """uint8 [T, sw, sw]."""
    return ndimage.map_coordinates(np.asarray(volume), coords(geom, T, sw, start, start_k), order=order, mode='constant', cval=0)


def quantize(probs):
    """The bytes of iunet_normalize_quantize at weight 1: uint8(255 * p / 1), fp32 product, truncating cast."""
    return (np.float32(255.0) * np.asarray(probs, dtype=np.float32)).astype(np.int32).astype(np.uint8)


def paste_indices(shape, geom, lo, length, T, sw, k_lo, k_hi, border, start=None, start_k=None):
    """(keep bool [len], k, i, j int64 [len]): which voxels of the box are written, and from which sample."""
    a, b, n, o = (np.asarray(t, dtype=np.float64) for t in geom)
    start = default_start(sw) if start is None else start
    start_k = default_start(T) if start_k is None else start_k
    p = [np.arange(lo[x], lo[x] + length[x]).astype(np.float64) for x in range(3)]
    d0 = (p[0] - o[0])[:, None, None]
    d1 = (p[1] - o[1])[None, :, None]
    d2 = (p[2] - o[2])[None, None, :]

    def nearest(v):
        s = d0 * v[0] + d1 * v[1]
        return np.rint(s + d2 * v[2])
    k, i, j = nearest(n) - start_k, nearest(a) - start, nearest(b) - start
    keep = (k >= k_lo) & (k < k_hi) & (i >= border) & (i < sw - border) & (j >= border) & (j < sw - border)
    return keep, k.astype(np.int64), i.astype(np.int64), j.astype(np.int64)


def paste(dest, probs, geom, k_lo=0, k_hi=None, border=0, lo=None, length=None, start=None, start_k=None):
    """A copy of dest (uint8 [Z, Y, X, C]) with the kept region of probs (fp32 [T, sw, sw, C]) pasted; lo / length: the box visited
    (default: the whole volume)."""
    out = np.array(dest, copy=True)
    T, sw = probs.shape[0], probs.shape[1]
    lo = (0, 0, 0) if lo is None else tuple(int(v) for v in lo)
    length = out.shape[:3] if length is None else tuple(int(v) for v in length)
    k_hi = T if k_hi is None else k_hi
    keep, k, i, j = paste_indices(out.shape, geom, lo, length, T, sw, k_lo, k_hi, border, start, start_k)
    box = out[lo[0]:lo[0] + length[0], lo[1]:lo[1] + length[1], lo[2]:lo[2] + length[2]]
    box[keep] = quantize(probs)[k[keep], i[keep], j[keep]]
    return out
