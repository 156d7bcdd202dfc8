"""The definition of grayscale reconstruction and of the h-maxima markers built on it: what iunet_rec_init,
iunet_rec_relax, iunet_rec_landscape and iunet_rec_select compute, and what interactive_unet/reconstruction.py builds on them, restated
with numpy.  Nothing here imports the package.

mask, marker: int32 [Z, Y, X], any values; h >= 0 an integer; connectivity 6, 18 or 26: the neighbours of rank <= 1, 2 or 3 (RANK).
By dilation: r0[v] = min(sat(marker[v] - h), mask[v]), sat clamping the 64-bit difference to int32; R is the fixed point of
    r[v] = min(mask[v], max(r[v], max over the neighbours u inside the volume of r[u]))
started at r0 -- written here as whole-volume sweeps over shifted arrays, one neighbour offset after the other on the state as it stands
(any order of updates reaches the same fixed point), until a sweep changes nothing.  By erosion: the dual, min and max exchanged and
sat(marker + h).
    hmaxima(f, h) = R_f(f, h);  regional_maxima(f) = {f - R_f(f, 1) >= 1}, the difference in 64 bits, a uint8 map;
    extended_maxima(f, h) = regional_maxima(hmaxima(f, h));  hminima, regional_minima, extended_minima: the duals.
Distance landscape of a class: A the member set (tests/instances_ref.py's rule), d2 the squared distance to the outside of A (>= 1 on A,
0 off it; INF = 2^31 - 1 where the volume has no outside), f = isqrt(scale^2 d2) on A and OFF = -2^31 elsewhere, 1 <= scale <= 256.
Markers: the extended maxima of f at h_int = floor(h scale + 0.5), labelled in first-voxel order; the split: the markers grown through A
by tests/geodesic_ref.py's growth and renumbered."""
import math

import numpy as np

from tests.instances_ref import RANK, components_of, feature_of, members, renumber  # noqa: F401 (the shared rules)

LOW, HIGH = -2 ** 31, 2 ** 31 - 1
OFF = LOW


def offsets(connectivity):
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if 0 < abs(dz) + abs(dy) + abs(dx) <= RANK[connectivity]]


def sat(v):
    return np.clip(v, LOW, HIGH).astype(np.int32)


def first_state(marker, mask, h=0, erosion=False):
    """r0, int32."""
    marker, mask = np.asarray(marker), np.asarray(mask)
    assert marker.dtype == np.int32 and mask.dtype == np.int32 and marker.shape == mask.shape and mask.ndim == 3 and 0 <= h <= HIGH
    if erosion:
        return np.maximum(sat(marker.astype(np.int64) + h), mask)
    return np.minimum(sat(marker.astype(np.int64) - h), mask)


def _views(shape, off):
    """(to, from): the slices of the voxels that have a neighbour at `off` inside the volume, and of those neighbours."""
    to = tuple(slice(max(0, -d), n - max(0, d)) for n, d in zip(shape, off))
    return to, tuple(slice(s.start + d, s.stop + d) for s, d in zip(to, off))


def relax(r, mask, connectivity=6, erosion=False):
    """(R, sweeps): r swept to rest under mask; sweeps counts the sweeps that changed something."""
    r = np.array(r, dtype=np.int32)
    spread, bound = (np.minimum, np.maximum) if erosion else (np.maximum, np.minimum)
    views = [_views(r.shape, off) for off in offsets(connectivity)]
    sweeps = 0
    while True:
        before = r.copy()
        for to, frm in views:
            r[to] = bound(spread(r[to], r[frm]), mask[to])
        if np.array_equal(r, before):
            return r, sweeps
        sweeps += 1


def reconstruct(marker, mask, connectivity=6, erosion=False, h=0):
    return relax(first_state(marker, mask, h, erosion), mask, connectivity, erosion)[0]


def select(a, b, t, value=1):
    return np.where(np.asarray(a, dtype=np.int64) - np.asarray(b, dtype=np.int64) >= t, value, 0).astype(np.uint8)


def hmaxima(f, h, connectivity=6):
    return reconstruct(f, f, connectivity, False, h)


def hminima(f, h, connectivity=6):
    return reconstruct(f, f, connectivity, True, h)


def regional_maxima(f, connectivity=6):
    return select(f, reconstruct(f, f, connectivity, False, 1), 1)


def regional_minima(f, connectivity=6):
    return select(reconstruct(f, f, connectivity, True, 1), f, 1)


def extended_maxima(f, h, connectivity=6):
    return regional_maxima(hmaxima(f, h, connectivity), connectivity)


def extended_minima(f, h, connectivity=6):
    return regional_minima(hminima(f, h, connectivity), connectivity)


def landscape_of(d2, scale=4, off=OFF):
    """f int32 of a squared-distance map: isqrt(scale^2 d2) where d2 > 0, off elsewhere."""
    d2 = np.asarray(d2)
    assert 1 <= scale <= 256
    values, at = np.unique(d2, return_inverse=True)            # math.isqrt once per value that occurs
    heights = np.array([math.isqrt(scale * scale * int(d)) if d > 0 else off for d in values.tolist()], dtype=np.int32)
    return heights[at.reshape(-1)].reshape(d2.shape)


def distance_landscape(src, target=1, scale=4):
    a = members(src, target)
    return landscape_of(feature_of(~a)[0], scale)              # the outside of the volume does not count: INF where A is everything


def h_int(h, scale):
    return int(math.floor(h * scale + 0.5))


def hmax_markers(src, target, h, connectivity=6, scale=4):
    """(labels int32, count): the components of the extended maxima of the landscape, numbered in first-voxel order."""
    f = distance_landscape(src, target, scale)
    return components_of(extended_maxima(f, h_int(h, scale), connectivity) > 0, connectivity)


def split_touching(src, target, h, connectivity=6, metric='chamfer', scale=4, parts=False):
    """(labels int32, K): the markers grown through A along paths inside it (section 27), the voxels of A no marker reaches one instance
    per object, renumbered by first voxel.  parts: also (markers, objects)."""
    from tests import geodesic_ref as gr
    a = members(src, target)
    lm, km = hmax_markers(src, target, h, connectivity, scale)
    la, ka = components_of(a, connectivity)
    labels, k = renumber(gr.finish(gr.grow_keys(a, lm, gr.split_weights(metric, connectivity))[0], fallback=la, offset=km)[0])
    return (labels, k, km, ka) if parts else (labels, k)
