"""Grayscale morphological reconstruction of a resident volume and the h-maxima markers that split touching objects (not in the
reference; DESIGN.md section 28, defined by tests/reconstruct_ref.py).

  reconstruct(marker, mask, connectivity, method, h)   int32 [Z, Y, X]: by 'dilation' the largest map below mask that spreads from
                                                        min(sat(marker - h), mask) without passing mask; by 'erosion' the dual
  hmaxima(f, h) / hminima(f, h)                         f with every peak cut (every pit filled) by h
  regional_maxima(f) / regional_minima(f)               uint8 [Z, Y, X]: 1 on the plateaus with no higher (lower) neighbour
  extended_maxima(f, h) / extended_minima(f, h)         the regional maxima of hmaxima(f, h): the peaks that stand at least h above
                                                        the saddle that joins them to a higher one
  distance_landscape(src, target, scale)                int32 [Z, Y, X]: isqrt(scale^2 d2) on class `target`, d2 the squared distance to
                                                        its outside; OFF = -2^31 elsewhere
  hmax_markers(src, target, h, connectivity, scale)     (labels, count): the extended maxima of the landscape at h voxels, labelled
  split_touching(src, target, h, connectivity, metric, scale)
                                                        (labels, count): geodesic.split_touching with those markers as its seeds

marker, mask and f are int32 [Z, Y, X] maps of any values; h of the map functions is an integer >= 0 in the map's units, h of the
last two a number of voxels (h scale <= 2^31 - 2).  src is uint8 as in morphology.py.  connectivity 6, 18 or 26.  Resident maps (CUDA
tensors) go through libiunet (iunet_rec_init, iunet_rec_relax, iunet_rec_select, iunet_rec_landscape; for the markers and the split also
iunet_edt_sq, iunet_cc_label and geodesic.py's calls) and stay on the device; numpy arrays take the numpy path below, which yields the
same integers.  A missing library is an error."""
import math

import numpy as np
import torch

from . import components, geodesic, instances, morphology, resident
from .morphology import MAX_SQ

LOW, HIGH = -2 ** 31, 2 ** 31 - 1
OFF = LOW                                                             # the landscape off the class: nothing spreads through it
METHODS = ('dilation', 'erosion')
MAX_SCALE = 256
ROUNDS_PER_CALL = 8                                                   # rounds between two reads of the 4-byte `changed`
_RANK = {6: 1, 18: 2, 26: 3}


def _method(method):
    if method not in METHODS:
        raise ValueError(f'method {method!r}: one of {METHODS}')
    return method == 'erosion'


def _height(h):
    if not resident.is_int(h) or not 0 <= h <= HIGH:
        raise ValueError(f'h {h!r}: an int in 0 .. 2^31 - 1')
    return int(h)


def _scale(scale):
    if not resident.is_int(scale) or not 1 <= scale <= MAX_SCALE:
        raise ValueError(f'scale {scale!r}: an int in 1 .. {MAX_SCALE}')
    return int(scale)


def _height_voxels(h, scale):
    """h voxels in the landscape's units: floor(h scale + 0.5)."""
    if isinstance(h, bool) or not isinstance(h, (int, float, np.integer, np.floating)) or not math.isfinite(h) or h < 0 or h * scale > HIGH - 1:
        raise ValueError(f'h {h!r}: a finite number >= 0 with h scale <= 2^31 - 2')
    return int(math.floor(h * scale + 0.5))


def _check_pair(marker, mask):
    dev, Z, Y, X = resident.check_map(mask, 'mask')
    resident.check_map(marker, 'marker', (dev, Z, Y, X))
    if dev and marker.device != mask.device:
        raise ValueError(f'marker on {marker.device}, mask on {mask.device}')
    return dev, Z, Y, X


# ---- the device path ----
def _reconstruct_device(marker, mask, Z, Y, X, connectivity, erosion, h, max_rounds):
    """R of resident maps: iunet_rec_init, then rounds of iunet_rec_relax until no tile changes; the 4-byte count is read back once per
    call."""
    from . import _native as nv
    ws_bytes = nv.lib().iunet_rec_ws_bytes(Z, Y, X)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=mask.device)
    r = torch.empty_like(mask)
    changed = torch.empty(1, dtype=torch.int32, device=mask.device)
    with torch.cuda.device(mask.device):
        nv.call('iunet_rec_init', nv.ptr(marker), nv.ptr(mask), Z, Y, X, h, int(erosion), nv.ptr(r), nv.ptr(ws), ws_bytes, nv.stream())
        done = 0
        while done < max_rounds:
            rounds = min(ROUNDS_PER_CALL, max_rounds - done)
            nv.call('iunet_rec_relax', nv.ptr(r), nv.ptr(mask), Z, Y, X, connectivity, int(erosion), rounds, nv.ptr(changed), nv.ptr(ws), ws_bytes,
                    nv.stream())
            done += rounds
            if int(changed.item()) == 0:
                return r
    raise RuntimeError(f'reconstruction: still changing after {done} rounds (max_rounds)')


def _select_device(a, b, Z, Y, X, t=1, value=1):
    from . import _native as nv
    out = torch.empty((Z, Y, X), dtype=torch.uint8, device=a.device)
    with torch.cuda.device(a.device):
        nv.call('iunet_rec_select', nv.ptr(a), nv.ptr(b), Z, Y, X, t, value, nv.ptr(out), nv.stream())
    return out


# ---- the host path ----
def _host_reconstruct(marker, mask, connectivity, erosion, h, max_rounds):
    """The fixed point by whole-volume sweeps, one neighbour offset after the other, until a sweep changes nothing."""
    spread, bound = (np.minimum, np.maximum) if erosion else (np.maximum, np.minimum)
    shifted = np.clip(marker.astype(np.int64) + (h if erosion else -h), LOW, HIGH).astype(np.int32)
    r = bound(shifted, mask)
    views = []
    for off in [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]:
        if 0 < sum(d != 0 for d in off) <= _RANK[connectivity]:
            to = tuple(slice(max(0, -d), n - max(0, d)) for n, d in zip(r.shape, off))
            views.append((to, tuple(slice(s.start + d, s.stop + d) for s, d in zip(to, off))))
    for _ in range(max_rounds):
        before = r.copy()
        for to, frm in views:
            r[to] = bound(spread(r[to], r[frm]), mask[to])
        if np.array_equal(r, before):
            return r
    raise RuntimeError(f'reconstruction: still changing after {max_rounds} rounds (max_rounds)')


def _host_select(a, b, t=1, value=1):
    return np.where(a.astype(np.int64) - b.astype(np.int64) >= t, value, 0).astype(np.uint8)


def _host_landscape(d2, scale):
    p = d2.astype(np.int64) * (scale * scale)                         # < 2^47: exact as a double
    s = np.sqrt(p.astype(np.float64)).astype(np.int64)
    s -= s * s > p
    s += (s + 1) * (s + 1) <= p
    return np.where(d2 > 0, s, OFF).astype(np.int32)


# ---- the functions ----
def _run(marker, mask, connectivity, erosion, h, max_rounds, checked):
    dev, Z, Y, X = checked
    if dev:
        return _reconstruct_device(marker, mask, Z, Y, X, connectivity, erosion, h, max_rounds)
    return _host_reconstruct(marker, mask, connectivity, erosion, h, max_rounds)


def reconstruct(marker, mask, connectivity=6, method='dilation', h=0, max_rounds=None):
    """int32 [Z, Y, X]: the reconstruction of mask from marker shifted by h.  max_rounds: a RuntimeError when it has not come to rest after
    that many rounds (default Z Y X + 1, which no input reaches)."""
    checked = _check_pair(marker, mask)
    connectivity, erosion, h = instances._connectivity(connectivity), _method(method), _height(h)
    return _run(marker, mask, connectivity, erosion, h, geodesic._check_rounds(max_rounds, *checked[1:]), checked)


def _of_one(f, h, connectivity, max_rounds):
    checked = resident.check_map(f, 'f')
    connectivity, h = instances._connectivity(connectivity), _height(h)
    return checked, connectivity, h, geodesic._check_rounds(max_rounds, *checked[1:])


def hmaxima(f, h, connectivity=6, max_rounds=None):
    """f with every peak lowered by h and cut at the level it then floods to: R_f(f - h) by dilation."""
    checked, connectivity, h, max_rounds = _of_one(f, h, connectivity, max_rounds)
    return _run(f, f, connectivity, False, h, max_rounds, checked)


def hminima(f, h, connectivity=6, max_rounds=None):
    checked, connectivity, h, max_rounds = _of_one(f, h, connectivity, max_rounds)
    return _run(f, f, connectivity, True, h, max_rounds, checked)


def _regional(f, connectivity, max_rounds, erosion, checked):
    r = _run(f, f, connectivity, erosion, 1, max_rounds, checked)
    a, b = (r, f) if erosion else (f, r)
    return _select_device(a, b, *checked[1:]) if checked[0] else _host_select(a, b)


def regional_maxima(f, connectivity=6, max_rounds=None):
    """uint8 [Z, Y, X]: 1 where f - R_f(f - 1) >= 1 -- the plateaus without a higher neighbour; never a voxel of value -2^31."""
    checked, connectivity, _, max_rounds = _of_one(f, 0, connectivity, max_rounds)
    return _regional(f, connectivity, max_rounds, False, checked)


def regional_minima(f, connectivity=6, max_rounds=None):
    checked, connectivity, _, max_rounds = _of_one(f, 0, connectivity, max_rounds)
    return _regional(f, connectivity, max_rounds, True, checked)


def extended_maxima(f, h, connectivity=6, max_rounds=None):
    """uint8 [Z, Y, X]: the regional maxima of hmaxima(f, h)."""
    checked, connectivity, h, max_rounds = _of_one(f, h, connectivity, max_rounds)
    return _regional(_run(f, f, connectivity, False, h, max_rounds, checked), connectivity, max_rounds, False, checked)


def extended_minima(f, h, connectivity=6, max_rounds=None):
    checked, connectivity, h, max_rounds = _of_one(f, h, connectivity, max_rounds)
    return _regional(_run(f, f, connectivity, True, h, max_rounds, checked), connectivity, max_rounds, True, checked)


def _landscape(src, dev, Z, Y, X, C, target, scale):
    """(f, a): the landscape, and A as geodesic.split_from_seeds takes it."""
    if dev:
        from . import _native as nv
        f = morphology._edt(src, Z, Y, X, C, target, True, want_cls=False)[0]      # the distance to the outside of A: > 0 exactly on A
        a = (f > 0).to(torch.uint8)
        with torch.cuda.device(src.device):
            nv.call('iunet_rec_landscape', nv.ptr(f), Z, Y, X, scale, OFF, nv.ptr(f), nv.stream())
        return f, a
    cls, has = resident.host_maps(src)
    a = has & (cls == target)
    return _host_landscape(morphology._host_d2(~a), scale), a


def distance_landscape(src, target=1, scale=4):
    """int32 [Z, Y, X]: floor(scale x the distance to the outside of class `target`) on the class, OFF = -2^31 elsewhere."""
    dev, Z, Y, X, C = resident.check_volume(src, MAX_SQ)
    target, scale = resident.check_byte(target, 'target'), _scale(scale)
    return _landscape(src, dev, Z, Y, X, C, target, scale)[0]


def _markers(f, dev, Z, Y, X, connectivity, h_int, max_rounds):
    checked = (dev, Z, Y, X)
    e = _regional(_run(f, f, connectivity, False, h_int, max_rounds, checked), connectivity, max_rounds, False, checked)
    if dev:
        return instances._label(e, Z, Y, X, connectivity)
    return components.label(e, connectivity)[:2]


def hmax_markers(src, target, h, connectivity=6, scale=4):
    """(labels int32 [Z, Y, X], count): the extended maxima of the distance landscape at h voxels, each component under `connectivity`
    one marker, numbered in increasing order of their first voxels.  Every object of the class holds at least one.  CUDA src: count is
    read back as a Python int."""
    dev, Z, Y, X, C = resident.check_volume(src, MAX_SQ)
    target, scale, connectivity = resident.check_byte(target, 'target'), _scale(scale), instances._connectivity(connectivity)
    h_int, max_rounds = _height_voxels(h, scale), geodesic._check_rounds(None, Z, Y, X)
    return _markers(_landscape(src, dev, Z, Y, X, C, target, scale)[0], dev, Z, Y, X, connectivity, h_int, max_rounds)


def split_touching(src, target, h, connectivity=6, metric='chamfer', scale=4, max_rounds=None):
    """(labels int32 [Z, Y, X], count): 0 off class `target`.  geodesic.split_touching with hmax_markers as its seeds instead of the
    cores of an erosion: a peak of the distance map is a seed if it stands at least h voxels above the saddle that joins it to a higher
    peak, whatever its own height, so a small object keeps its seed beside a large one.  Numbered in increasing order of the instances'
    first voxels."""
    dev, Z, Y, X, C = resident.check_volume(src, MAX_SQ)
    target, scale, connectivity = resident.check_byte(target, 'target'), _scale(scale), instances._connectivity(connectivity)
    h_int = _height_voxels(h, scale)
    weights = geodesic.split_weights(metric, connectivity)
    geodesic._check_overflow(Z, Y, X, weights)
    max_rounds = geodesic._check_rounds(max_rounds, Z, Y, X)
    f, a = _landscape(src, dev, Z, Y, X, C, target, scale)
    lm, km = _markers(f, dev, Z, Y, X, connectivity, h_int, max_rounds)
    seeds = [lm]
    del f, lm
    return geodesic.split_from_seeds(a, seeds, km, connectivity, weights, max_rounds)
