"""Where to annotate next (not in the reference, whose Randomize button draws a blind uniform plane: app.py:301-315; DESIGN.md section
20, defined by tests/propose_ref.py): take the user to the plane where the current model is least sure and that is not annotated yet.

  uncertainty(pred, weight, image, brick)   the predicted volume's uncertainty bytes (top-two margin) and their brick sums
  candidate_origins(bricks, ...)            the centres of the most uncertain bricks
  score_planes(u, planes, slice_width)      the uncertainty summed over each candidate plane
  propose_slices(shape, pred, ...)          candidate origins x orientations, scored in one launch and ranked
  next_slice(slicer, pred, ...)             sets the slicer to the best proposal -- the call that replaces Slicer.randomize in the app

Resident volumes (CUDA uint8 tensors) go through libiunet (iunet_uncertainty_volume, iunet_plane_scores) and stay on the device;
numpy arrays take the vectorised numpy path below, which computes the same integers.  A missing library is an error."""
import numpy as np
import torch

from . import resident
from .slicer import Slicer

BRICKS = (4, 8, 16, 32)


def _volumes(pred, weight, image):
    """Validated (on_device, pred, weight, wch, image, ich); weight / image None where not given.  Raises ValueError before any GPU work."""
    vols = [v for v in (pred, weight, image) if v is not None]
    tens = [torch.is_tensor(v) for v in vols]
    if pred is None or (any(tens) and not all(tens)) or not all(t or isinstance(v, np.ndarray) for t, v in zip(tens, vols)):
        raise ValueError('pred, weight and image must all be CUDA tensors or all be numpy arrays')
    dev = tens[0]
    if dev and not all(v.is_cuda and v.device == pred.device for v in vols):
        raise ValueError('resident volumes must be CUDA tensors on one device (a host volume goes in as a numpy array)')
    for name, v in (('pred', pred), ('weight', weight), ('image', image)):
        if v is None:
            continue
        resident.check_bytes(name, v, dev)
    if pred.ndim != 4 or not 2 <= pred.shape[3] <= 16 or min(pred.shape) < 1:
        raise ValueError(f'pred must be [Z, Y, X, C] with 2 <= C <= 16, got {tuple(pred.shape)}')
    zyx = tuple(pred.shape[:3])

    def channels(name, v, allowed):
        if v is None:
            return 0
        ch = 1 if v.ndim == 3 else int(v.shape[-1])
        if v.ndim not in (3, 4) or tuple(v.shape[:3]) != zyx or ch not in allowed:
            raise ValueError(f'{name} must be [Z, Y, X] or [Z, Y, X, ch] over the volume {zyx}, ch in {tuple(allowed)}; got {tuple(v.shape)}')
        return ch
    return dev, pred, weight, channels('weight', weight, (1, 2)), image, channels('image', image, (1, 2, 3, 4))


def uncertainty(pred, weight=None, image=None, brick=8):
    """(u, bricks) of a predicted volume pred, uint8 [Z, Y, X, C]: u uint8 [Z, Y, X] = 255 - (largest byte - second largest byte), 0
    where the voxel was never predicted (all bytes 0), is annotated (a byte of weight, uint8 [Z, Y, X] / [Z, Y, X, 1 or 2], is > 0) or is
    dark (channel 0 of image, uint8 [Z, Y, X] / [Z, Y, X, 1 .. 4], is 0); bricks [ceil(dim / brick)] * 3 = the sum of u over each brick's
    voxels inside the volume.  CUDA tensors: one kernel, the results stay on the device (bricks as int32: a sum is below 2^24); numpy
    arrays: numpy, bricks as uint32."""
    dev, pred, weight, wch, image, ich = _volumes(pred, weight, image)
    if brick not in BRICKS:
        raise ValueError(f'brick size {brick}: one of {BRICKS}')
    Z, Y, X, C = (int(n) for n in pred.shape)
    if Z * Y * X >= 1 << 42:
        raise ValueError(f'volume {Z} x {Y} x {X}: 2^42 voxels or more')
    nb = [-(-n // brick) for n in (Z, Y, X)]
    if dev:
        from . import _native as nv
        u = torch.empty((Z, Y, X), dtype=torch.uint8, device=pred.device)
        bricks = torch.empty(nb, dtype=torch.int32, device=pred.device)
        with torch.cuda.device(pred.device):
            nv.call('iunet_uncertainty_volume', nv.ptr(pred), Z, Y, X, C, nv.ptr(weight), wch, nv.ptr(image), ich, int(brick), nv.ptr(u),
                    nv.ptr(bricks), nv.stream())
        return u, bricks
    top = np.partition(pred, C - 2, axis=-1)[..., C - 2:].astype(np.int16)               # (second largest, largest)
    u = np.where(top[..., 1] > 0, 255 - (top[..., 1] - top[..., 0]), 0)
    if weight is not None:
        u[weight.reshape(Z, Y, X, wch).max(axis=-1) > 0] = 0
    if image is not None:
        u[image.reshape(Z, Y, X, ich)[..., 0] == 0] = 0
    u = u.astype(np.uint8)
    padded = np.zeros([n * brick for n in nb], dtype=np.uint32)
    padded[:Z, :Y, :X] = u
    bricks = padded.reshape(nb[0], brick, nb[1], brick, nb[2], brick).sum(axis=(1, 3, 5), dtype=np.uint32)
    return u, bricks


def score_planes(u, planes, slice_width=256):
    """int64 [P, 2] = (score, inside) of each plane of `planes`, float64 [P, 3, 3] of (a, b, origin): the sum of u, uint8 [Z, Y, X], over
    the plane's slice_width^2 samples origin + a r_i + b r_j that lie inside the volume (sampled at order 0, as the slicer samples them),
    and their number.  A CUDA u: one iunet_plane_scores launch for all planes, the result stays on the device."""
    dev = torch.is_tensor(u)
    if not (dev or isinstance(u, np.ndarray)) or u.dtype != (torch.uint8 if dev else np.uint8) or u.ndim != 3 or min(u.shape) < 1:
        raise ValueError('u must be a uint8 [Z, Y, X] CUDA tensor or numpy array')
    if dev and not (u.is_cuda and u.is_contiguous()):
        raise ValueError('a resident u must be a contiguous CUDA tensor (a host volume goes in as a numpy array)')
    planes = np.ascontiguousarray(planes, dtype=np.float64)
    if planes.ndim != 3 or planes.shape[1:] != (3, 3) or not 1 <= planes.shape[0] <= 65535 or not np.isfinite(planes).all():
        raise ValueError(f'planes must be a finite float64 [P, 3, 3] array of (a, b, origin), 1 <= P <= 65535; got {planes.shape}')
    sw = int(slice_width)
    if not 1 <= sw <= 4096:
        raise ValueError(f'slice width {sw} outside 1..4096')
    P, start = planes.shape[0], int(-np.floor(sw / 2))
    if dev:
        from . import _native as nv
        geoms = torch.from_numpy(planes).to(u.device)
        ws_bytes = nv.answer(nv.lib().iunet_plane_scores_ws_bytes(P, sw))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=u.device)
        out = torch.empty((P, 2), dtype=torch.int64, device=u.device)
        with torch.cuda.device(u.device):
            nv.call('iunet_plane_scores', nv.ptr(u), int(u.shape[0]), int(u.shape[1]), int(u.shape[2]), nv.ptr(geoms), P, sw, start,
                    nv.ptr(ws), ws_bytes, nv.ptr(out), nv.stream())
        return out
    r = (start + np.arange(sw)).astype(np.float64)
    hi = np.array(u.shape, dtype=np.float64) - 1.0
    out = np.zeros((P, 2), dtype=np.int64)
    for p, (a, b, o) in enumerate(planes):
        c = (a[:, None, None] * r[None, :, None] + b[:, None, None] * r[None, None, :]) + o[:, None, None]
        inside = ((c >= 0.0) & (c <= hi[:, None, None])).all(axis=0)
        z, y, x = np.floor(c[:, inside] + 0.5).astype(np.int64)
        out[p] = u[z, y, x].sum(dtype=np.int64), inside.sum()
    return out


def candidate_origins(bricks, brick, shape, count):
    """float64 [n <= count, 3]: the `count` bricks of largest sum, in the order (sum descending, flat index ascending), bricks of sum 0
    dropped; each as the centre of the brick's part inside the volume `shape`."""
    if torch.is_tensor(bricks):
        vals, idx = torch.sort(bricks.reshape(-1).to(torch.int64), descending=True, stable=True)
        vals, idx = vals[:count].cpu().numpy(), idx[:count].cpu().numpy()
    else:
        flat = np.asarray(bricks).reshape(-1).astype(np.int64)
        idx = np.argsort(-flat, kind='stable')[:count]
        vals = flat[idx]
    b = np.stack(np.unravel_index(idx[vals > 0], tuple(bricks.shape)), axis=-1).astype(np.int64).reshape(-1, 3)
    dim = np.asarray(shape, dtype=np.int64)[:3]
    lo = b * brick
    return lo + (np.minimum(lo + brick, dim) - lo - 1) / 2


def _rotation_vectors(sampling_mode, sampling_axis, orientations, generator):
    """[(rotation vector, the sampling_axis Slicer.randomize would set -- None: it leaves it alone)] of one candidate."""
    if sampling_mode == 'grid':
        names = 'xyz' if sampling_axis == 'random' else sampling_axis
        if names not in ('xyz', 'x', 'y', 'z'):
            raise ValueError('sampling_axis must be "random", "x", "y" or "z".')
        return [(np.eye(3)['xyz'.index(n)].astype(int), n) for n in names]
    if sampling_mode != 'random':
        raise ValueError('sampling_mode must be either "random" or "grid".')
    out = []
    while len(out) < orientations:
        v = torch.randn(3, dtype=torch.float64, generator=generator).numpy()
        if np.linalg.norm(v) >= 0.0001:                                                  # slicer.py: _generate_uniformly_random_unit_vector
            out.append((v / np.linalg.norm(v), None))
    return out


def propose_slices(shape, pred, weight=None, image=None, slice_width=256, axis=0, brick=8, candidates=32, orientations=8,
                   sampling_mode='random', sampling_axis='random', generator=None):
    """The planes worth annotating next, best first: a list of dicts (rot_vec, origin, score, inside, sampling_axis).  The `candidates`
    most uncertain bricks of pred (see uncertainty) give the origins; each gets `orientations` random rotation vectors drawn from the
    torch `generator` ('random'), or the axis vectors ('grid': all three, or the one sampling_axis names).  Every plane is built by a
    scratch Slicer(shape) -- update_orientation_vectors(rot_vec), then the plane vectors of `axis` -- so it is bit for bit the plane a
    slicer holds after update_orientation_vectors(rot_vec) with that origin.  score = the uncertainty summed over the plane's samples
    inside the volume, inside = their number; ranked by (score descending, plane index ascending).  The raw sum is the key on purpose: a
    mean over `inside` would favour slivers at the volume's faces.  No brick of positive sum: []."""
    if tuple(int(n) for n in shape)[:3] != tuple(pred.shape[:3]):
        raise ValueError(f'shape {tuple(shape)} is not the predicted volume\'s {tuple(pred.shape[:3])}')
    if axis not in (0, 1, 2) or candidates < 1 or orientations < 1:
        raise ValueError('axis must be 0, 1 or 2; candidates and orientations at least 1')
    _rotation_vectors(sampling_mode, sampling_axis, 0, None)                             # refuse a bad mode before any GPU work
    u, bricks = uncertainty(pred, weight, image, brick)
    origins = candidate_origins(bricks, brick, shape, candidates)
    scratch = Slicer([int(n) for n in shape])
    planes, found = [], []
    for origin in origins:
        for vec, name in _rotation_vectors(sampling_mode, sampling_axis, orientations, generator):
            scratch.update_orientation_vectors(vec)
            a, b = scratch._plane_vectors(axis)
            planes.append((a, b, origin))
            found.append({'rot_vec': vec, 'origin': origin.copy(), 'sampling_axis': name})
    if not found:
        return []
    scores = score_planes(u, np.array(planes, dtype=np.float64), slice_width)
    scores = scores.cpu().numpy() if torch.is_tensor(scores) else scores
    for f, (score, inside) in zip(found, scores):
        f['score'], f['inside'] = int(score), int(inside)
    return [found[p] for p in sorted(range(len(found)), key=lambda p: (-found[p]['score'], p))]


def next_slice(slicer, pred, **kw):
    """Set `slicer` to the best proposal of propose_slices(slicer.volume_shape, pred, **kw) -- orientation, origin, and sampling_axis
    as Slicer.randomize sets it -- and return the proposals.  Where nothing uncertain is left (no brick of positive sum) it falls back to
    slicer.randomize(sampling_mode, sampling_axis) and returns []."""
    found = propose_slices(slicer.volume_shape, pred, **kw)
    if not found:
        slicer.randomize(sampling_mode=kw.get('sampling_mode', 'random'), sampling_axis=kw.get('sampling_axis', 'random'))
        return []
    best = found[0]
    if best['sampling_axis'] is not None:
        slicer.sampling_axis = best['sampling_axis']
    slicer.update_orientation_vectors(best['rot_vec'])
    slicer.origin = best['origin'].copy()
    return found
