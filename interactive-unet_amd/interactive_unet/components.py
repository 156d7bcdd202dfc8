"""Connected components of a predicted volume (not in the reference; DESIGN.md section 22, defined by tests/components_ref.py): how
many objects there are, how big each one is, the specks removed, only the largest kept.

  label(src, connectivity, background)         (labels, count, cls): components numbered 1 .. count in order of their first voxel
  table(labels, cls, count)                    (sizes, classes, first) of the labels 0 .. count
  remove_small(src, min_size, ...)             the class map with the components below min_size voxels set to `fill`
  keep_largest(src, n, per_class, ...)         the class map with all but the n largest components (of each class) set to `fill`

src is uint8: a class map [Z, Y, X], or a predicted volume [Z, Y, X, C], 2 <= C <= 16, whose voxels take the class of their largest byte
(the lowest index on a tie; a voxel whose bytes are all 0 was never predicted and belongs to no component).  Resident volumes (CUDA
uint8 tensors) go through libiunet (iunet_cc_label, iunet_cc_table, iunet_cc_filter) and stay on the device; numpy arrays take the scipy
/ numpy path below, which yields the same integers.  A missing library is an error."""
import numpy as np
import torch

from . import resident

TILE = (4, 16, 64)                # (tz, ty, tx) of csrc/components.hip: CC_TZ, CC_TY, CC_TX (tests/test_components_cpu.py compares them)
CONNECTIVITIES = (6, 18, 26)


def _check(src, connectivity, background):
    """Validated (on_device, Z, Y, X, C, background as -1 .. 255).  Raises ValueError before any GPU work."""
    dev, Z, Y, X, C = resident.check_volume(src)
    if connectivity not in CONNECTIVITIES:
        raise ValueError(f'connectivity {connectivity}: one of {CONNECTIVITIES}')
    background = -1 if background is None else background
    if not resident.is_int(background) or not -1 <= background <= 255:
        raise ValueError(f'background {background!r}: None / -1 (every class is labelled) or 0 .. 255')
    return dev, Z, Y, X, C, int(background)


def _fill(fill, background):
    return resident.check_byte((0 if background in (None, -1) else background) if fill is None else fill, 'fill')


def _pair(labels, cls):
    """Validated (on_device, Z, Y, X) of a (labels, cls) pair."""
    dev = torch.is_tensor(labels)
    if dev != torch.is_tensor(cls) or not (dev or (isinstance(labels, np.ndarray) and isinstance(cls, np.ndarray))):
        raise ValueError('labels and cls must both be CUDA tensors or both be numpy arrays')
    if dev and not (labels.is_cuda and cls.is_cuda and labels.device == cls.device):
        raise ValueError('resident labels and cls must be CUDA tensors on one device')
    if labels.dtype != (torch.int32 if dev else np.int32) or cls.dtype != (torch.uint8 if dev else np.uint8):
        raise ValueError(f'labels must be int32 and cls uint8, got {labels.dtype} and {cls.dtype}')
    if labels.ndim != 3 or tuple(labels.shape) != tuple(cls.shape) or min(labels.shape) < 1:
        raise ValueError(f'labels and cls must be [Z, Y, X] over one volume, got {tuple(labels.shape)} and {tuple(cls.shape)}')
    if not ((labels.is_contiguous() and cls.is_contiguous()) if dev else (labels.flags['C_CONTIGUOUS'] and cls.flags['C_CONTIGUOUS'])):
        raise ValueError('labels and cls must be contiguous')
    Z, Y, X = (int(n) for n in labels.shape)
    if Z * Y * X > resident.MAX_VOXELS:
        raise ValueError(f'volume {Z} x {Y} x {X}: more than 2^31 - 1 voxels')
    return dev, Z, Y, X


def _count(count):
    return resident.check_count(count, 'count', 'the number of components, an int >= 0')


def label(src, connectivity=6, background=0):
    """(labels, count, cls): labels int32 [Z, Y, X], 0 for a voxel of no component (class `background`; never predicted), else the
    number 1 .. count of its component -- voxels of one class connected under the 6-, 18- or 26-neighbourhood -- in increasing order
    of the components' first voxels in raster order; cls uint8 [Z, Y, X], the class map that was labelled.  background None or -1:
    every class is labelled.  CUDA src: labels and cls stay on the device; count is read back as a Python int (4 bytes: the call's only
    synchronisation)."""
    dev, Z, Y, X, C, bg = _check(src, connectivity, background)
    if dev:
        from . import _native as nv
        labels = torch.empty((Z, Y, X), dtype=torch.int32, device=src.device)
        cls = torch.empty((Z, Y, X), dtype=torch.uint8, device=src.device)
        count = torch.empty(1, dtype=torch.int32, device=src.device)
        ws_bytes = nv.lib().iunet_cc_ws_bytes(Z, Y, X)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=src.device)
        with torch.cuda.device(src.device):
            nv.call('iunet_cc_label', nv.ptr(src), Z, Y, X, C, int(connectivity), bg, nv.ptr(labels), nv.ptr(cls), nv.ptr(count), nv.ptr(ws),
                    ws_bytes, nv.stream())
        return labels, int(count.item()), cls
    from scipy import ndimage
    cls, has = resident.host_maps(src)
    fg = has & (cls != bg)
    structure = ndimage.generate_binary_structure(3, CONNECTIVITIES.index(connectivity) + 1)
    # per class: scipy's labels and the raster index of each one's first voxel; then all components in order of first voxel
    firsts, flat = [], np.zeros(Z * Y * X, dtype=np.int64)
    for c in np.unique(cls[fg]):
        lab, _ = ndimage.label(fg & (cls == c), structure=structure)
        lab = lab.reshape(-1)
        at = np.flatnonzero(lab)
        _, where = np.unique(lab[at], return_index=True)                                 # first occurrence = smallest raster index
        flat[at] = lab[at] + len(firsts)
        firsts.extend(at[where].tolist())
    order = np.argsort(np.asarray(firsts, dtype=np.int64), kind='stable')
    number = np.zeros(len(firsts) + 1, dtype=np.int32)
    number[order + 1] = np.arange(1, len(firsts) + 1, dtype=np.int32)
    return number[flat].reshape(Z, Y, X), len(firsts), cls


def table(labels, cls, count):
    """(sizes int32 [count + 1], classes uint8 [count + 1], first int32 [count + 1]) of a labelling: the voxels, the class and the raster
    index of the first voxel of each label; entry 0 (no component) is (0, 0, -1)."""
    dev, Z, Y, X = _pair(labels, cls)
    K = _count(count)
    if dev:
        from . import _native as nv
        sizes = torch.empty(K + 1, dtype=torch.int32, device=labels.device)
        classes = torch.empty(K + 1, dtype=torch.uint8, device=labels.device)
        first = torch.empty(K + 1, dtype=torch.int32, device=labels.device)
        with torch.cuda.device(labels.device):
            nv.call('iunet_cc_table', nv.ptr(labels), nv.ptr(cls), Z, Y, X, K, nv.ptr(sizes), nv.ptr(classes), nv.ptr(first), nv.stream())
        return sizes, classes, first
    flat = labels.reshape(-1)
    sizes = np.bincount(flat, minlength=K + 1)[:K + 1].astype(np.int32)
    sizes[0] = 0
    first = np.full(K + 1, -1, dtype=np.int32)
    at = np.flatnonzero(flat)
    found, where = np.unique(flat[at], return_index=True)
    first[found] = at[where]
    classes = np.zeros(K + 1, dtype=np.uint8)
    classes[1:] = cls.reshape(-1)[first[1:]]
    return sizes, classes, first


def filter_components(labels, cls, count, keep, fill):
    """uint8 [Z, Y, X]: cls with the voxels of every component k whose keep[k] is 0 set to `fill` (keep: uint8 / bool [count + 1], where
    labels and cls live)."""
    dev, Z, Y, X = _pair(labels, cls)
    K, fill = _count(count), _fill(fill, None)
    if dev:
        from . import _native as nv
        keep = keep.to(torch.uint8).contiguous()
        if keep.device != labels.device or keep.numel() != K + 1:
            raise ValueError(f'keep must hold count + 1 = {K + 1} flags on the labels\' device')
        out = torch.empty_like(cls)
        with torch.cuda.device(labels.device):
            nv.call('iunet_cc_filter', nv.ptr(labels), nv.ptr(cls), Z, Y, X, K, nv.ptr(keep), fill, nv.ptr(out), nv.stream())
        return out
    keep = np.asarray(keep).astype(bool)
    if keep.shape != (K + 1,):
        raise ValueError(f'keep must hold count + 1 = {K + 1} flags')
    return np.where((labels > 0) & ~keep[labels], np.uint8(fill), cls).astype(np.uint8)


def largest_flags(sizes, classes, n, per_class):
    """uint8 / bool [K + 1] flags of the n largest components (of each class: per_class), equal sizes in order of label.  Plumbing on the
    K-entry tables, with torch where they are resident."""
    dev = torch.is_tensor(sizes)
    K = int(sizes.shape[0]) - 1
    if dev:
        order = torch.sort(sizes[1:].to(torch.int64), descending=True, stable=True).indices
        if per_class:
            order = order[torch.sort(classes[1:][order].to(torch.int64), stable=True).indices]
            c = classes[1:][order]
            pos = torch.arange(K, device=sizes.device)
            head = torch.ones(K, dtype=torch.bool, device=sizes.device)
            head[1:] = c[1:] != c[:-1]
            rank = pos - torch.cummax(torch.where(head, pos, torch.zeros_like(pos)), 0).values if K else pos
        else:
            rank = torch.arange(K, device=sizes.device)
        keep = torch.zeros(K + 1, dtype=torch.uint8, device=sizes.device)
        keep[order + 1] = (rank < n).to(torch.uint8)
        return keep
    order = np.argsort(-sizes[1:].astype(np.int64), kind='stable')
    if per_class:
        order = order[np.argsort(classes[1:][order], kind='stable')]
        c = classes[1:][order]
        pos = np.arange(K)
        head = np.ones(K, dtype=bool)
        head[1:] = c[1:] != c[:-1]
        rank = pos - np.maximum.accumulate(np.where(head, pos, 0)) if K else pos
    else:
        rank = np.arange(K)
    keep = np.zeros(K + 1, dtype=bool)
    keep[order + 1] = rank < n
    return keep


def remove_small(src, min_size, connectivity=6, background=0, fill=None):
    """The class map uint8 [Z, Y, X] of src with every component of fewer than min_size voxels set to `fill` (default: the background,
    0 where every class is labelled)."""
    fill = _fill(fill, background)
    min_size = resident.check_count(min_size, 'min_size')
    labels, count, cls = label(src, connectivity, background)
    sizes, _, _ = table(labels, cls, count)
    return filter_components(labels, cls, count, sizes >= min_size, fill)


def keep_largest(src, n=1, per_class=True, connectivity=6, background=0, fill=None):
    """The class map uint8 [Z, Y, X] of src with only the n largest components kept -- of each class (per_class) or of all -- and the
    others set to `fill` (default: the background, 0 where every class is labelled).  Of components of equal size the one with the
    smaller label (the earlier first voxel) is kept."""
    fill = _fill(fill, background)
    n = resident.check_count(n, 'n')
    labels, count, cls = label(src, connectivity, background)
    sizes, classes, _ = table(labels, cls, count)
    return filter_components(labels, cls, count, largest_flags(sizes, classes, n, bool(per_class)), fill)
