"""The definition of the connected-component labelling: what iunet_cc_label, iunet_cc_table and iunet_cc_filter
compute, and what interactive_unet/components.py builds on them, restated with numpy and scipy.ndimage.  Nothing here imports the package.

Input src, uint8: a class map [Z][Y][X], or a predicted volume [Z][Y][X][C], 2 <= C <= 16 -- a voxel's class is the index of its
largest byte, the lowest index on a tie; a voxel whose bytes are all 0 was never predicted and belongs to no component.
background = None / -1 (every class is labelled) or 0 .. 255: voxels of that class belong to no component.
connectivity 6, 18 or 26 = scipy.ndimage.generate_binary_structure(3, 1 | 2 | 3).
Two voxels are connected if they are neighbours under the structure, have the same class and are both foreground; a component is a
class of the transitive closure; its first voxel is the member with the smallest raster index (z Y + y) X + x; components are numbered
1 .. K in increasing order of first voxel.  labels int32 [Z][Y][X], 0 for voxels of no component.  For a binary class map this is
scipy.ndimage.label's own numbering (tests/test_components_cpu.py checks it).
Table: sizes int32 [K + 1] (entry 0 = 0), classes uint8 [K + 1] (entry 0 = 0), first int32 [K + 1] (entry 0 = -1).
Filter: out[v] = (keep[labels[v]] ? cls[v] : fill) where labels[v] > 0, cls[v] elsewhere."""
import numpy as np
from scipy import ndimage

RANK = {6: 1, 18: 2, 26: 3}


def class_map(src, background=0):
    """(cls uint8 [Z, Y, X], foreground bool [Z, Y, X]) of src."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim in (3, 4)
    if src.ndim == 3:
        cls, fg = src.copy(), np.ones(src.shape, dtype=bool)
    else:
        assert 2 <= src.shape[3] <= 16
        cls = np.argmax(src, axis=-1).astype(np.uint8)          # numpy's argmax returns the first of equal maxima
        fg = src.max(axis=-1) > 0
    if background is not None and background != -1:
        fg = fg & (cls != background)
    return cls, fg


def label(src, connectivity=6, background=0):
    """(labels int32 [Z, Y, X], K, cls uint8 [Z, Y, X]): one ndimage.label call per class, ndimage.minimum of the raster index per
    label, np.unique / searchsorted for the numbering."""
    cls, fg = class_map(src, background)
    structure = ndimage.generate_binary_structure(3, RANK[connectivity])
    lin = np.arange(cls.size, dtype=np.int64).reshape(cls.shape)
    root = np.full(cls.shape, -1, dtype=np.int64)               # the raster index of the first voxel of the voxel's component
    for c in np.unique(cls[fg]):
        lab, k = ndimage.label(fg & (cls == c), structure=structure)
        if k == 0:
            continue
        mins = np.asarray(ndimage.minimum(lin, lab, index=np.arange(1, k + 1))).astype(np.int64)
        m = lab > 0
        root[m] = mins[lab[m] - 1]
    roots = np.unique(root[root >= 0])
    labels = np.zeros(cls.shape, dtype=np.int32)
    m = root >= 0
    labels[m] = np.searchsorted(roots, root[m]) + 1
    return labels, len(roots), cls


def table(labels, cls, K):
    """(sizes, classes, first) by a loop over the voxels' labels."""
    flat, c = np.asarray(labels).reshape(-1), np.asarray(cls).reshape(-1)
    sizes, classes, first = np.zeros(K + 1, np.int32), np.zeros(K + 1, np.uint8), np.full(K + 1, -1, np.int32)
    for v in np.flatnonzero(flat).tolist():
        k = flat[v]
        sizes[k] += 1
        if first[k] < 0:
            first[k], classes[k] = v, c[v]
    return sizes, classes, first


def filter_components(labels, cls, keep, fill):
    keep = np.asarray(keep).astype(bool)
    out = np.asarray(cls).copy()
    drop = (labels > 0) & ~keep[labels]
    out[drop] = fill
    return out


def default_fill(background):
    return 0 if background in (None, -1) else background


def remove_small(src, min_size, connectivity=6, background=0, fill=None):
    labels, K, cls = label(src, connectivity, background)
    sizes, _, _ = table(labels, cls, K)
    return filter_components(labels, cls, sizes >= min_size, default_fill(background) if fill is None else fill)


def keep_largest(src, n=1, per_class=True, connectivity=6, background=0, fill=None):
    """The n largest components (of each class: per_class); of equal sizes the smaller label first."""
    labels, K, cls = label(src, connectivity, background)
    sizes, classes, _ = table(labels, cls, K)
    keep = np.zeros(K + 1, dtype=bool)
    groups = sorted(set(classes[1:].tolist())) if per_class else [None]
    for g in groups:
        members = [k for k in range(1, K + 1) if g is None or classes[k] == g]
        for k in sorted(members, key=lambda k: (-int(sizes[k]), k))[:n]:
            keep[k] = True
    return filter_components(labels, cls, keep, default_fill(background) if fill is None else fill)
