"""Helpers of tests/test_gpu_volume_scale.py -- a helper, not a test module; nothing here imports the package.

The shapes at which the resident-volume kernels change their launch policy or pass 2^31 elements / 2^32 bytes, the tiled closed form
of a labelling too large for a direct reference, and the dyadic geometries under which a definition evaluated on a host crop IS the
definition on the whole volume.  tests/test_volume_scale_cpu.py checks all of it without a GPU.

The tiled closed form.  A block B [bz, Y, X] is labelled once by tests/components_ref.py: labels lab_B, K_B components.  The big volume
is n copies of B along z, each followed by one separator plane that belongs to no component of B and touches none: the background
class (background given), one class that does not occur in B (background None: the plane is component K_B + 1 of its copy), or all-zero
bytes ("never predicted": C >= 2, no component under either background).  Components never cross a separator plane, every voxel of
copy i follows every voxel of copy i - 1 in raster order, so copy i holds the labels lab_B + i * period where lab_B > 0, period = K_B
(+ 1 with a separator component); sizes and classes repeat; first shifts by i * (bz + 1) * Y * X.  bz + 1 is no multiple of the tile's 4
planes, so the copies sit differently in the tiles."""
import numpy as np
import torch

from tests import components_ref as cr

# ---- Part A: connected components where the launch policy changes (csrc/components.hip) ----
A1_SHAPE = (131, 258, 261)                # 2154 chunks: scan per = 3, table per = 2; ragged against the 4 x 16 x 64 tile on every axis
A2_COLUMN = (4194320, 1, 1)               # 1 048 580 tiles: four more than the tile grid's cap
A2_THIN = (2097160, 1, 65)                # the same number of tiles, two across x
A2_THIN_BZ = 36                           # 56 680 copies of 36 planes + 1
A3_SHAPE = (700, 1201, 1301, 4)           # = V8C: 1.09e9 voxels, 4.37e9 bytes
A3_BZ = 4                                 # 140 copies of 4 planes + 1
A4_SHAPE = (32767, 256, 256)              # 2^31 - 65536 voxels
A4_BZ = 30                                # 1057 copies of 30 planes + 1

# ---- Part B: flat indices past 2^31 elements and 2^32 bytes ----
V8_SHAPE = (1031, 2053, 2063)             # uint8, 4 366 634 509 voxels > 2^32; no extent a multiple of 16
V8C_SHAPE = A3_SHAPE                      # uint8, 4.37e9 bytes
VF_SHAPE = (700, 1201, 1301, 2)           # fp32, 2.19e9 elements > 2^31
CROP = 128                                # the host crops: the first / last CROP planes, rows and columns


def copies(shape, bz):
    """The number of copies of a block of bz planes (+ 1 separator) that make up `shape` exactly."""
    assert shape[0] % (bz + 1) == 0 and (bz + 1) % 4 != 0, (shape, bz)
    return shape[0] // (bz + 1)


def table_fast(labels, cls, K):
    """tests/components_ref.table by np.bincount / np.unique instead of a loop over the voxels (test_volume_scale_cpu.py: equal)."""
    flat, c = np.asarray(labels).reshape(-1), np.asarray(cls).reshape(-1)
    sizes = np.bincount(flat, minlength=K + 1).astype(np.int32)
    sizes[0] = 0
    first, classes = np.full(K + 1, -1, np.int32), np.zeros(K + 1, np.uint8)
    at = np.flatnonzero(flat)
    ids, where = np.unique(flat[at], return_index=True)            # the first occurrence of every label
    first[ids] = at[where]
    classes[ids] = c[at[where]]
    return sizes, classes, first


class Tiled(object):
    """The closed form of one (block, connectivity, background): everything torch, on the device of `device`."""

    def __init__(self, block, connectivity, background, separator, device='cpu'):
        """block: uint8 [bz, Y, X] class map or [bz, Y, X, C] predicted bytes; separator: the separator plane's byte (C >= 2: 0)."""
        block = np.asarray(block)
        self.bz, self.Y, self.X = block.shape[:3]
        self.C = 1 if block.ndim == 3 else block.shape[3]
        self.separator, self.background = int(separator), background
        lab, K, cls = cr.label(block, connectivity, background)
        sizes, classes, first = table_fast(lab, cls, K)
        # the separator plane as a component of its own: a class map under background None
        self.sep_component = self.C == 1 and background in (None, -1)
        if self.C == 1:
            assert separator == background or (self.sep_component and not (block == separator).any())
        else:
            assert separator == 0
        self.K_B, self.period = K, K + int(self.sep_component)
        self.plane = self.Y * self.X
        self.stride = (self.bz + 1) * self.plane                   # voxels from one copy to the next
        if self.sep_component:
            sizes = np.append(sizes, self.plane).astype(np.int32)
            classes = np.append(classes, separator).astype(np.uint8)
            first = np.append(first, self.bz * self.plane).astype(np.int32)
        self.sep_cls = separator if self.C == 1 else 0
        dev = torch.device(device)
        self.block = torch.from_numpy(block).to(dev)
        self.lab = torch.from_numpy(lab).to(dev)
        self.cls_B = torch.from_numpy(cls).to(dev)
        self.sizes_B, self.classes_B, self.first_B = (torch.from_numpy(t).to(dev) for t in (sizes, classes, first))

    def count(self, n):
        return n * self.period

    def volume(self, n):
        """The source: uint8 [n (bz + 1), Y, X(, C)]."""
        tail = tuple(self.block.shape[1:])
        out = torch.full((n, self.bz + 1) + tail, self.separator, dtype=torch.uint8, device=self.block.device)
        out[:, :self.bz] = self.block[None]
        return out.view((n * (self.bz + 1),) + tail)

    def labels(self, i0, i1):
        """int32 [(i1 - i0) (bz + 1), Y, X]: the labels of copies i0 .. i1 - 1."""
        dev = self.lab.device
        shift = (torch.arange(i0, i1, device=dev, dtype=torch.int64) * self.period).to(torch.int32)[:, None, None, None]
        out = torch.empty((i1 - i0, self.bz + 1, self.Y, self.X), dtype=torch.int32, device=dev)
        out[:, :self.bz] = torch.where(self.lab[None] > 0, self.lab[None] + shift, torch.zeros((), dtype=torch.int32, device=dev))
        out[:, self.bz] = (shift[:, 0] + self.period) if self.sep_component else 0
        return out.view(-1, self.Y, self.X)

    def cls(self, i0, i1):
        """uint8 [(i1 - i0) (bz + 1), Y, X]: the class map of copies i0 .. i1 - 1."""
        out = torch.full((i1 - i0, self.bz + 1, self.Y, self.X), self.sep_cls, dtype=torch.uint8, device=self.lab.device)
        out[:, :self.bz] = self.cls_B[None]
        return out.view(-1, self.Y, self.X)

    def table(self, n):
        """(sizes int32, classes uint8, first int32) [n period + 1]."""
        dev = self.lab.device
        head = lambda v, dt: torch.tensor([v], dtype=dt, device=dev)
        sizes = torch.cat([head(0, torch.int32), self.sizes_B[1:].repeat(n)])
        classes = torch.cat([head(0, torch.uint8), self.classes_B[1:].repeat(n)])
        shift = torch.arange(n, device=dev, dtype=torch.int64)[:, None] * self.stride
        first = (self.first_B[1:].to(torch.int64)[None] + shift).reshape(-1)
        assert n == 0 or self.period == 0 or int(first.max()) <= 0x7fffffff
        return sizes, classes, torch.cat([head(-1, torch.int32), first.to(torch.int32)])


# ---- dyadic geometries ----------------------------------------------------------------------------------------------------
# Direction vectors and origins whose components are multiples of 2^-8 (|direction| <= 2, origin < 4096): with integer sample offsets
# below 2^12 every product has at most 10 + 12 significant bits and every sum is a multiple of 2^-8 below 2^14 -- 22 bits --, so every
# float64 operation of the definitions is exact, and subtracting a crop's integer offset from the origin shifts every coordinate by
# exactly that integer.  floor(c + 0.5) and the linear weights then shift with it for any integer offset, rint (ties to even) for an even
# one: far_offset() is even.  The fp32 patch producer: multiples of 2^-4, |m| <= 2, centres below 4096, patch offsets half-integers below 64:
# products of 6 + 7 bits, sums multiples of 2^-5 below 2^13 -- 18 bits of 24.
D8 = 1.0 / 256


def is_dyadic(values, unit, bound):
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    return bool(np.all(v / unit == np.rint(v / unit)) and np.all(np.abs(v) <= bound))


# oblique, not unit: (a, b, n) in units of 2^-8
SLAB_VECTORS = (np.array([192.0, 64.0, -128.0]) * D8, np.array([-32.0, 224.0, 96.0]) * D8, np.array([160.0, -96.0, 208.0]) * D8)
E = np.eye(3)
SLAB = (9, 48)                            # (planes, width) of the slabs and planes the tests take


def far_origin(shape, back):
    """An origin `back` voxels (+ a dyadic fraction) inside the far corner of `shape`."""
    return np.array([shape[0] - back[0] + 37 * D8, shape[1] - back[1] - 101 * D8, shape[2] - back[2] + 200 * D8])


def far_offset(shape):
    """The offset of the crop of the last CROP (or CROP + 1) planes, rows and columns: EVEN on every axis.  The paste, the scatter and
    the patch producer round to the nearest voxel with ties to even, and rint(c - k) = rint(c) - k at a tie only for an even k."""
    return np.array([(shape[x] - CROP) // 2 * 2 for x in range(3)], dtype=np.int64)


def slab_geometries(shape):
    """name -> (a, b, n, origin) of the slabs / planes at the far corner of `shape`."""
    a, b, n = SLAB_VECTORS
    return {'oblique': (a, b, n, far_origin(shape, (20, 24, 18))),
            'axes': (E[1], E[2], E[0], np.array([shape[0] - 3.0, shape[1] - 9.0, shape[2] - 5.0])),
            'half-integer': (E[2], E[0], E[1], np.array([shape[0] - 8.5, shape[1] - 4.5, shape[2] - 10.5]))}


def origin_geometries():
    """The same directions around the volume's first corner."""
    a, b, n = SLAB_VECTORS
    return {'oblique': (a, b, n, np.array([20 + 37 * D8, 24 - 101 * D8, 18 + 200 * D8])),
            'axes': (E[1], E[2], E[0], np.array([3.0, 9.0, 5.0]))}


def shifted(geom, offset):
    """The geometry seen from a crop that starts at the integer `offset`: the origin (the last vector) moves, nothing else."""
    return tuple(geom[:-1]) + (np.asarray(geom[-1], dtype=np.float64) - np.asarray(offset, dtype=np.float64),)


D4 = 1.0 / 16
PATCH = (16, 24, 32)
PATCH_POSES = {'identity': np.eye(3), 'signed permutation': np.array([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]),
               'dyadic': np.array([[16.0, 4.0, -8.0], [-4.0, 14.0, 2.0], [8.0, 0.0, 12.0]]) * D4,
               'dyadic, scaled': np.array([[24.0, -6.0, 0.0], [2.0, 20.0, -10.0], [-12.0, 4.0, 18.0]]) * D4}


def patch_centre(shape):
    return np.array([shape[0] - 9 + 3 * D4, shape[1] - 14 - 5 * D4, shape[2] - 12 + 8 * D4])
