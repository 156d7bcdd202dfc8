"""Inputs that tests/test_reconstruct_cpu.py and tests/test_gpu_reconstruct.py share: written once, so a name means the same bytes in both."""
import numpy as np

HIGH = 2 ** 31 - 1


def ball(shape, c, r):
    z, y, x = np.indices(shape)
    return (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= r * r


def planted():
    """48^3: two overlapping balls of radius 9 and, apart from them, one of radius 3.  Two objects, three grains."""
    shape = (48, 48, 48)
    return (ball(shape, (24, 24, 14), 9) | ball(shape, (24, 24, 29), 9) | ball(shape, (8, 8, 40), 3)).astype(np.uint8)


def blobs(shape, density, seed):
    """uint8: a Gaussian-smoothed random field above the quantile that leaves `density` of the voxels."""
    from scipy import ndimage
    f = ndimage.gaussian_filter(np.random.default_rng(seed).standard_normal(shape), 2.0)
    return (f > np.quantile(f, 1 - density)).astype(np.uint8)


def landscape_values():
    """int32 [1, 1, N] squared distances: 0 .. 3, k^2 - 1, k^2, k^2 + 1 for every k up to 46340, and 2^31 - 1."""
    k = np.arange(1, 46341, dtype=np.int64)
    values = np.concatenate([[0, 1, 2, 3], k * k - 1, k * k, k * k + 1, [HIGH]])
    assert values.max() == HIGH and values.min() == 0
    return values.astype(np.int32).reshape(1, 1, -1)


def serpentine(shape, z=None):
    """(a uint8 [Z, Y, X], path int [n, 3]): section 27's corridor of one voxel's width in the plane z: the rows of even y, joined at
    alternating ends through the odd rows; path lists its voxels from one end to the other."""
    Z, Y, X = shape
    z = Z // 2 if z is None else z
    path = []
    for k, y in enumerate(range(0, Y, 2)):
        xs = range(X) if k % 2 == 0 else range(X - 1, -1, -1)
        path += [(z, y, x) for x in xs]
        if y + 2 < Y:
            path.append((z, y + 1, path[-1][2]))
    path = np.array(path)
    a = np.zeros(shape, np.uint8)
    a[tuple(path.T)] = 1
    assert a.sum() == len(path)
    return a, path
