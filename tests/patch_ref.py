"""The arithmetic contract of iunet_patch_batch restated in numpy float32 -- a helper, not a test module.
Written from the contract, not from the kernel: every multiply and add below is one float32 operation, rounded, in the order the
contract gives (numpy never fuses a multiply into an add), so the kernel's fp16 outputs must equal these bit for bit.

  t_j = o_j - (S_j - 1) / 2;  p_a = ((m[a][0] t_z + m[a][1] t_y) + m[a][2] t_x) + c[a];  r_a = rint(p_a) (ties to even)
  inside <=> 0 <= r_a <= dim_a - 1 on the three axes;  lit = inside and (image[r][0] != 0 or keep_dark)
  y[k] = lut[255] if lit and mask[r] == k else lut[0];  w[k] = lut[weight[r]] if lit else lut[0]
  X, order 0: lut[image[r][c]] if inside else lut[0]
  X, order 1: trilinear over the 8 neighbours of floor(p) (outside taps 0), f = p - floor(p), a + f (b - a) along x, y, z; fp16(v / 255)
"""
import numpy as np

F = np.float32
LUT = (np.arange(256) / 255).astype(np.float32).astype(np.float16)          # the 2-D producer's table: fp16(float32(v / 255))


def coordinates(m, c, patch):
    """Source coordinates p [3][SZ][SY][SX] (float32) of a patch's voxels."""
    m, c = np.asarray(m, dtype=F).reshape(3, 3), np.asarray(c, dtype=F)
    t = [np.arange(S, dtype=F) - F((S - 1) / 2) for S in patch]
    tz, ty, tx = t[0][:, None, None], t[1][None, :, None], t[2][None, None, :]
    return np.stack([((m[a, 0] * tz + m[a, 1] * ty) + m[a, 2] * tx) + c[a] for a in range(3)])


def nearest(p, shape):
    """(r int64 [3][...] clipped into the volume for indexing, inside bool [...])."""
    r = np.rint(p)
    inside = np.ones(p.shape[1:], bool)
    for a in range(3):
        inside &= (r[a] >= 0) & (r[a] <= shape[a] - 1)
    idx = [np.clip(r[a], 0, shape[a] - 1).astype(np.int64) for a in range(3)]
    return idx, inside


def patch(image, mask, weight, m, c, patch, num_classes, order, keep_dark=False):
    """(X [ch][SZ][SY][SX], y [C][...], w [C][...]) float16 of one sample.  image uint8 [Z][Y][X][ch] (or [Z][Y][X]), mask and
    weight uint8 [Z][Y][X]."""
    image = image[..., None] if image.ndim == 3 else image
    shape, ch = image.shape[:3], image.shape[3]
    p = coordinates(m, c, patch)
    (rz, ry, rx), inside = nearest(p, shape)
    lit = inside & ((image[rz, ry, rx, 0] != 0) | bool(keep_dark))
    k = mask[rz, ry, rx]
    wv = np.where(lit, LUT[weight[rz, ry, rx]], LUT[0])
    y = np.stack([np.where(lit & (k == cls), LUT[255], LUT[0]) for cls in range(num_classes)])
    w = np.stack([wv] * num_classes)
    if order == 0:
        X = np.stack([np.where(inside, LUT[image[rz, ry, rx, q]], LUT[0]) for q in range(ch)])
        return X, y, w
    fl = np.floor(p)
    f = p - fl                                                              # float32
    lo = fl.astype(np.int64)

    def tap(q, dz, dy, dx):
        z, yy, x = lo[0] + dz, lo[1] + dy, lo[2] + dx
        ok = (z >= 0) & (z < shape[0]) & (yy >= 0) & (yy < shape[1]) & (x >= 0) & (x < shape[2])
        v = image[np.clip(z, 0, shape[0] - 1), np.clip(yy, 0, shape[1] - 1), np.clip(x, 0, shape[2] - 1), q]
        return np.where(ok, v, 0).astype(F)

    def lerp(a, b, fr):
        return a + fr * (b - a)

    X = []
    for q in range(ch):
        along_x = [[lerp(tap(q, dz, dy, 0), tap(q, dz, dy, 1), f[2]) for dy in (0, 1)] for dz in (0, 1)]
        along_y = [lerp(along_x[dz][0], along_x[dz][1], f[1]) for dz in (0, 1)]
        v = lerp(along_y[0], along_y[1], f[0])
        assert v.dtype == F
        X.append((v / F(255.0)).astype(np.float16))
    return np.stack(X), y, w


def crop(image, mask, weight, corner, patch, num_classes):
    """The plain crop at integer `corner` (inside the volume) through the LUT: image, one-hot mask, repeated weight (no dark rule)."""
    image = image[..., None] if image.ndim == 3 else image
    box = tuple(slice(o, o + s) for o, s in zip(corner, patch))
    X = np.moveaxis(LUT[image[box]], -1, 0)
    y = np.stack([np.where(mask[box] == cls, LUT[255], LUT[0]) for cls in range(num_classes)])
    w = np.stack([LUT[weight[box]]] * num_classes)
    return X, y, w


def signed_permutations():
    """The 48 signed permutation matrices of three axes."""
    import itertools
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            M = np.zeros((3, 3))
            for a in range(3):
                M[a, perm[a]] = signs[a]
            out.append(M)
    return out


def transform_crop(arr, M, corner, patch):
    """out[o] = arr[corner + source offset] for a signed permutation M (rows: source axes, columns: patch axes) by np.transpose /
    np.flip of a plain crop: source axis a runs along patch axis perm[a] with sign M[a][perm[a]].  arr: [Z][Y][X] (+ trailing axes);
    corner: the lowest source index the patch reads on each axis."""
    perm = [int(np.argmax(np.abs(M[a]))) for a in range(3)]
    box = tuple(slice(corner[a], corner[a] + patch[perm[a]]) for a in range(3))
    sub = arr[box]
    for a in range(3):
        if M[a, perm[a]] < 0:
            sub = np.flip(sub, axis=a)
    inv = [perm.index(j) for j in range(3)]                                # patch axis j is source axis inv[j]
    return np.transpose(sub, inv + list(range(3, sub.ndim)))


def snapped_centre(M, corner, patch):
    """The centre that makes a signed permutation M read the integer source box starting at `corner` (even patch sizes: half-integer)."""
    return [corner[a] + (patch[int(np.argmax(np.abs(M[a])))] - 1) / 2 for a in range(3)]


def make_volume(rng, shape, ch=1, classes=2, dark=False):
    """(image [Z][Y][X][ch] without zeros unless `dark`, mask class ids < classes, weight [Z][Y][X][2]) uint8."""
    image = rng.integers(0 if dark else 1, 256, tuple(shape) + (ch,), dtype=np.uint8)
    mask = rng.integers(0, classes, shape, dtype=np.uint8)
    weight = rng.integers(0, 256, tuple(shape) + (2,), dtype=np.uint8)
    return image, mask, weight


def rotation(axis, degrees, scale=1.0):
    """scale * (rotation by `degrees` about `axis`), Rodrigues' formula in float64."""
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = np.radians(degrees)
    return scale * (np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K))
