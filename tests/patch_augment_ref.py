"""The definition of the 3-D patch producer's three further transforms -- elastic deformation, intensity
jitter and "Gaussian blur or Gaussian noise", what section 17 gave the 2-D producer, on top of the oblique patch gather of
tests/patch_ref.py -- in numpy float32.  A helper, not a test module.  Every multiply and add below is one float32 operation,
rounded, in the order given (numpy never fuses a multiply into an add), so the fp16 outputs of iunet_patch_batch_extra can be asked
to equal these bit for bit (X on Gaussian-noise samples: up to a device's logf / cosf, see `gaussian_noise`).

  notation   patch_ref's: patch (SZ, SY, SX), voxel o = (oz, oy, ox), t_j = o_j - (S_j - 1) / 2,
             p_a = ((m[a][0] t_z + m[a][1] t_y) + m[a][2] t_x) + c[a]
  noise      augment_ref.philox4x32 under one 64-bit key per sample and use; counter words (ox, oy, oz, 2 c) for elastic field c
             (0 / 1 / 2: the displacement along patch z / y / x), (ox, oy, oz, 2 q + 1) for the noise of image channel q
  elastic    n_c[o] = 2 u - 1, u = (word0 >> 8) 2^-24; taps augment_ref.taps(sigma) (K = int(8 sigma + 1) made odd, r = K // 2);
             three passes, along x, then y, then z, each acc = 0; acc += g_i * src[reflect(p + i - r)], i ascending, reflect without
             edge repeat (every patch extent must exceed r); d_c = blurred_c * float32(alpha / 2) voxels, NOT rounded;
             t'_j = t_j + d_j (one float32 add per axis); p = the chain above at t'.  From p on everything is patch_ref.patch:
             rint / inside / dark rule / one-hot / weight for y and w, order 0 or trilinear order 1 (outside taps 0) for the image.
  jitter     (image only) x_q = the float32 value that patch_ref rounds to fp16: order 1: v / 255; order 0: float32(byte / 255), 0
             outside.  bright(x) = clamp(x b, 0, 1), contrast(x) = clamp(c x + (1 - c) m, 0, 1), in drawn order.  The mean m is
             exact and independent of how a device reduces: a 256-bin integer histogram of the sample's BYTE values over all
             channels and voxels (order 0: the gathered byte, outside 0; order 1: rint(v), ties to even), N = ch SZ SY SX,
             m = float32(sum_v hist[v] float64(E[v]) / N) summed in float64 in ascending v, E[v] = what enters the contrast step:
             float32(v / 255), or bright of it when brightness comes first.  At order 1 the mean comes from the byte rounding
             while the transform acts on the unrounded x: this is the definition.
  blur       (image only, on the jittered field J) 5 taps augment_ref.taps(sigma_b, 5), separable, along x, then y, then z, the same
             ascending accumulation and reflecting borders (every extent must exceed 2); float32 denormal taps are kept
  noise      clamp(J + sigma_n z, 0, 1), u1 = ((w0 >> 8) + 1) 2^-24, u2 = (w1 >> 8) 2^-24, z = sqrtf(-2 logf(u1)) cosf(6.2831855f u2)
  X          = fp16 (nearest even) of the float32 result; y and w as patch_ref's, at the displaced coordinate

With alpha = 0, b = c = 1 and neither blur nor noise the result is patch_ref.patch bit for bit: t + 0 = t; clamp(x 1, 0, 1) = x
for x in [0, 1]; 1 x + 0 m = x.

Draw order the definition fixes for a loader (one torch generator; per sample): loader.VolumeDataset.draw() -- volume index, m, c --
then loader.draw_extra(gen, ...) exactly as the 2-D loader calls it: the elastic key; rand < 0.5 -> contrast first, then b ~
U(0.75, 1.25), then c ~ U(0.5, 2); randint(0, 2): 0 blur, then sigma_b ~ U(0.1, 2); 1 noise, then the key.  With the transforms off
nothing more is drawn.
"""
import numpy as np

from tests import augment_ref as ar
from tests import patch_ref as pr

F = np.float32
LUT32 = ar.LUT32                                                  # float32(v / 255)
LUT = pr.LUT


def _counter(patch):
    SZ, SY, SX = patch
    return (np.arange(SX, dtype=np.uint32)[None, None, :], np.arange(SY, dtype=np.uint32)[None, :, None],
            np.arange(SZ, dtype=np.uint32)[:, None, None])


def noise_field(patch, key, c):
    """n_c [SZ][SY][SX] float32 in [-1, 1)."""
    xs, ys, zs = _counter(patch)
    w0 = ar.philox4x32((xs, ys, zs, np.uint32(2 * c)), ar.key_words(key))[0]
    u = (w0 >> np.uint32(8)).astype(F) * F(2.0 ** -24)
    return F(2) * u - F(1)


def smooth(field, g):
    """The three passes: along x, then y, then z."""
    return ar.blur_pass(ar.blur_pass(ar.blur_pass(field, g, 2), g, 1), g, 0)


def displacement(patch, key, alpha, g):
    """d [3][SZ][SY][SX] float32, voxels along patch z / y / x."""
    return np.stack([smooth(noise_field(patch, key, c), g) * F(alpha / 2) for c in range(3)])


def coordinates(m, c, patch, d=None):
    """Source coordinates p [3][SZ][SY][SX] (float32) at t' = t + d (d = None: t, which is patch_ref.coordinates)."""
    m, c = np.asarray(m, dtype=F).reshape(3, 3), np.asarray(c, dtype=F)
    t = [np.arange(S, dtype=F) - F((S - 1) / 2) for S in patch]
    tz, ty, tx = [np.broadcast_to(v, patch) for v in (t[0][:, None, None], t[1][None, :, None], t[2][None, None, :])]
    if d is not None:
        assert d.dtype == F
        tz, ty, tx = tz + d[0], ty + d[1], tx + d[2]
    p = np.stack([((m[a, 0] * tz + m[a, 1] * ty) + m[a, 2] * tx) + c[a] for a in range(3)])
    assert p.dtype == F
    return p


def gather(image, mask, weight, p, num_classes, order, keep_dark=False):
    """patch_ref.patch from p on: (x [ch][...] float32 -- the value patch_ref rounds to fp16 --, byte [ch][...] uint8 -- what the
    jitter histogram counts --, y, w float16)."""
    shape, ch = image.shape[:3], image.shape[3]
    (rz, ry, rx), inside = pr.nearest(p, shape)
    lit = inside & ((image[rz, ry, rx, 0] != 0) | bool(keep_dark))
    k = mask[rz, ry, rx]
    wv = np.where(lit, LUT[weight[rz, ry, rx]], LUT[0])
    y = np.stack([np.where(lit & (k == cls), LUT[255], LUT[0]) for cls in range(num_classes)])
    w = np.stack([wv] * num_classes)
    if order == 0:
        byte = np.stack([np.where(inside, image[rz, ry, rx, q], 0) for q in range(ch)]).astype(np.uint8)
        return LUT32[byte], byte, y, w
    fl = np.floor(p)
    f = p - fl
    lo = fl.astype(np.int64)

    def tap(q, dz, dy, dx):
        z, yy, x = lo[0] + dz, lo[1] + dy, lo[2] + dx
        ok = (z >= 0) & (z < shape[0]) & (yy >= 0) & (yy < shape[1]) & (x >= 0) & (x < shape[2])
        v = image[np.clip(z, 0, shape[0] - 1), np.clip(yy, 0, shape[1] - 1), np.clip(x, 0, shape[2] - 1), q]
        return np.where(ok, v, 0).astype(F)

    def lerp(a, b, fr):
        return a + fr * (b - a)

    xs, bytes_ = [], []
    for q in range(ch):
        along_x = [[lerp(tap(q, dz, dy, 0), tap(q, dz, dy, 1), f[2]) for dy in (0, 1)] for dz in (0, 1)]
        along_y = [lerp(along_x[dz][0], along_x[dz][1], f[1]) for dz in (0, 1)]
        v = lerp(along_y[0], along_y[1], f[0])
        assert v.dtype == F
        xs.append(v / F(255.0))
        bytes_.append(np.rint(v).astype(np.uint8))
    return np.stack(xs), np.stack(bytes_), y, w


clamp01 = ar.clamp01


def contrast_mean(byte, b, contrast_first):
    """m: the exact mean of what enters the contrast step, from the histogram of the sample's bytes (augment_ref.histogram_mean)."""
    entering = LUT32 if contrast_first else clamp01(LUT32 * F(b))
    return ar.histogram_mean(byte, entering)


def jitter(x, byte, b, c, contrast_first):
    b, c = F(b), F(c)
    m = contrast_mean(byte, b, contrast_first)

    def bright(v):
        return clamp01(v * b)

    def contrast(v):
        return clamp01(c * v + (F(1) - c) * m)
    out = bright(contrast(x)) if contrast_first else contrast(bright(x))
    assert out.dtype == F
    return out


def gaussian_blur(J, sigma_b):
    """The separable 5-tap blur of J [ch][SZ][SY][SX] float32: along x, then y, then z."""
    k = ar.taps(sigma_b, 5)
    return ar.blur_pass(ar.blur_pass(ar.blur_pass(J, k, 3), k, 2), k, 1)


def noise_uniforms(ch, patch, key):
    """(u1, u2) [ch][SZ][SY][SX] float32 of Box-Muller."""
    xs, ys, zs = _counter(patch)
    q = np.arange(ch, dtype=np.uint32)[:, None, None, None]
    w = ar.philox4x32((xs[None], ys[None], zs[None], np.uint32(2) * q + np.uint32(1)), ar.key_words(key))
    u1 = ((w[0] >> np.uint32(8)) + np.uint32(1)).astype(F) * F(2.0 ** -24)
    u2 = (w[1] >> np.uint32(8)).astype(F) * F(2.0 ** -24)
    return u1, u2


def gaussian_noise(J, key, sigma_n):
    """clamp(J + sigma_n z).  logf and cosf are taken correctly rounded (float64, then float32): a device's differ from that by
    float32 ulps, which scaled by sigma_n moves the fp16 rounding of X by one step at most."""
    u1, u2 = noise_uniforms(J.shape[0], J.shape[1:], key)
    return clamp01(J + F(sigma_n) * ar.box_muller(u1, u2))


def sample(image, mask, weight, m, c, patch, num_classes, order, extra=None, sigma=5.0, keep_dark=False):
    """(X [ch][SZ][SY][SX], y [C][...], w [C][...]) float16 of one sample.  image uint8 [Z][Y][X][ch] (or [Z][Y][X]), mask and weight
    uint8 [Z][Y][X]; extra: the sample's parameters as loader.draw_extra returns them ('elastic': {key, alpha}, 'color_jitter':
    {brightness, contrast, contrast_first}, 'blur_or_noise': {kind: 'blur', sigma} or {kind: 'noise', key, sigma}; a missing entry =
    off; key: 64 bits); sigma: the elastic Gaussian's."""
    extra = extra or {}
    image = image[..., None] if image.ndim == 3 else image
    patch = tuple(patch)
    d = None
    if 'elastic' in extra:
        d = displacement(patch, extra['elastic']['key'], extra['elastic']['alpha'], ar.taps(sigma))
    x, byte, y, w = gather(image, mask, weight, coordinates(m, c, patch, d), num_classes, order, keep_dark)
    if 'color_jitter' in extra:
        cj = extra['color_jitter']
        x = jitter(x, byte, cj['brightness'], cj['contrast'], cj['contrast_first'])
    bn = extra.get('blur_or_noise')
    if bn is not None:
        x = gaussian_blur(x, bn['sigma']) if bn['kind'] == 'blur' else gaussian_noise(x, bn['key'], bn['sigma'])
    assert x.dtype == F
    return x.astype(np.float16), y, w
