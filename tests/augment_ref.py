"""The definition of the 2-D batch producer's three further transforms -- the reference's
ElasticTransform(NEAREST), ColorJitter(brightness, contrast) and RandomChoice([GaussianBlur(5), GaussianNoise()])
(interactive_unet/loader.py:115-123) on top of the flips / rotation / resized crop the device producer has today -- in numpy
float32.  A helper, not a test module.  There is no torchvision here, so this restatement IS the definition a device
implementation is held to: every multiply and add below is one float32 operation, rounded, in the order given (numpy never fuses a
multiply into an add), so fp16 outputs can be asked to equal these bit for bit (X on Gaussian-noise samples: up to a device's logf /
cosf, see `gaussian_noise`).  The device side is not in the tree; tests/test_augment_extra_cpu.py pins this file against Philox's
known answers and against oracle/loader_ref (whose helpers for the affine grid it shares: at 512 x 512 the geometry test holds the
output-size parameter and the evaluation at a displaced pixel together with the oracle, not the affine arithmetic independently).

  geometry   today's chain -- resized crop, rotation, flips: oracle/loader_ref.source_index -- with the output size (OH, OW) as a
             parameter and evaluated at a displaced output pixel (ey, ex) instead of (oy, ox)
  elastic    n_c[y][x] = 2u - 1, u = (word0 >> 8) 2^-24 of Philox4x32-10 at counter (x, y, c, 0) under the sample's elastic key;
             c = 0: x, c = 1: y.  K = int(8 sigma + 1) made odd; g_i = exp(-((i - (K-1)/2) / sigma)^2 / 2) / sum in float64, rounded to
             float32.  Horizontal pass then vertical pass, each acc = 0; acc += g_i * src[reflect(p + i - r)], i ascending, reflect
             without edge repeat.  d_c = blurred_c * float32(alpha / 2); ey = rint(oy + d_1), ex = rint(ox + d_0); a pixel displaced
             out of [0, OH) x [0, OW) is "outside": image byte 0, y = w = 0.
  jitter     on the gathered bytes G (all channels, outside = byte 0), L[v] = float32(v / 255): bright(x) = clamp(x b, 0, 1),
             contrast(x) = clamp(c x + (1 - c) m, 0, 1), m = float32(sum_v hist[v] float64(x_v) / N) summed in float64 in ascending
             v (x_v: the value entering the contrast step); brightness first or contrast first; the table T[v]
  blur       5 taps g (as above, sigma_b), w2[i][j] = float32(g_i g_j); out = sum_i sum_j w2[i][j] J[reflect(y+i-2)][reflect(x+j-2)]
             over J = T[G], i then j ascending, per channel
  noise      counter (x, y, channel, 1) under the sample's noise key: u1 = ((w0 >> 8) + 1) 2^-24, u2 = (w1 >> 8) 2^-24,
             z = sqrtf(-2 logf(u1)) cosf(6.2831855f u2); X = clamp(J + sigma_n z, 0, 1)
  X          = fp16 (nearest even) of the float32 result; y and w exactly as without the extras

Draw order the definition fixes for a loader (one torch generator; per sample): the four draws of interactive_unet.loader.draw_params
-- hflip, vflip, angle, crop box -- then, for each transform switched on, in this order: elastic: two 32-bit key words (one
randint(0, 2^32, (2,)), low word first); color_jitter: rand < 0.5 -> contrast first, brightness ~ U(0.75, 1.25), contrast ~ U(0.5,
2.0); blur_or_noise: randint(0, 2): 0 blur, then sigma_b ~ U(0.1, 2.0); 1 noise, then two 32-bit key words.  With no transform
switched on nothing more is drawn, so today's sequence stays what it is.
"""
import numpy as np

from oracle import loader_ref as lr

F = np.float32
LUT32 = (np.arange(256) / 255).astype(np.float32)                 # L[v]
LUT = LUT32.astype(np.float16)                                    # the producer's table: fp16(float32(v / 255))
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key):
    """Philox4x32-10.  counter: four uint32 arrays (broadcastable), key: (k0, k1) ints -> four uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(*[np.asarray(v) for v in counter])]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def key_words(key):
    """(k0, k1) of a 64-bit key: low word, high word."""
    return int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF


def taps(sigma, K=None):
    """The normalised Gaussian taps: float64, rounded to float32.  K: int(8 sigma + 1) made odd unless given."""
    if K is None:
        K = int(8 * sigma + 1)
        K += 1 - K % 2
    x = np.arange(K, dtype=np.float64) - (K - 1) / 2
    g = np.exp(-0.5 * (x / float(sigma)) ** 2)
    return (g / g.sum()).astype(np.float32)


def blur_pass(src, g, axis):
    """acc = 0; acc += g_i * src[reflect(p + i - r)] for i ascending, along `axis` of a float32 array."""
    r = len(g) // 2
    assert src.dtype == F and src.shape[axis] > r
    pad = np.pad(src, [(r, r) if a == axis else (0, 0) for a in range(src.ndim)], mode='reflect')
    n = src.shape[axis]
    acc = np.zeros_like(src)
    for i in range(len(g)):
        acc = acc + g[i] * np.take(pad, np.arange(i, i + n), axis=axis)
        assert acc.dtype == F
    return acc


def displaced(OH, OW, key, alpha, g):
    """(ey, ex, inside): the displaced output pixel of every output pixel (int64, clipped for indexing) and whether it lies inside."""
    xs, ys = np.arange(OW, dtype=np.uint32)[None, :], np.arange(OH, dtype=np.uint32)[:, None]
    d = []
    for c in (0, 1):
        w0 = philox4x32((xs, ys, np.uint32(c), np.uint32(0)), key_words(key))[0]
        u = (w0 >> np.uint32(8)).astype(F) * F(2.0 ** -24)
        n = F(2) * u - F(1)
        d.append(blur_pass(blur_pass(n, g, 1), g, 0) * F(alpha / 2))
    fy = np.rint(np.arange(OH, dtype=F)[:, None] + d[1])
    fx = np.rint(np.arange(OW, dtype=F)[None, :] + d[0])
    inside = (fy >= 0) & (fy <= OH - 1) & (fx >= 0) & (fx <= OW - 1)
    return np.where(inside, fy, 0).astype(np.int64), np.where(inside, fx, 0).astype(np.int64), inside


def source_index(H, W, hflip, vflip, angle, crop, out, ey=None, ex=None):
    """oracle/loader_ref.source_index for an (OH, OW) output, evaluated at output pixels (ey, ex) (default: every pixel's own
    position): the source (row, col) in the unflipped annotation, or -1 where the rotation samples outside."""
    OH, OW = out
    if ey is None:
        ey, ex = np.meshgrid(np.arange(OH), np.arange(OW), indexing='ij')
    i, j, h, w = crop
    CY = i + np.minimum(np.floor(ey.astype(F) * (F(h) / F(OH))).astype(np.int64), h - 1)          # interpolate(mode='nearest')
    CX = j + np.minimum(np.floor(ex.astype(F) * (F(w) / F(OW))).astype(np.int64), w - 1)
    kind = lr.rotation_kind(angle, H, W)
    ok = np.ones(CY.shape, bool)
    if kind == 1:
        ry, rx = CY, CX
    elif kind == 2:
        ry, rx = H - 1 - CY, W - 1 - CX
    elif kind == 3:
        ry, rx = CX, W - 1 - CY
    elif kind == 4:
        ry, rx = H - 1 - CX, CY
    else:
        xg, yg = [g.numpy() for g in lr.base_grids(W, H)]
        r = lr.rescaled_theta(angle, W, H).numpy()
        X, Y = xg[CX], yg[CY]
        gx = lr._fma(Y, r[1, 0], X * r[0, 0]) + r[2, 0]
        gy = lr._fma(Y, r[1, 1], X * r[0, 1]) + r[2, 1]
        ix = ((gx + F(1)) * F(W) - F(1)) / F(2)
        iy = ((gy + F(1)) * F(H) - F(1)) / F(2)
        rx, ry = np.rint(ix).astype(np.int64), np.rint(iy).astype(np.int64)
        ok = (rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)
    if vflip:
        ry = H - 1 - ry
    if hflip:
        rx = W - 1 - rx
    return np.where(ok, ry, -1), np.where(ok, rx, -1)


def clamp01(x):
    return np.minimum(np.maximum(x, F(0)), F(1))


def histogram_mean(byte, entering):
    """m: the exact mean of entering[v] (float32 [256]: what enters the contrast step for byte value v) over the bytes `byte`
    (uint8), from their histogram: float64 products summed in ascending v, divided by N, rounded to float32."""
    hist = np.bincount(byte.reshape(-1), minlength=256)
    acc = np.float64(0.0)
    for v in range(256):
        acc = acc + np.float64(int(hist[v])) * np.float64(entering[v])
    return F(acc / np.float64(byte.size))


def jitter_table(G, b, c, contrast_first):
    """T[v] float32 for the gathered bytes G (uint8, every channel of the sample)."""
    b, c = F(b), F(c)
    entering = LUT32 if contrast_first else clamp01(LUT32 * b)
    m = histogram_mean(G, entering)
    t = clamp01(c * entering + (F(1) - c) * m)
    return clamp01(t * b) if contrast_first else t


def gaussian_blur(J, sigma_b):
    """The 5 x 5 blur of J [ch][OH][OW] float32."""
    k = taps(sigma_b, 5)
    w2 = k[:, None] * k[None, :]
    assert w2.dtype == F
    OH, OW = J.shape[1:]
    pad = np.pad(J, ((0, 0), (2, 2), (2, 2)), mode='reflect')
    acc = np.zeros_like(J)
    for i in range(5):
        for j in range(5):
            acc = acc + w2[i, j] * pad[:, i:i + OH, j:j + OW]
    return acc


def box_muller(u1, u2):
    """z = sqrtf(-2 logf(u1)) cosf(6.2831855f u2), logf and cosf taken correctly rounded (float64, then float32)."""
    logf = np.log(u1.astype(np.float64)).astype(F)
    ang = F(6.2831855) * u2
    z = np.sqrt(F(-2) * logf) * np.cos(ang.astype(np.float64)).astype(F)
    assert z.dtype == F
    return z


def gaussian_noise(J, key, sigma_n):
    """clamp(J + sigma_n z).  logf and cosf are taken correctly rounded (float64, then float32): a device's differ from that by
    float32 ulps, which scaled by sigma_n moves the fp16 rounding of X by one step at most."""
    ch, OH, OW = J.shape
    xs, ys, cs = np.arange(OW, dtype=np.uint32)[None, None, :], np.arange(OH, dtype=np.uint32)[None, :, None], np.arange(ch, dtype=np.uint32)[:, None, None]
    w = philox4x32((xs, ys, cs, np.uint32(1)), key_words(key))
    u1 = ((w[0] >> np.uint32(8)) + np.uint32(1)).astype(F) * F(2.0 ** -24)
    u2 = (w[1] >> np.uint32(8)).astype(F) * F(2.0 ** -24)
    return clamp01(J + F(sigma_n) * box_muller(u1, u2))


def sample(image, mask, weight, params, extra=None, out=(512, 512), sigma=5.0, keep_dark=False):
    """(X [ch][OH][OW], y [C][OH][OW], w [C][OH][OW]) float16 of one sample.  image uint8 [H][W][ch] (or [H][W]), mask uint8
    [H][W][C], weight uint8 [H][W]; params = (hflip, vflip, angle, crop); extra: the sample's parameters, a dict with
    'elastic': {key, alpha}, 'color_jitter': {brightness, contrast, contrast_first}, 'blur_or_noise': {kind: 'blur', sigma} or
    {kind: 'noise', key, sigma} (a missing entry = off; key: 64 bits); sigma: the elastic Gaussian's."""
    extra = extra or {}
    image = image[:, :, None] if image.ndim == 2 else image
    H, W, ch = image.shape
    OH, OW = out
    ey = ex = inside = None
    if 'elastic' in extra:
        ey, ex, inside = displaced(OH, OW, extra['elastic']['key'], extra['elastic']['alpha'], taps(sigma))
    ry, rx = source_index(H, W, *params, out, ey, ex)
    ok = ry >= 0 if inside is None else (ry >= 0) & inside
    ry, rx = np.clip(ry, 0, None), np.clip(rx, 0, None)
    G = np.where(ok[None], np.moveaxis(image[ry, rx], -1, 0), 0).astype(np.uint8)
    lit = ok & ((image[ry, rx, 0] != 0) | bool(keep_dark))
    y = np.where(lit[None], np.moveaxis(LUT[mask[ry, rx]], -1, 0), LUT[0])
    w = np.stack([np.where(lit, LUT[weight[ry, rx]], LUT[0])] * mask.shape[2])
    T = LUT32
    if 'color_jitter' in extra:
        cj = extra['color_jitter']
        T = jitter_table(G, cj['brightness'], cj['contrast'], cj['contrast_first'])
    J = T[G]
    bn = extra.get('blur_or_noise')
    if bn is not None:
        J = gaussian_blur(J, bn['sigma']) if bn['kind'] == 'blur' else gaussian_noise(J, bn['key'], bn['sigma'])
    assert J.dtype == F
    return J.astype(np.float16), y, w
