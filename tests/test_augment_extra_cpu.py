"""The definition of the batch producer's three further transforms (tests/augment_ref.py), pinned without a
GPU: its Philox against the published known answers, its geometry against oracle/loader_ref at 512 x 512, neutral parameters as the
identity, the taps, the reflecting blur against an index-by-index loop, the contrast mean, the noise's range and moments, and the
elastic cases a device test will want (defaults: about a pixel; alpha = 400, sigma = 2: several pixels, across the border)."""
import numpy as np

from oracle import loader_ref as lr
from tests import augment_ref as ar

F = np.float32


def _annotation(rng, H, W, C, ch=1):
    image = rng.integers(1, 256, (H, W, ch), dtype=np.uint8)
    image[H // 3:H // 3 + 5, :, 0] = 0                                # a dark band in channel 0: mask and weight are zeroed there
    cls = rng.integers(0, C + 1, (H, W))
    mask = np.stack([(cls == k + 1) * 255 for k in range(C)], -1).astype(np.uint8)
    return image, mask, rng.integers(0, 256, (H, W), dtype=np.uint8)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def test_philox_known_answers():
    """Philox4x32-10's known-answer vectors (Random123's kat_vectors: zeros, all ones, the digits of pi)."""
    for counter, key, want in (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                               ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                               ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        got = ar.philox4x32([np.uint32(c) for c in counter], key)
        assert tuple(int(v) for v in got) == want, [hex(int(v)) for v in got]
    # vectorised over the counter, and the 64-bit key splits low word first
    got = ar.philox4x32((np.array([0, 0x243f6a88], np.uint32), np.array([0, 0x85a308d3], np.uint32), np.array([0, 0x13198a2e], np.uint32),
                         np.array([0, 0x03707344], np.uint32)), (0, 0))
    assert int(got[0][0]) == 0x6627e8d5 and got[0].dtype == np.uint32
    assert ar.key_words(0x299f31d0a4093822) == (0xa4093822, 0x299f31d0)


def test_geometry_with_extras_off_is_the_oracles_at_512():
    rng = np.random.default_rng(2)
    for (H, W), (hflip, vflip, angle) in (((300, 400), (True, False, 37.25)), ((256, 256), (False, True, 90.0)), ((611, 389), (True, True, 180.0))):
        image, mask, weight = _annotation(rng, H, W, 3, ch=2)
        crop = lr.resized_crop_params(H, W, lambda a, c: float(rng.uniform(a, c)), lambda n: int(rng.integers(n)))
        params = (hflip, vflip, angle, crop)
        for got, want in zip(ar.source_index(H, W, *params, (512, 512)), lr.source_index(H, W, *params)):
            assert np.array_equal(got, want), params
        got = ar.sample(image, mask, weight, params)
        want = lr.get_item(*lr.normalise(image, mask, weight), *params)
        for g, w, name in zip(got, want, ('image', 'mask', 'weight')):
            assert g.dtype == np.float16 and np.array_equal(_bits(g), _bits(w.numpy())), (params, name)


def test_neutral_parameters_are_the_identity():
    rng = np.random.default_rng(3)
    image, mask, weight = _annotation(rng, 64, 80, 2, ch=3)
    params = (True, False, -21.5, (3, 5, 50, 60))
    out = (45, 70)
    plain = ar.sample(image, mask, weight, params, None, out)
    assert plain[0].shape == (3,) + out and plain[1].shape == plain[2].shape == (2,) + out
    for extra in ({'elastic': {'key': 0x1234567890abcdef, 'alpha': 0.0}},
                  {'color_jitter': {'brightness': 1.0, 'contrast': 1.0, 'contrast_first': False}},
                  {'color_jitter': {'brightness': 1.0, 'contrast': 1.0, 'contrast_first': True}},
                  {'blur_or_noise': {'kind': 'noise', 'key': 77, 'sigma': 0.0}},
                  {'elastic': {'key': 5, 'alpha': 0.0}, 'color_jitter': {'brightness': 1.0, 'contrast': 1.0, 'contrast_first': True},
                   'blur_or_noise': {'kind': 'noise', 'key': 9, 'sigma': 0.0}}):
        got = ar.sample(image, mask, weight, params, extra, out)
        assert all(np.array_equal(_bits(g), _bits(p)) for g, p in zip(got, plain)), extra
    # and they are not the identity once switched on: the elastic map moves pixels of all three tensors, the others change grey values only
    moved = ar.sample(image, mask, weight, params, {'elastic': {'key': 5, 'alpha': 400.0}}, out, sigma=2.0)
    assert not np.array_equal(moved[1], plain[1]) and not np.array_equal(moved[0], plain[0]) and not np.array_equal(moved[2], plain[2])
    for extra in ({'color_jitter': {'brightness': 1.25, 'contrast': 2.0, 'contrast_first': False}}, {'blur_or_noise': {'kind': 'noise', 'key': 77, 'sigma': 0.1}},
                  {'blur_or_noise': {'kind': 'blur', 'sigma': 1.0}}):
        got = ar.sample(image, mask, weight, params, extra, out)
        assert not np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1]) and np.array_equal(got[2], plain[2])


def test_taps_sum_to_one():
    for sigma, K in ((5.0, 41), (2.0, 17), (0.1, 1), (1.3, 11)):
        g = ar.taps(sigma)
        assert g.dtype == np.float32 and len(g) == K and np.array_equal(g, g[::-1]) and g.argmax() == K // 2
        assert abs(float(g.astype(np.float64).sum()) - 1.0) <= K * 2.0 ** -25           # K roundings of at most half an ulp below 1
    for sigma in (0.1, 1.0, 2.0):
        assert len(ar.taps(sigma, 5)) == 5 and abs(float(ar.taps(sigma, 5).astype(np.float64).sum()) - 1.0) <= 5 * 2.0 ** -25


def test_blur_pass_is_the_reflecting_loop():
    """-1 -> 1, n -> n - 2, ascending taps, one rounding per multiply and per add: an index-by-index loop gives the same bits."""
    rng = np.random.default_rng(6)
    src = rng.random((7, 9), dtype=np.float32)
    g = ar.taps(1.0, 7)                                               # radius 3 on 7 x 9: both borders reflect into every row

    def reflect(p, n):
        p = -p if p < 0 else p
        return 2 * n - 2 - p if p >= n else p
    assert [reflect(p, 9) for p in (-3, -1, 0, 8, 9, 11)] == [3, 1, 0, 8, 7, 5]
    for axis in (0, 1):
        got = ar.blur_pass(src, g, axis)
        for y in range(7):
            for x in range(9):
                acc = F(0)
                for i in range(7):
                    v = src[reflect(y + i - 3, 7), x] if axis == 0 else src[y, reflect(x + i - 3, 9)]
                    acc = F(acc + F(g[i] * v))
                assert got[y, x] == acc, (axis, y, x)
    J = rng.random((2, 6, 5), dtype=np.float32)
    k = ar.taps(0.8, 5)
    got = ar.gaussian_blur(J, 0.8)
    for c, y, x in ((0, 0, 0), (1, 5, 4), (1, 2, 3), (0, 5, 0)):
        acc = F(0)
        for i in range(5):
            for j in range(5):
                acc = F(acc + F(F(k[i] * k[j]) * J[c, reflect(y + i - 2, 6), reflect(x + j - 2, 5)]))
        assert got[c, y, x] == acc, (c, y, x)


def test_jitter_table():
    rng = np.random.default_rng(7)
    G = rng.integers(0, 256, (2, 30, 40), dtype=np.uint8)
    # contrast 1: the mean drops out -- brightness alone, clamped at 1 (b = 1.25 saturates the bright bytes)
    T = ar.jitter_table(G, 1.25, 1.0, False)
    assert np.array_equal(T, np.minimum(ar.LUT32 * F(1.25), F(1))) and T[255] == 1 and (T == 1).sum() > 40
    # the mean is the exact one: a constant image has m = x_v, and contrast leaves the value where it is up to the blend's roundings
    for v in (3, 128, 250):
        T = ar.jitter_table(np.full((1, 8, 8), v, np.uint8), 1.0, 2.0, True)
        assert abs(float(T[v]) - float(ar.LUT32[v])) <= 2.0 ** -22
    # both corners, both orders: values stay in [0, 1], both clamps are hit, the order matters
    for corner in ((1.25, 2.0), (0.75, 0.5)):
        a, b = ar.jitter_table(G, *corner, False), ar.jitter_table(G, *corner, True)
        assert a.dtype == b.dtype == np.float32 and a.min() >= 0 and a.max() <= 1 and b.min() >= 0 and b.max() <= 1
        assert np.all(np.diff(a) >= 0) and np.all(np.diff(b) >= 0) and not np.array_equal(a, b)
    hi = ar.jitter_table(G, 1.25, 2.0, False)
    assert hi[0] == 0 and hi[255] == 1 and (hi == 0).sum() > 10 and (hi == 1).sum() > 10
    # a contrast below 1 lifts byte 0 -- "outside" pixels go through the table like any other byte 0
    assert ar.jitter_table(G, 0.75, 0.5, False)[0] > 0.1


def test_noise_and_elastic_cases():
    J = np.full((2, 64, 96), 0.5, np.float32)
    z = (ar.gaussian_noise(J, 0xfedcba9876543210, 0.1).astype(np.float64) - 0.5) / 0.1          # |z| < 5: no clamp at J = 0.5
    assert np.isfinite(z).all() and abs(z.mean()) < 0.05 and abs(z.std() - 1.0) < 0.05 and np.abs(z).max() < 5.8
    assert not np.array_equal(z[0], z[1])                             # the channel is part of the counter
    lo = ar.gaussian_noise(np.zeros((1, 16, 16), np.float32), 3, 0.1)
    assert lo.min() == 0 and lo.max() > 0                             # clamped at 0
    OH, OW = 45, 70
    oy, ox = np.arange(OH)[:, None], np.arange(OW)[None, :]
    ey, ex, inside = ar.displaced(OH, OW, 0x0123456789abcdef, 50.0, ar.taps(5.0))
    d = np.maximum(np.abs(ey - oy), np.abs(ex - ox))[inside]
    assert 1 <= d.max() <= 6 and inside.mean() > 0.9                  # the defaults: about a pixel
    ey, ex, inside = ar.displaced(OH, OW, 0x0123456789abcdef, 400.0, ar.taps(2.0))
    d = np.maximum(np.abs(ey - oy), np.abs(ex - ox))[inside]
    assert d.max() >= 8 and 0.2 < inside.mean() < 0.95               # several pixels, and across the border
    assert ey.min() >= 0 and ey.max() <= OH - 1 and ex.min() >= 0 and ex.max() <= OW - 1
