"""The 3-D patch producer's three further transforms without a GPU: the definition tests/patch_augment_ref.py
pinned against patch_ref (neutral parameters), against index-by-index loops (the smoothing passes, the displaced coordinates, the
separable blur) and against its own statements (jitter clamps, the histogram byte, the noise's moments, the elastic magnitudes);
then the host side of interactive_unet.loader -- draw order, the untouched path with everything off, the descriptor mirror, the
keywords -- and every refusal of iunet_patch_batch_extra, which comes before any launch."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import augment_ref as ar
from tests import patch_augment_ref as par
from tests import patch_ref as pr

F = np.float32
SHAPE = (20, 30, 40)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _reflect(p, n):
    p = -p if p < 0 else p
    return 2 * n - 2 - p if p >= n else p


@pytest.fixture(scope='module')
def volume():
    image, mask, weight = pr.make_volume(np.random.default_rng(31), SHAPE, ch=2, classes=3, dark=True)
    return image, mask, weight[..., 0].copy()


M = pr.rotation((1, 2, 3), 37.0, 0.8)
CENTRE = [2.5, 26.25, 36.0]


def test_neutral_parameters_are_patch_ref(volume):
    image, mask, weight = volume
    patch = (6, 10, 12)
    assert np.array_equal(par.coordinates(M, CENTRE, patch), pr.coordinates(M, CENTRE, patch))
    assert np.array_equal(F(np.arange(256)) / F(255), par.LUT32)        # one float32 division is float32(v / 255)
    neutral = ({'elastic': {'key': 0x1234567890abcdef, 'alpha': 0.0}},
               {'color_jitter': {'brightness': 1.0, 'contrast': 1.0, 'contrast_first': False}},
               {'color_jitter': {'brightness': 1.0, 'contrast': 1.0, 'contrast_first': True}},
               {'blur_or_noise': {'kind': 'noise', 'key': 77, 'sigma': 0.0}},
               {'elastic': {'key': 5, 'alpha': 0.0}, 'color_jitter': {'brightness': 1.0, 'contrast': 1.0, 'contrast_first': True},
                'blur_or_noise': {'kind': 'noise', 'key': 9, 'sigma': 0.0}})
    for order in (0, 1):
        plain = pr.patch(image, mask, weight, M, CENTRE, patch, 3, order)
        assert (plain[0] == 0).any() and (plain[2] > 0).any()          # partly outside the volume
        for extra in (None, {}) + neutral:
            got = par.sample(image, mask, weight, M, CENTRE, patch, 3, order, extra, sigma=1.0)
            assert all(g.dtype == np.float16 and np.array_equal(_bits(g), _bits(p)) for g, p in zip(got, plain)), (order, extra)
        # ... and not once switched on: elastic moves all three tensors, the others change grey values only
        moved = par.sample(image, mask, weight, M, CENTRE, patch, 3, order, {'elastic': {'key': 5, 'alpha': 400.0}}, sigma=1.0)
        assert all(not np.array_equal(a, b) for a, b in zip(moved, plain))
        for extra in ({'color_jitter': {'brightness': 1.25, 'contrast': 2.0, 'contrast_first': False}},
                      {'blur_or_noise': {'kind': 'noise', 'key': 77, 'sigma': 0.1}}, {'blur_or_noise': {'kind': 'blur', 'sigma': 1.0}}):
            got = par.sample(image, mask, weight, M, CENTRE, patch, 3, order, extra)
            assert not np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1]) and np.array_equal(got[2], plain[2])


def test_each_smoothing_pass_is_the_reflecting_loop():
    patch = (5, 6, 7)
    g = ar.taps(1.0, 9)                                                 # radius 4: both borders reflect into every voxel
    n = par.noise_field(patch, 0x0123456789abcdef, 1)
    assert n.dtype == F and n.shape == patch and n.min() >= -1 and n.max() < 1
    # the counter: (ox, oy, oz, 2 c), word 0
    w0 = int(ar.philox4x32([np.uint32(v) for v in (6, 4, 3, 2)], ar.key_words(0x0123456789abcdef))[0])
    assert n[3, 4, 6] == F(2) * (F(w0 >> 8) * F(2.0 ** -24)) - F(1)
    assert not np.array_equal(n, par.noise_field(patch, 0x0123456789abcdef, 0))
    stages = [n, ar.blur_pass(n, g, 2), None, None]
    stages[2] = ar.blur_pass(stages[1], g, 1)
    stages[3] = ar.blur_pass(stages[2], g, 0)
    assert np.array_equal(par.smooth(n, g), stages[3])                  # x, then y, then z
    for k, axis in enumerate((2, 1, 0)):
        src, got = stages[k], stages[k + 1]
        for z in range(patch[0]):
            for y in range(patch[1]):
                for x in range(patch[2]):
                    acc = F(0)
                    for i in range(9):
                        idx = [z, y, x]
                        idx[axis] = _reflect(idx[axis] + i - 4, patch[axis])
                        acc = F(acc + F(g[i] * src[tuple(idx)]))
                    assert got[z, y, x] == acc, (axis, z, y, x)


def test_displaced_coordinates_are_the_hand_written_loop():
    patch = (6, 7, 9)
    g = ar.taps(0.6)                                                    # K = 5, radius 2
    assert len(g) == 5
    d = par.displacement(patch, 42, 7.0, g)
    assert d.dtype == F and d.shape == (3,) + patch and np.abs(d).max() > 0.5
    for c in range(3):
        assert np.array_equal(d[c], par.smooth(par.noise_field(patch, 42, c), g) * F(3.5))
    m, c = np.asarray(M, dtype=F), np.asarray(CENTRE, dtype=F)
    p = par.coordinates(M, CENTRE, patch, d)
    for oz in range(6):
        for oy in range(7):
            for ox in range(9):
                t = [F(F(o) - F((S - 1) / 2)) for o, S in zip((oz, oy, ox), patch)]
                t = [F(t[j] + d[j, oz, oy, ox]) for j in range(3)]      # not rounded to a voxel: one add per axis
                for a in range(3):
                    want = F(F(F(F(m[a, 0] * t[0]) + F(m[a, 1] * t[1])) + F(m[a, 2] * t[2])) + c[a])
                    assert p[a, oz, oy, ox] == want, (a, oz, oy, ox)


def test_jitter_clamps_in_both_orders(volume):
    image, mask, weight = volume
    patch = (6, 10, 12)
    for order in (0, 1):
        x, byte, _, _ = par.gather(image, mask, weight, par.coordinates(M, CENTRE, patch), 3, order)
        assert x.dtype == F and byte.dtype == np.uint8 and x.shape == byte.shape == (2,) + patch and x.min() == 0 and x.max() <= 1
        for cf in (False, True):
            hi = par.jitter(x, byte, 1.25, 2.0, cf)
            assert hi.dtype == F and hi.min() == 0 and hi.max() == 1 and (hi == 0).sum() > 10 and (hi == 1).sum() > 10
            lo = par.jitter(x, byte, 0.75, 0.5, cf)
            assert lo.min() > 0.05 and lo.max() < 0.9                   # a contrast below 1 lifts the zeros outside the volume
        assert not np.array_equal(par.jitter(x, byte, 1.25, 2.0, False), par.jitter(x, byte, 1.25, 2.0, True))
        # contrast 1: the mean drops out (up to x + 0) -- brightness alone, clamped at 1
        assert np.array_equal(par.jitter(x, byte, 1.25, 1.0, False), np.minimum(x * F(1.25), F(1)))
        # the mean is the histogram's: float64 products summed in ascending v
        hist = np.bincount(byte.reshape(-1), minlength=256)
        for cf in (False, True):
            E = par.LUT32 if cf else par.clamp01(par.LUT32 * F(0.8))
            acc = 0.0
            for v in range(256):
                acc += float(hist[v]) * float(E[v])
            assert par.contrast_mean(byte, 0.8, cf) == F(acc / byte.size)
    # a constant volume: m = E[v], and contrast leaves the value where it is up to the blend's roundings
    const = np.full(SHAPE + (1,), 77, np.uint8)
    inside = [10.0, 15.0, 20.0]
    for order in (0, 1):
        x, byte, _, _ = par.gather(const, mask, weight, par.coordinates(np.eye(3), inside, (4, 4, 4)), 3, order)
        assert (byte == 77).all() and np.abs(par.jitter(x, byte, 1.0, 2.0, True) - par.LUT32[77]).max() <= 2.0 ** -22


def test_order_1_histogram_byte_is_rint(volume):
    image, mask, weight = volume
    patch = (6, 10, 12)
    p = par.coordinates(M, CENTRE, patch)
    x, byte, _, _ = par.gather(image, mask, weight, p, 3, 1)
    v = x * F(255)                                                      # not the definition's v, but within an ulp of it
    near_tie = np.abs(v - np.floor(v) - 0.5) < 1e-3
    assert np.array_equal(byte[~near_tie], np.rint(v[~near_tie]).astype(np.uint8))
    assert np.array_equal(pr.patch(image, mask, weight, M, CENTRE, patch, 3, 1)[0], x.astype(np.float16))
    # exact ties go to even: at the midpoint between two voxels along x the value is (a + b) / 2
    img = np.zeros((4, 4, 4, 1), np.uint8)
    img[..., 0] = np.array([0, 1, 4, 9], np.uint8)                      # along x: midpoints 0.5, 2.5, 6.5
    k, wt = np.zeros((4, 4, 4), np.uint8), np.full((4, 4, 4), 255, np.uint8)
    _, byte, _, _ = par.gather(img, k, wt, par.coordinates(np.eye(3), [1.0, 1.0, 1.5], (1, 1, 3)), 2, 1)
    assert byte.reshape(-1).tolist() == [0, 2, 6]
    _, byte0, _, _ = par.gather(img, k, wt, par.coordinates(np.eye(3), [1.0, 1.0, 1.0], (1, 1, 3)), 2, 0)
    assert byte0.reshape(-1).tolist() == [0, 1, 4]                      # order 0: the gathered byte


def test_separable_blur_is_the_loop():
    rng = np.random.default_rng(6)
    J = rng.random((2, 4, 5, 6), dtype=np.float32)
    for sigma in (0.1, 0.148, 0.8, 2.0):
        k = ar.taps(sigma, 5)
        got = par.gaussian_blur(J, sigma)
        assert got.dtype == F

        def line(src, axis):
            out = np.zeros_like(src)
            for idx in np.ndindex(src.shape):
                acc = F(0)
                for i in range(5):
                    j = list(idx)
                    j[axis] = _reflect(j[axis] + i - 2, src.shape[axis])
                    acc = F(acc + F(k[i] * src[tuple(j)]))
                out[idx] = acc
            return out
        assert np.array_equal(got, line(line(line(J, 3), 2), 1)), sigma
    k = ar.taps(0.148, 5)
    assert 0 < k[0] < np.finfo(np.float32).tiny and k[2] == 1           # small sigma_b: the outer taps are float32 denormals, and kept
    assert ar.taps(0.1, 5)[0] == 0 and ar.taps(0.1, 5)[1] > 0           # at the range's end 0.1 they are below even those
    with pytest.raises(AssertionError):
        par.gaussian_blur(J[:, :2], 1.0)                                # every extent must exceed 2


def test_noise_moments():
    J = np.full((2, 16, 24, 32), 0.5, np.float32)
    z = (par.gaussian_noise(J, 0xfedcba9876543210, 0.1).astype(np.float64) - 0.5) / 0.1         # |z| < 5: no clamp at J = 0.5
    assert np.isfinite(z).all() and abs(z.mean()) < 0.05 and abs(z.std() - 1.0) < 0.05 and np.abs(z).max() < 5.8
    assert not np.array_equal(z[0], z[1])                               # the channel is part of the counter
    u1, u2 = par.noise_uniforms(2, (16, 24, 32), 0xfedcba9876543210)
    w = ar.philox4x32([np.uint32(v) for v in (31, 5, 7, 3)], ar.key_words(0xfedcba9876543210))      # (ox, oy, oz, 2 q + 1), q = 1
    assert u1[1, 7, 5, 31] == F((int(w[0]) >> 8) + 1) * F(2.0 ** -24) and u2[1, 7, 5, 31] == F(int(w[1]) >> 8) * F(2.0 ** -24)
    assert u1.min() > 0 and u1.max() <= 1 and u2.min() >= 0 and u2.max() < 1
    lo = par.gaussian_noise(np.zeros((1, 8, 8, 8), np.float32), 3, 0.1)
    assert lo.min() == 0 and lo.max() > 0                               # clamped at 0
    # the elastic fields (even counter words) and the noise (odd ones) never share a counter
    assert not np.array_equal(par.noise_field((16, 24, 32), 5, 0), F(2) * par.noise_uniforms(1, (16, 24, 32), 5)[1][0] - F(1))


def test_elastic_magnitudes():
    """The defaults (alpha 50, sigma 5) move a voxel by less than one -- the third smoothing pass shrinks the field below the 2-D
    one's: about half a voxel RMS, by the variance of uniform noise under three sigma = 5 passes (1 / 3) (sum g^2)^3 -- while alpha
    400 with sigma 2 moves voxels by several."""
    patch = (44, 42, 48)
    g = ar.taps(5.0)
    d = par.displacement(patch, 0x0123456789abcdef, 50.0, g)
    expected = 25.0 * np.sqrt(float((g.astype(np.float64) ** 2).sum()) ** 3 / 3.0)
    rms = float(np.sqrt((d.astype(np.float64) ** 2).mean()))
    assert 0.15 < expected < 0.5 and 0.5 * expected < rms < 2.0 * expected and np.abs(d).max() < 1.0, (expected, rms)
    big = par.displacement((24, 22, 26), 0x0123456789abcdef, 400.0, ar.taps(2.0))
    assert np.abs(big).max() > 4.0 and float(np.sqrt((big.astype(np.float64) ** 2).mean())) > 1.5


# ---- the host side -----------------------------------------------------------------------------------------------------------------
def _cpu_dataset(volume, **kw):
    from interactive_unet import loader
    image, mask, weight = volume
    vols = loader.volume_annotations_from_arrays([(image, mask, weight), (image[:15], mask[:15], weight[:15])], device='cpu')
    return loader.VolumeDataset(vols, 3, patch_size=(6, 10, 12), count=4, **kw)


def _spy(monkeypatch):
    """Record nv.call instead of launching: (name, args) per call.  The library's host-only answers stay real."""
    from interactive_unet import _native as nv, loader
    if not os.path.isfile(nv.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    calls = []
    monkeypatch.setattr(nv, 'call', lambda name, *args: calls.append((name, args)))
    monkeypatch.setattr(nv, 'stream', lambda: None)
    monkeypatch.setattr(loader.torch.cuda, 'device', lambda dev: contextlib.nullcontext())
    return calls


def test_draw_order_is_draw_then_draw_extra(volume, monkeypatch):
    from interactive_unet import loader
    calls = _spy(monkeypatch)
    on = dict(elastic=True, color_jitter=True, blur_or_noise=True, elastic_alpha=33.0, noise_sigma=0.2)
    ds = _cpu_dataset(volume, generator=torch.Generator().manual_seed(5), **on)
    seen = []
    real = loader._fill_patch_extra
    monkeypatch.setattr(loader, '_fill_patch_extra', lambda d, e: seen.append(e) or real(d, e))
    ds.batch([0, 1, 2])
    # the same seed, the torch calls written out: per sample the volume index and draw_patch_params, then the three transforms' draws
    g = torch.Generator().manual_seed(5)
    kinds = set()
    for k in range(3):
        vi = torch.randint(0, 2, (1,), generator=g).item()
        loader.draw_patch_params(tuple(ds.volumes[vi][1].shape), ds.patch, ds.candidates[vi], g)
        lo, hi = torch.randint(0, 2 ** 32, (2,), generator=g).tolist()
        want = {'elastic': {'key': lo | hi << 32, 'alpha': 33.0}}
        cf = bool(torch.rand(1, generator=g).item() < 0.5)
        b = torch.empty(1).uniform_(0.75, 1.25, generator=g).item()
        c = torch.empty(1).uniform_(0.5, 2.0, generator=g).item()
        want['color_jitter'] = {'brightness': b, 'contrast': c, 'contrast_first': cf}
        if torch.randint(0, 2, (1,), generator=g).item() == 0:
            want['blur_or_noise'] = {'kind': 'blur', 'sigma': torch.empty(1).uniform_(0.1, 2.0, generator=g).item()}
        else:
            lo, hi = torch.randint(0, 2 ** 32, (2,), generator=g).tolist()
            want['blur_or_noise'] = {'kind': 'noise', 'key': lo | hi << 32, 'sigma': 0.2}
        kinds.add(want['blur_or_noise']['kind'])
        assert seen[k] == want, k
    assert torch.equal(ds.generator.get_state(), g.get_state())         # nothing else was drawn
    assert [name for name, _ in calls] == ['iunet_patch_batch_extra']
    args = calls[0][1]
    use = args[2]
    assert use & 3 == 3 and use & 12 == (4 if kinds == {'blur'} else 8 if kinds == {'noise'} else 12)
    assert tuple(args[3:10]) == (3, 2, 3, 6, 10, 12, 1)                # B, ch, C, patch, order
    assert args[12] == 41 and args[14] >= loader.nv.lib().iunet_patch_extra_ws_bytes(3, 2, 6, 10, 12) > 0   # K of sigma 5; the workspace
    # imposed parameters draw nothing; a batch-size mismatch is refused
    state = ds.generator.get_state()
    ds.batch([0], params=[(0, [float(v) for v in np.eye(3).reshape(-1)], [5.0, 5.0, 5.0])], extra=[{}])
    assert torch.equal(ds.generator.get_state(), state) and calls[-1][0] == 'iunet_patch_batch_extra' and calls[-1][1][2] == 0
    with pytest.raises(ValueError, match='2 entries for a batch of 1'):
        ds.batch([0], extra=[{}, {}])
    with pytest.raises(ValueError, match="'blur' or 'noise'"):
        ds.batch([0], extra=[{'blur_or_noise': {'kind': 'median'}}])


def test_everything_off_is_todays_call_and_todays_draws(volume, monkeypatch):
    from interactive_unet import loader
    calls = _spy(monkeypatch)
    ds = _cpu_dataset(volume, generator=torch.Generator().manual_seed(9))
    assert not (ds.elastic or ds.color_jitter or ds.blur_or_noise) and (ds.elastic_alpha, ds.elastic_sigma, ds.noise_sigma) == (50.0, 5.0, 0.1)
    out = ds.batch([0, 1, 2])
    assert [t.shape for t in out] == [(3, 2, 6, 10, 12), (3, 3, 6, 10, 12), (3, 3, 6, 10, 12)] and out[0].dtype == torch.float16
    assert [name for name, _ in calls] == ['iunet_patch_batch'] and len(calls[0][1]) == 13
    twin = _cpu_dataset(volume, generator=torch.Generator().manual_seed(9))
    for _ in range(3):
        twin.draw()                                                     # today's sequence: three draw() calls and nothing else
    assert torch.equal(ds.generator.get_state(), twin.generator.get_state())


def test_descriptor_mirror_and_keywords(volume):
    from interactive_unet import _native as nv, loader
    if not os.path.isfile(nv.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    D = loader.PatchExtraDesc
    assert nv.lib().iunet_patch_extra_desc_bytes() == ctypes.sizeof(D) == 64
    assert [(name, getattr(D, name).offset) for name, _ in D._fields_] == [
        ('flags', 0), ('kind', 4), ('ekey', 8), ('a2', 16), ('brightness', 20), ('contrast', 24), ('contrast_first', 28), ('taps', 32),
        ('nkey', 52), ('sigma_n', 60)]
    assert ctypes.sizeof(loader.PatchDesc) % 8 == 0                     # the two arrays go up in one copy: the second stays aligned
    d = D()
    use = loader._fill_patch_extra(d, {'elastic': {'key': 0x299f31d0a4093822, 'alpha': 50.0},
                                       'color_jitter': {'brightness': 1.1, 'contrast': 0.7, 'contrast_first': True},
                                       'blur_or_noise': {'kind': 'blur', 'sigma': 0.148}})
    assert use == 7 and d.flags == 3 and d.kind == 1 and (d.ekey[0], d.ekey[1]) == (0xa4093822, 0x299f31d0) and d.a2 == 25.0
    assert (d.brightness, d.contrast, d.contrast_first) == (F(1.1), F(0.7), 1)
    assert np.array_equal(np.array(d.taps[:], dtype=F), ar.taps(0.148, 5)) and d.taps[0] > 0       # the denormal taps survive the mirror
    d = D()
    assert loader._fill_patch_extra(d, {'blur_or_noise': {'kind': 'noise', 'key': 3 << 32 | 7, 'sigma': 0.1}}) == 8
    assert d.flags == 0 and d.kind == 2 and (d.nkey[0], d.nkey[1]) == (7, 3) and d.sigma_n == F(0.1)
    assert np.array_equal(loader.gaussian_taps(5.0), ar.taps(5.0)) and np.array_equal(loader.gaussian_taps(1.3, 5), ar.taps(1.3, 5))
    # the keywords, through get_volume_loader; augment=False with one of them is refused
    image, mask, weight = volume
    vols = loader.volume_annotations_from_arrays([(image, mask, weight)], device='cpu')
    ld = loader.get_volume_loader('train', num_classes=3, batch_size=2, patch_size=8, count=4, volumes=vols, generator=torch.Generator().manual_seed(1),
                                  elastic=True, blur_or_noise=True, elastic_alpha=20.0, elastic_sigma=2.0, noise_sigma=0.05)
    ds = ld.dataset
    assert (ds.elastic, ds.color_jitter, ds.blur_or_noise, ds.elastic_alpha, ds.elastic_sigma, ds.noise_sigma) == (True, False, True, 20.0, 2.0, 0.05)
    plain = loader.get_volume_loader('val', num_classes=3, patch_size=8, count=4, volumes=vols, augment=False).dataset
    assert not (plain.elastic or plain.color_jitter or plain.blur_or_noise) and plain.weight_channel == 1
    for kw in (dict(elastic=True), dict(color_jitter=True), dict(blur_or_noise=True)):
        with pytest.raises(ValueError, match='augment=True'):
            loader.get_volume_loader('val', num_classes=3, patch_size=8, count=4, volumes=vols, augment=False, **kw)
        with pytest.raises(ValueError, match='augment=True'):
            loader.VolumeDataset(vols, 3, patch_size=8, count=4, augment=False, **kw)
    with pytest.raises(ValueError, match='augment=True'):
        plain.batch([0], extra=[{}])


def test_patch_batch_extra_refuses_bad_arguments_before_any_launch():
    from interactive_unet import _native as nv
    if not os.path.isfile(nv.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    l = nv.lib()
    need = l.iunet_patch_extra_ws_bytes(2, 1, 8, 8, 8)
    assert need >= 2 * 2 * 3 * 512 * 4 + 2 * 512 * 4 + 2 * 1024 + 8
    assert l.iunet_patch_extra_ws_bytes(2, 3, 8, 8, 8) > need
    for bad in ((0, 1, 8, 8, 8), (2, 0, 8, 8, 8), (2, 5, 8, 8, 8), (2, 1, 0, 8, 8), (2, 1, 8, -1, 8), (2, 1, 8, 8, 0), (8192, 1, 8, 8, 8)):
        assert l.iunet_patch_extra_ws_bytes(*bad) < 0 and b'patch_extra_ws_bytes' in l.iunet_last_error(), bad
    buf = (ctypes.c_int * 64)()
    good = dict(descs=buf, extras=buf, use=15, B=2, ch=1, C=2, SZ=8, SY=8, SX=8, order=1, lut=buf, taps=buf, K=5, ws=buf, ws_bytes=need, X=buf,
                y=buf, w=buf, stream=None)
    cases = [(dict(descs=None), b'null'), (dict(extras=None), b'null'), (dict(lut=None), b'null'), (dict(ws=None), b'null'),
             (dict(X=None), b'null'), (dict(y=None), b'null'), (dict(w=None), b'null'),
             # every range iunet_patch_batch refuses
             (dict(B=0), b'B 0'), (dict(ch=0), b'channels 0'), (dict(ch=5), b'channels 5'), (dict(C=0), b'classes 0'), (dict(C=17), b'classes 17'),
             (dict(SZ=0), b'patch 0 x'), (dict(SY=-1), b'x -1 x'), (dict(SX=0), b'x 0'), (dict(order=2), b'order 2'), (dict(order=-1), b'order -1'),
             (dict(B=8192, SZ=8), b'grid limit'),
             (dict(use=16), b'use 16'), (dict(use=-1), b'use -1'),
             (dict(ws_bytes=need - 1), b'workspace'), (dict(ws_bytes=0), b'workspace'),
             # elastic: the taps
             (dict(taps=None), b'without taps'), (dict(K=4), b'4 elastic taps'), (dict(K=0), b'0 elastic taps'), (dict(K=-3), b'-3 elastic taps'),
             (dict(K=131), b'131 elastic taps'), (dict(K=17), b'radius 8'), (dict(K=17, SX=20, SY=20, ws_bytes=1 << 40), b'radius 8'),
             (dict(K=17, SZ=20, SX=20, ws_bytes=1 << 40), b'radius 8'),
             # blur: radius 2
             (dict(use=4, SZ=2), b'radius 2'), (dict(use=6, SY=2), b'radius 2'), (dict(use=12, SX=1), b'radius 2')]
    for change, word in cases:
        rc = l.iunet_patch_batch_extra(*{**good, **change}.values())
        assert rc < 0 and b'patch_batch_extra' in l.iunet_last_error() and word in l.iunet_last_error(), (change, l.iunet_last_error())
