"""The 3-D patch producer's three further transforms on the device (iunet_patch_batch_extra) against their
definition, tests/patch_augment_ref.py, with imposed parameters: y, w and X bit for bit; X on Gaussian-noise samples within one fp16
step and different on at most 0.2 % of the sample's voxels (section 17's gate: the device's logf / cosf against correctly rounded
ones).  Volumes are 20 x 30 x 40, several patches reach outside them; the patch shapes are the smallest that reach every branch:
(6, 10, 70) -- one extent barely above the Gaussian's radius, a row longer than one block --, (24, 22, 26) -- no multiple of any
tile --, (4, 5, 150) -- two blocks of the x pass along a row, an odd number of rows, inside its volume along x --, and one (44, 42, 48) at the default sigma 5,
whose radius 20 needs it."""
import numpy as np
import pytest
import torch

from tests import augment_ref as ar
from tests import patch_augment_ref as par
from tests import patch_ref as pr

pytestmark = pytest.mark.gpu

SHAPE = (20, 30, 40)
NOISE_SHARE = 0.002
ELASTIC = {'elastic': {'key': 0x0123456789abcdef, 'alpha': 50.0}}
JITTER = {'color_jitter': {'brightness': 1.1, 'contrast': 1.6, 'contrast_first': False}}
BLUR = {'blur_or_noise': {'kind': 'blur', 'sigma': 1.0}}
NOISE = {'blur_or_noise': {'kind': 'noise', 'key': 0xfedcba9876543210, 'sigma': 0.1}}
ALL_BLUR = {'elastic': {'key': 77, 'alpha': 50.0}, 'color_jitter': {'brightness': 0.8, 'contrast': 0.6, 'contrast_first': True},
            'blur_or_noise': {'kind': 'blur', 'sigma': 1.7}}
ALL_NOISE = {'elastic': {'key': 1 << 63 | 5, 'alpha': 50.0}, 'color_jitter': {'brightness': 1.2, 'contrast': 1.9, 'contrast_first': False},
             'blur_or_noise': {'kind': 'noise', 'key': 3, 'sigma': 0.1}}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _flat(M):
    return [float(v) for v in np.asarray(M).reshape(-1)]


_cache = {}


def _setup(ch, C):
    """(numpy volumes, resident volumes): two 20 x 30 x 40 volumes, the second with zeros in the image (dark=True) and a slab where
    image channel 0 is zero; made once per (ch, C)."""
    if (ch, C) not in _cache:
        from interactive_unet import loader
        rng = np.random.default_rng(50 + ch)
        vols = []
        for dark in (False, True):
            image, mask, weight = pr.make_volume(rng, SHAPE, ch=ch, classes=C, dark=dark)
            if dark:
                image[:, 9:13, :, 0] = 0
            vols.append((image, mask, weight))
        _cache[ch, C] = (vols, loader.volume_annotations_from_arrays(vols))
    return _cache[ch, C]


def _dataset(ch, C, patch, order, sigma=5.0, keep_dark=False, **kw):
    from interactive_unet import loader
    return loader.VolumeDataset(_setup(ch, C)[1], C, patch_size=patch, count=4, order=order, elastic_sigma=sigma, keep_dark=keep_dark, **kw)


def _params(patch):
    """Four samples: rotated and scaled, partly outside; the identity at a half-integer centre in the dark volume (an odd extent: every
    coordinate of that axis is an exact .5 tie); a rotation about another axis reaching across a corner; a signed permutation."""
    return [(0, _flat(pr.rotation((1, 2, 3), 37.0, 0.6)), [8.0, 17.0, 21.5]),
            (1, _flat(np.eye(3)), [9.5, 14.5, 19.5]),
            (1, _flat(pr.rotation((3, 1, 2), 61.0, 0.45)), [3.0, 24.25, 33.0]),
            (0, _flat(pr.signed_permutations()[13] * 0.5), [10.0, 12.5, 20.0])]


LONG = (4, 5, 150)


def _long_params():
    """Four samples for the LONG patch whose whole x extent lies inside its volume, so that every column shows the displacement:
    patch x runs along source x at 0.25 voxels a step (150 x 0.25 = 37.5 of the 40), backwards on one; z and y at scale 1 or 0.5,
    flipped on two; the third in the dark volume, beside its slab."""
    return [(0, _flat(np.diag([1.0, 1.0, 0.25])), [9.5, 14.0, 19.5]),
            (0, _flat(np.diag([-1.0, 0.5, -0.25])), [10.0, 20.5, 19.75]),
            (1, _flat(np.diag([0.5, 1.0, 0.25])), [6.0, 20.0, 19.5]),
            (0, _flat(np.diag([1.0, -1.0, 0.25])), [12.5, 8.0, 20.0])]


def _compare(got, want, extra, where):
    """One sample: y, w, X bit-equal; a noise sample's X within one fp16 step, differing on at most NOISE_SHARE of its voxels."""
    (X, y, w), (rX, ry, rw) = got, want
    assert X.dtype == y.dtype == w.dtype == np.float16 and X.shape == rX.shape and y.shape == ry.shape and w.shape == rw.shape, where
    assert np.array_equal(_bits(y), _bits(ry)), (where, 'mask', int((_bits(y) != _bits(ry)).sum()))
    assert np.array_equal(_bits(w), _bits(rw)), (where, 'weight', int((_bits(w) != _bits(rw)).sum()))
    if (extra or {}).get('blur_or_noise', {}).get('kind') == 'noise':
        step = np.abs(_bits(X).astype(np.int32) - _bits(rX).astype(np.int32))          # X >= 0: fp16 bits are ordered
        share = float((step != 0).mean())
        print(f'{where}: noise sample, {int((step != 0).sum())} of {step.size} voxels differ from the definition ({100 * share:.4f} %), '
              f'largest difference {int(step.max())} fp16 step(s)')
        assert step.max() <= 1 and share <= NOISE_SHARE, (where, int(step.max()), share)
    else:
        bad = _bits(X) != _bits(rX)
        assert not bad.any(), (where, 'image', int(bad.sum()), np.argwhere(bad)[:5].tolist())


def _check(ch, C, patch, order, params, extras, sigma=5.0, keep_dark=False, where=''):
    vols = _setup(ch, C)[0]
    ds = _dataset(ch, C, patch, order, sigma, keep_dark)
    got = [t.cpu().numpy() for t in ds.batch(list(range(len(params))), params=params, extra=extras)]
    refs = []
    for b, (vi, m, c) in enumerate(params):
        image, mask, weight = vols[vi]
        want = par.sample(image, mask, weight[..., 0], m, c, patch, C, order, extras[b], sigma, keep_dark)
        _compare([t[b] for t in got], want, extras[b], (where, patch, order, b))
        refs.append(want)
    return got, refs, ds


def _quiet_noise(extras, ch, patch):
    """The chosen noise keys keep the restatement's own u1 away from its smallest value 2^-24, where logf is steepest: the gate is
    then the device's libm alone."""
    for e in extras:
        bn = (e or {}).get('blur_or_noise', {})
        if bn.get('kind') == 'noise':
            assert par.noise_uniforms(ch, patch, bn['key'])[0].min() >= 2.0 ** -21, hex(bn['key'])


@pytest.mark.parametrize('order', [0, 1])
def test_neutral_is_the_plain_producer(order):
    patch = (6, 10, 70)
    params = _params(patch)
    ds = _dataset(3, 2, patch, order, sigma=1.0)
    plain = [t.cpu().numpy() for t in ds.batch([0, 1, 2, 3], params=params)]                 # iunet_patch_batch
    assert (plain[0] == 0).any() and (plain[2] > 0).any()
    neutral = {'elastic': {'key': 5, 'alpha': 0.0}, 'color_jitter': {'brightness': 1.0, 'contrast': 1.0, 'contrast_first': True},
               'blur_or_noise': {'kind': 'noise', 'key': 9, 'sigma': 0.0}}
    other = {'elastic': {'key': 0x1234567890abcdef, 'alpha': 0.0}, 'color_jitter': {'brightness': 1.0, 'contrast': 1.0, 'contrast_first': False}}
    for extras in ([{}, {}, {}, {}], [None, {}, None, {}], [neutral, other, {}, neutral], [other, neutral, neutral, other]):
        got = [t.cpu().numpy() for t in ds.batch([0, 1, 2, 3], params=params, extra=extras)]  # iunet_patch_batch_extra
        for g, p, name in zip(got, plain, ('image', 'mask', 'weight')):
            assert np.array_equal(_bits(g), _bits(p)), (extras, name)


@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('ch,C,mixes', [(1, 3, (ELASTIC, JITTER, BLUR, ALL_NOISE)), (3, 2, (NOISE, ALL_BLUR, ALL_NOISE, ELASTIC))])
def test_each_transform_alone_and_all_together(order, ch, C, mixes):
    """(6, 10, 70) at sigma 1 (K = 9: the z extent 6 is barely above the radius 4; a row of 70 crosses a 64-lane block), and
    (24, 22, 26) at sigma 2.5 (K = 21, radius 10), in batches of four with mixed per-sample settings; (4, 5, 150) at sigma 0.8
    (K = 7, radius 3 below the z extent 4): a row of 150 takes a second block of the x pass's 128 lanes, the odd y extent 5 leaves
    the second row of its last 128 x 2 block idle.  That patch lies inside its volumes along x (`_long_params`), and every elastic
    sample's mask or weight differs from the plain producer's at ox >= 128 and in row oy = 4: what the second block and the last row
    wrote is in the compared result."""
    for patch, sigma in (((6, 10, 70), 1.0), ((24, 22, 26), 2.5)):
        _quiet_noise(mixes, ch, patch)
        _check(ch, C, patch, order, _params(patch), list(mixes), sigma, where='mixed')
    _quiet_noise(mixes, ch, LONG)
    params = _long_params()
    got, refs, ds = _check(ch, C, LONG, order, params, list(mixes), 0.8, where='mixed, long rows')
    plain = [t.cpu().numpy() for t in ds.batch([0, 1, 2, 3], params=params)]
    for b, e in enumerate(mixes):
        if 'elastic' in e:
            moved = (_bits(got[1][b]) != _bits(plain[1][b])).any(0) | (_bits(got[2][b]) != _bits(plain[2][b])).any(0)      # [SZ][SY][SX]
            assert moved[:, :, 128:].any() and moved[:, 4, :].any() and moved[:, 4, 128:].any(), (b, int(moved.sum()))


@pytest.mark.parametrize('order', [0, 1])
def test_default_sigma(order):
    """One (44, 42, 48) patch at the defaults alpha 50, sigma 5 (K = 41, radius 20), every transform on."""
    patch = (44, 42, 48)
    params = [(1, _flat(pr.rotation((1, 2, 3), 37.0, 0.5)), [9.0, 15.0, 20.5])]
    got, refs, ds = _check(1, 3, patch, order, params, [ALL_BLUR], where='defaults')
    plain = [t.cpu().numpy() for t in ds.batch([0], params=params)]
    assert not np.array_equal(got[2], plain[2]) and not np.array_equal(got[0], plain[0])
    d = par.displacement(patch, 77, 50.0, ar.taps(5.0)).astype(np.float64)
    print(f'defaults: RMS of a displacement component {np.sqrt((d ** 2).mean()):.4f}, of the vector {np.sqrt((d ** 2).sum(0).mean()):.4f} voxels')


def test_large_displacement_moves_the_dark_band():
    """alpha 400, sigma 2 (K = 17): several voxels, across the volume's faces -- and the dark slab of the second volume moves with
    the field; keep_dark leaves it lit."""
    patch = (24, 22, 26)
    params = [(1, _flat(np.eye(3)), [9.5, 14.5, 19.5]), (1, _flat(pr.rotation((3, 1, 2), 61.0, 0.8)), [10.0, 12.0, 22.0])]
    extras = [{'elastic': {'key': 0x0123456789abcdef, 'alpha': 400.0}}, {'elastic': {'key': 5, 'alpha': 400.0}}]
    got, refs, ds = _check(1, 3, patch, 1, params, extras, sigma=2.0, where='alpha 400')
    plain = [t.cpu().numpy() for t in ds.batch([0, 1], params=params)]
    dark = lambda w: (w[0] == 0)
    assert dark(plain[2][0])[:, 5:9].all() and dark(plain[2][0]).mean() < 0.5                 # source y = 9 .. 12: patch rows 5 .. 8
    assert not np.array_equal(dark(got[2][0]), dark(plain[2][0])) and dark(got[2][0]).any()
    d = par.displacement(patch, 0x0123456789abcdef, 400.0, ar.taps(2.0))
    assert np.abs(d).max() > 4.0
    _check(1, 3, patch, 0, params, extras, sigma=2.0, keep_dark=True, where='alpha 400, keep_dark')


def test_jitter_corners():
    patch = (6, 10, 70)
    corners = [(1.25, 2.0, False), (1.25, 2.0, True), (0.75, 0.5, False), (0.75, 0.5, True)]
    extras = [{'color_jitter': {'brightness': b, 'contrast': c, 'contrast_first': f}} for b, c, f in corners]
    for order in (0, 1):
        got, _, _ = _check(3, 2, patch, order, _params(patch), extras, where='jitter corners')
        assert (got[0][0] == 0).any() and (got[0][0] == 1).any()       # both clamps are hit
        assert got[0][2].min() > 0                                      # a contrast below 1 lifts the zeros outside the volume


def test_blur_sigmas_and_smallest_patch():
    from interactive_unet import _native as nv
    extras = [{'blur_or_noise': {'kind': 'blur', 'sigma': s}} for s in (0.1, 0.148, 1.0, 2.0)]      # 0.148: denormal outer taps
    for patch in ((6, 10, 70), (3, 3, 3), (5, 9, 4)):                 # (3, 3, 3): the smallest the reflection allows
        _check(3, 2, patch, 1, _params(patch), extras, where='blur')
    for patch in ((2, 8, 8), (8, 2, 8), (8, 8, 2)):
        ds = _dataset(3, 2, patch, 1)
        with pytest.raises(nv.NativeError, match='reflect'):
            ds.batch([0, 1, 2, 3], params=_params(patch), extra=extras)
        ds.batch([0, 1, 2, 3], params=_params(patch), extra=[JITTER, NOISE, {}, {}])          # without blur the size is fine
    ds = _dataset(3, 2, (4, 10, 70), 1, sigma=1.0)
    with pytest.raises(nv.NativeError, match='reflect'):
        ds.batch([0], params=_params((4, 10, 70))[:1], extra=[ELASTIC])                       # radius 4: 4 voxels are not enough, 6 are


def test_noise():
    patch = (24, 22, 26)
    extras = [{'blur_or_noise': {'kind': 'noise', 'key': 0xfedcba9876543210, 'sigma': 0.1}}, JITTER,
              {'blur_or_noise': {'kind': 'noise', 'key': 12345, 'sigma': 0.1}}, {}]
    _quiet_noise(extras, 3, patch)
    params = _params(patch)
    for order in (0, 1):
        got, refs, ds = _check(3, 2, patch, order, params, extras, where='noise 3 x 24 x 22 x 26')    # 41 184 voxels a sample
    plain = [t.cpu().numpy() for t in ds.batch([0, 1, 2, 3], params=params)]
    z = (got[0][0].astype(np.float64) - plain[0][0]) / 0.1
    inner = (plain[0][0] > 0.45) & (plain[0][0] < 0.55)               # away from both clamps
    assert inner.sum() > 1000 and abs(z[inner].mean()) < 0.1 and abs(z[inner].std() - 1.0) < 0.1


def test_repeated_call_and_one_elastic_sample():
    """The same descriptors launched again: the histogram and the workspace carry nothing over.  And a batch in which only one sample
    has elastic leaves the others' bits equal to the plain producer's."""
    patch = (24, 22, 26)
    params = _params(patch)
    extras = [ALL_BLUR, ALL_NOISE, JITTER, ELASTIC]
    ds = _dataset(1, 3, patch, 1, sigma=2.5)
    first = [t.cpu().numpy() for t in ds.batch([0, 1, 2, 3], params=params, extra=extras)]
    other = ds.batch([0, 1, 2, 3], params=params[::-1], extra=[NOISE, {}, ALL_BLUR, JITTER])   # dirties the workspace
    again = [t.cpu().numpy() for t in ds.batch([0, 1, 2, 3], params=params, extra=extras)]
    for a, b in zip(first, again):
        assert np.array_equal(_bits(a), _bits(b))
    plain = [t.cpu().numpy() for t in ds.batch([0, 1, 2, 3], params=params)]
    got, _, _ = _check(1, 3, patch, 1, params, [{}, ELASTIC, {}, None], sigma=2.5, where='one elastic sample')
    for b in (0, 2, 3):
        assert all(np.array_equal(_bits(g[b]), _bits(p[b])) for g, p in zip(got, plain)), b
    assert not np.array_equal(got[2][1], plain[2][1])


def test_drawn_parameters():
    """One VolumeDataset.batch with drawn parameters equals the restatement on the same draws: per sample draw(), then draw_extra."""
    from interactive_unet import loader
    patch = (24, 22, 26)
    on = dict(elastic=True, color_jitter=True, blur_or_noise=True)
    vols = _setup(1, 3)[0]
    ds = _dataset(1, 3, patch, 1, sigma=2.5, generator=torch.Generator().manual_seed(5), **on)
    got = [t.cpu().numpy() for t in ds.batch([0, 1, 2])]
    twin = _dataset(1, 3, patch, 1, sigma=2.5, generator=torch.Generator().manual_seed(5), **on)
    for b in range(3):
        vi, m, c = twin.draw()
        extra = loader.draw_extra(twin.generator, True, True, True, 50.0, 0.1)
        assert set(extra) == {'elastic', 'color_jitter', 'blur_or_noise'}
        image, mask, weight = vols[vi]
        _compare([t[b] for t in got], par.sample(image, mask, weight[..., 0], m, c, patch, 3, 1, extra, 2.5), extra, ('drawn', b))
    assert torch.equal(ds.generator.get_state(), twin.generator.get_state())
    # through the loader: repeatable under a seed, and not the plain producer's batch
    mk = lambda **kw: loader.get_volume_loader(num_classes=3, batch_size=2, patch_size=patch, count=3, volumes=_setup(1, 3)[1],
                                               generator=torch.Generator().manual_seed(7), elastic_sigma=2.5, **kw)
    a = [[t.cpu().numpy() for t in batch] for batch in mk(**on)]
    b = [[t.cpu().numpy() for t in batch] for batch in mk(**on)]
    assert len(a) == 2 and a[0][0].shape == (2, 1) + patch and a[1][0].shape[0] == 1
    assert all(np.array_equal(_bits(u), _bits(v)) for x, y in zip(a, b) for u, v in zip(x, y))
    assert not np.array_equal(a[0][0], next(iter(mk()))[0].cpu().numpy())
