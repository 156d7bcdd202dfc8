"""The batch producer's three further transforms on the device (iunet_augment_batch_extra) against their
definition, tests/augment_ref.py, with imposed parameters: y, w and X bit for bit; X on Gaussian-noise samples within one fp16
step and different on at most 0.2 % of the sample's pixels (the device's logf / cosf against correctly rounded ones: moving the
definition's logf and cosf by up to 4 float32 ulps either way changed at most 0.033 % of 57 600 pixels, never by more than a step).
Shapes are the smallest that reach every branch, plus one batch of the workload's own shape."""
import csv
import glob
import os

import numpy as np
import pytest
import torch

from tests import augment_ref as ar
from tests.test_augment_extra_cpu import _annotation, _bits

pytestmark = pytest.mark.gpu

NOISE_SHARE = 0.002
ELASTIC = {'elastic': {'key': 0x0123456789abcdef, 'alpha': 50.0}}
JITTER = {'color_jitter': {'brightness': 1.1, 'contrast': 1.6, 'contrast_first': False}}
BLUR = {'blur_or_noise': {'kind': 'blur', 'sigma': 1.0}}
NOISE = {'blur_or_noise': {'kind': 'noise', 'key': 0xfedcba9876543210, 'sigma': 0.1}}
ALL_BLUR = {'elastic': {'key': 77, 'alpha': 50.0}, 'color_jitter': {'brightness': 0.8, 'contrast': 0.6, 'contrast_first': True},
            'blur_or_noise': {'kind': 'blur', 'sigma': 1.7}}
ALL_NOISE = {'elastic': {'key': 1 << 63 | 5, 'alpha': 50.0}, 'color_jitter': {'brightness': 1.2, 'contrast': 1.9, 'contrast_first': False},
             'blur_or_noise': {'kind': 'noise', 'key': 3, 'sigma': 0.1}}


def _device(samples, params, extras, out, sigma=5.0, keep=None):
    """(X, y, w) numpy of one batch through UNetDataset.batch; `keep`: a list that receives the dataset (to launch again)."""
    from interactive_unet import loader
    ds = loader.UNetDataset(loader.annotations_from_arrays(samples), None, augment=True, out_size=out, elastic_sigma=sigma)
    if keep is not None:
        keep.append(ds)
    return [t.cpu().numpy() for t in ds.batch(list(range(len(samples))), params=params, extra=extras)]


def _compare(got, want, extra, where):
    """One sample: y, w, X bit-equal; a noise sample's X within one fp16 step, differing on at most NOISE_SHARE of its pixels."""
    (X, y, w), (rX, ry, rw) = got, want
    assert X.dtype == y.dtype == w.dtype == np.float16 and X.shape == rX.shape and y.shape == ry.shape and w.shape == rw.shape, where
    assert np.array_equal(_bits(y), _bits(ry)), (where, 'mask')
    assert np.array_equal(_bits(w), _bits(rw)), (where, 'weight')
    if (extra or {}).get('blur_or_noise', {}).get('kind') == 'noise':
        step = np.abs(_bits(X).astype(np.int32) - _bits(rX).astype(np.int32))          # X >= 0: fp16 bits are ordered
        share = float((step != 0).mean())
        print(f'{where}: noise sample, {int((step != 0).sum())} of {step.size} pixels differ from the definition ({100 * share:.4f} %), '
              f'largest difference {int(step.max())} fp16 step(s)')
        assert step.max() <= 1 and share <= NOISE_SHARE, (where, int(step.max()), share)
    else:
        bad = _bits(X) != _bits(rX)
        assert not bad.any(), (where, 'image', int(bad.sum()), np.argwhere(bad)[:5].tolist())


def _check(samples, params, extras, out, sigma=5.0, where=''):
    got = _device(samples, params, extras, out, sigma)
    refs = []
    for b, (image, mask, weight) in enumerate(samples):
        want = ar.sample(image, mask, weight, params[b], extras[b], out, sigma)
        _compare([t[b] for t in got], want, extras[b], (where, b))
        refs.append(want)
    return got, refs


def test_neutral_is_todays_batch():
    from interactive_unet import loader
    rng = np.random.default_rng(3)
    samples = [_annotation(rng, 64, 80, 2, ch=3), _annotation(rng, 50, 50, 2, ch=3)]
    params = [(True, False, -21.5, (3, 5, 50, 60)), (False, True, 90.0, (0, 2, 40, 44))]
    out = (45, 70)
    ds = loader.UNetDataset(loader.annotations_from_arrays(samples), None, augment=True, out_size=out)
    plain = [t.cpu().numpy() for t in ds.batch([0, 1], params=params)]                      # iunet_augment_batch
    neutral = {'elastic': {'key': 5, 'alpha': 0.0}, 'color_jitter': {'brightness': 1.0, 'contrast': 1.0, 'contrast_first': True},
               'blur_or_noise': {'kind': 'noise', 'key': 9, 'sigma': 0.0}}
    other = {'elastic': {'key': 0x1234567890abcdef, 'alpha': 0.0}, 'color_jitter': {'brightness': 1.0, 'contrast': 1.0, 'contrast_first': False}}
    for extras in ([{}, {}], [None, {}], [neutral, other], [other, neutral]):
        got = [t.cpu().numpy() for t in ds.batch([0, 1], params=params, extra=extras)]     # iunet_augment_batch_extra
        for g, p, name in zip(got, plain, ('image', 'mask', 'weight')):
            assert np.array_equal(_bits(g), _bits(p)), (extras, name)


@pytest.mark.parametrize('out', [(45, 70), (40, 300)])          # (40, 300): a row crosses a 256-lane block
@pytest.mark.parametrize('ch,C,mixes', [(3, 2, (ELASTIC, JITTER, BLUR, ALL_NOISE)), (1, 3, (NOISE, ALL_BLUR, ALL_NOISE, ELASTIC))])
def test_each_transform_alone_and_all_together(out, ch, C, mixes):
    rng = np.random.default_rng(10 + ch)
    samples = [_annotation(rng, 64, 80, C, ch=ch), _annotation(rng, 300, 400, C, ch=ch), _annotation(rng, 61, 47, C, ch=ch),
               _annotation(rng, 50, 50, C, ch=ch)]
    params = [(True, True, 37.25, (3, 5, 50, 60)),                    # an affine angle, both flips
              (False, True, 180.0, (20, 31, 200, 260)),               # 180 degrees: a fast path
              (True, False, 90.0, (1, 2, 55, 40)),                    # 90 degrees on a non-square source: the affine grid
              (False, False, 90.0, (4, 0, 40, 45))]                   # 90 degrees on a square source: the fast path
    _check(samples, params, list(mixes), out, where=(out, ch))


def test_elastic():
    from interactive_unet import _native as nv
    rng = np.random.default_rng(12)
    samples = [_annotation(rng, 64, 80, 2, ch=2), _annotation(rng, 61, 47, 2, ch=2)]
    params = [(False, True, -21.5, (3, 5, 50, 60)), (True, False, 0.0, (0, 0, 61, 47))]
    out = (45, 70)
    plain = _device(samples, params, [{}, {}], out)
    # the defaults: alpha 50, sigma 5, K = 41
    extras = [{'elastic': {'key': 0x0123456789abcdef, 'alpha': 50.0}}, {'elastic': {'key': 42, 'alpha': 50.0}}]
    got, _ = _check(samples, params, extras, out, where='defaults')
    assert not np.array_equal(got[2], plain[2])
    # alpha 400, sigma 2 (K = 17): several pixels, across the border -- and the dark band of the annotation moves with the map
    extras = [{'elastic': {'key': 0x0123456789abcdef, 'alpha': 400.0}}, {'elastic': {'key': 5, 'alpha': 400.0}}]
    got, refs = _check(samples, params, extras, out, sigma=2.0, where='alpha 400')
    _, _, inside = ar.displaced(*out, 5, 400.0, ar.taps(2.0))
    assert (~inside).any() and inside.any() and (refs[1][2][0][~inside] == 0).all()         # across the border; outside: w = 0
    dark = lambda w: (w[0] == 0)
    assert dark(plain[2][1]).any() and not np.array_equal(dark(got[2][1]), dark(plain[2][1]))
    # reflect without edge repeat: every side must exceed the radius 20 -- 21 rows pass, 20 are refused before any launch
    _check(samples[:1], params[:1], extras[:1], (21, 70), where='21 rows')
    with pytest.raises(nv.NativeError, match='reflect'):
        _device(samples[:1], params[:1], extras[:1], (20, 70))
    with pytest.raises(nv.NativeError, match='reflect'):
        _device(samples[:1], params[:1], extras[:1], (70, 20))
    _device(samples[:1], params[:1], [{}], (20, 70))                                        # without elastic the size is fine


def test_colour_jitter():
    rng = np.random.default_rng(13)
    corners = [(1.25, 2.0, False), (1.25, 2.0, True), (0.75, 0.5, False), (0.75, 0.5, True)]
    samples = [_annotation(rng, 64, 80, 2, ch=3) for _ in corners]
    params = [(bool(k & 1), bool(k & 2), 30.0 + 17 * k, (2, 3, 55, 70)) for k in range(4)]           # rotated: outside pixels in every sample
    extras = [{'color_jitter': {'brightness': b, 'contrast': c, 'contrast_first': f}} for b, c, f in corners]
    got, refs = _check(samples, params, extras, (45, 70), where='corners')
    hi, lo = got[0][0], got[0][2]
    assert (hi == 0).any() and (hi == 1).any()                        # both clamps are hit
    assert ar.source_index(64, 80, *params[2], (45, 70))[0][0, 0] == -1 and refs[2][2][0, 0, 0] == 0          # the corner is outside: w = 0
    assert lo[0, 0, 0] > 0.1                                          # ... and a contrast below 1 lifts its byte 0
    swapped = _device(samples[:1], params[:1], extras[1:2], (45, 70))
    assert not np.array_equal(got[0][0], swapped[0][0])               # the same corner, contrast first: the order matters
    # a constant image: with and without outside pixels
    image = np.full((40, 52, 2), 77, np.uint8)
    _, mask, weight = _annotation(rng, 40, 52, 2, ch=2)
    const = [(image, mask, weight)] * 2
    cparams = [(False, False, 0.0, (0, 0, 40, 52)), (False, False, 45.0, (0, 0, 40, 52))]
    cextras = [{'color_jitter': {'brightness': 1.0, 'contrast': 2.0, 'contrast_first': True}},
               {'color_jitter': {'brightness': 1.2, 'contrast': 1.5, 'contrast_first': False}}]
    got, _ = _check(const, cparams, cextras, (33, 35), where='constant')
    assert len(np.unique(got[0][0])) == 1 and abs(float(got[0][0, 0, 0, 0]) - 77 / 255) < 1e-3


def test_blur():
    from interactive_unet import _native as nv
    rng = np.random.default_rng(14)
    samples = [_annotation(rng, 64, 80, 2, ch=2) for _ in range(3)]
    params = [(False, False, 12.0, (3, 5, 50, 60)), (True, False, 180.0, (0, 0, 64, 80)), (False, True, -75.0, (10, 10, 40, 50))]
    extras = [{'blur_or_noise': {'kind': 'blur', 'sigma': s}} for s in (0.1, 1.0, 2.0)]
    _check(samples, params, extras, (45, 70), where='blur')
    _check(samples, params, extras, (6, 5), where='blur 6 x 5')       # both borders reflect into every pixel
    _check(samples, params, extras, (3, 3), where='blur 3 x 3')       # the smallest output the reflection allows
    for out in ((2, 70), (70, 2)):
        with pytest.raises(nv.NativeError, match='reflect'):
            _device(samples, params, extras, out)
    _device(samples, params, [{}] * 3, (2, 70))


def test_noise():
    rng = np.random.default_rng(15)
    samples = [_annotation(rng, 64, 80, 2, ch=3), _annotation(rng, 300, 400, 2, ch=3)]
    params = [(False, False, 12.0, (3, 5, 50, 60)), (True, True, 180.0, (20, 31, 200, 260))]
    extras = [{'blur_or_noise': {'kind': 'noise', 'key': 0xfedcba9876543210, 'sigma': 0.1}},
              {'blur_or_noise': {'kind': 'noise', 'key': 12345, 'sigma': 0.1}}]
    got, refs = _check(samples, params, extras, (120, 160), where='noise 3 x 120 x 160')    # 57 600 pixels a sample
    plain = _device(samples, params, [{}, {}], (120, 160))
    z = (got[0][1].astype(np.float64) - plain[0][1]) / 0.1
    inner = (plain[0][1] > 0.45) & (plain[0][1] < 0.55)               # away from both clamps
    assert inner.sum() > 2000 and abs(z[inner].mean()) < 0.1 and abs(z[inner].std() - 1.0) < 0.1


def test_workload_shape_and_repeated_launch():
    """One 2 x 512 x 512 batch with everything on, and the same descriptors launched again: the histogram and the workspace carry
    nothing over."""
    rng = np.random.default_rng(16)
    samples = [_annotation(rng, 512, 512, 2), _annotation(rng, 300, 400, 2)]
    params = [(True, False, 33.0, (40, 60, 400, 380)), (False, True, -120.5, (10, 20, 250, 300))]
    extras = [ALL_BLUR, ALL_NOISE]
    keep = []
    first = _device(samples, params, extras, (512, 512), keep=keep)
    again = [t.cpu().numpy() for t in keep[0].batch([0, 1], params=params, extra=extras)]
    for a, b in zip(first, again):
        assert np.array_equal(_bits(a), _bits(b))
    for b, (image, mask, weight) in enumerate(samples):
        _compare([t[b] for t in first], ar.sample(image, mask, weight, params[b], extras[b]), extras[b], ('512', b))


def test_seeded_loader():
    from interactive_unet import loader
    rng = np.random.default_rng(17)
    samples = [_annotation(rng, 96, 96, 2) for _ in range(3)]
    ann = loader.annotations_from_arrays(samples)
    on = dict(elastic=True, color_jitter=True, blur_or_noise=True)
    a = [[t.cpu().numpy() for t in batch] for batch in loader.get_data_loader(batch_size=2, annotations=ann, generator=torch.Generator().manual_seed(5), **on)]
    b = [[t.cpu().numpy() for t in batch] for batch in loader.get_data_loader(batch_size=2, annotations=ann, generator=torch.Generator().manual_seed(5), **on)]
    assert len(a) == 2 and a[0][0].shape == (2, 1, 512, 512) and a[1][0].shape[0] == 1
    assert all(np.array_equal(_bits(u), _bits(v)) for x, y in zip(a, b) for u, v in zip(x, y))       # repeatable
    plain = next(iter(loader.get_data_loader(batch_size=2, annotations=ann, generator=torch.Generator().manual_seed(5))))
    assert not np.array_equal(a[0][0], plain[0].cpu().numpy())
    # the first batch is the definition on the parameters the same seed gives: the shuffle, then per sample draw_params, draw_extra
    g = torch.Generator().manual_seed(5)
    order = torch.randperm(3, generator=g).tolist()
    for k, i in enumerate(order[:2]):
        params = loader.draw_params(96, 96, g)
        extra = loader.draw_extra(g, True, True, True)
        assert set(extra) == {'elastic', 'color_jitter', 'blur_or_noise'}
        _compare([t[k] for t in a[0]], ar.sample(*samples[i], params, extra), extra, ('loader', k))


def test_train_model_with_the_transforms(tmp_path, monkeypatch):
    from PIL import Image
    from interactive_unet import trainer, loader
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(18)
    for split, n in (('train', 2), ('val', 1)):
        for sub in ('images', 'masks', 'weights'):
            os.makedirs(os.path.join('data', split, sub))
        for k in range(n):
            img = rng.integers(1, 256, (96, 96), dtype=np.uint8)
            cls = (img > 127).astype(int) + 1                             # palette colours 1 and 2; colour 0 = unlabelled
            cls[rng.random(cls.shape) < 0.1] = 0
            Image.fromarray(img).save(os.path.join('data', split, 'images', f'{k:04d}.tiff'))
            Image.fromarray(loader.COLORS[cls]).save(os.path.join('data', split, 'masks', f'{k:04d}.tiff'))
            Image.fromarray(np.full((96, 96), 255, np.uint8)).save(os.path.join('data', split, 'weights', f'{k:04d}.tiff'))
    seen = []
    make = loader.get_data_loader

    def spy(**kw):
        seen.append(kw)
        return make(**kw)
    monkeypatch.setattr(loader, 'get_data_loader', spy)
    trainer.train_model(1e-3, 2, 1, 1, 2, 'MCC + CE', 'U-Net', 'mit_b0', False, elastic=True, color_jitter=True, blur_or_noise=True)
    assert [bool(kw.get('elastic') and kw.get('color_jitter') and kw.get('blur_or_noise')) for kw in seen] == [True, False]
    rows = list(csv.DictReader(open(glob.glob('model/history/*/version_0/metrics.csv')[0])))
    losses = [float(r['train/Loss']) for r in rows if r['train/Loss']]
    assert len(losses) == 1 and np.isfinite(losses[0]) and os.path.isfile('model/model.ckpt')
