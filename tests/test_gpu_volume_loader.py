"""The 3-D patch batch producer on the GPU: iunet_patch_batch through loader.VolumeDataset.batch gives the
fp16 bits of the numpy float32 restatement (tests/patch_ref.py) for X, y and w, at spline orders 0 and 1, for 1 and 3 image channels
and 2 and 5 classes, on two non-cubic volumes mixed in one batch of 3 with the patch (8, 16, 24); then the loader and
trainer.train_model(dim=3) from annotation volumes on disk."""
import csv
import glob
import os

import numpy as np
import pytest
import torch

from tests import patch_ref as pr

pytestmark = pytest.mark.gpu

PATCH = (8, 16, 24)
SHAPES = ((20, 24, 28), (17, 31, 22))
IDS = 6                                   # class ids 0 .. 5 in the masks: with C = 2 and C = 5 some set no channel
PERMS = [pr.signed_permutations()[i] for i in (3, 13, 22, 26, 36, 47)]     # six: every axis order once, flips included


def _volumes(ch):
    """The two volumes, with a slab where image channel 0 is zero (the other channels are not)."""
    rng = np.random.default_rng(40 + ch)
    out = []
    for shape in SHAPES:
        image, mask, weight = pr.make_volume(rng, shape, ch=ch, classes=IDS)
        image[:, 9:13, :, 0] = 0
        out.append((image, mask, weight))
    return out


_cache = {}


def _setup(ch):
    """(numpy volumes, resident volumes) per channel count, made once."""
    if ch not in _cache:
        from interactive_unet import loader
        vols = _volumes(ch)
        _cache[ch] = (vols, loader.volume_annotations_from_arrays(vols))
    return _cache[ch]


def _dataset(ch, C, order, weight_channel=0, keep_dark=False):
    from interactive_unet import loader
    return loader.VolumeDataset(_setup(ch)[1], C, patch_size=PATCH, count=3, weight_channel=weight_channel, order=order, keep_dark=keep_dark)


def _reference(ch, C, order, params, weight_channel=0, keep_dark=False):
    vols = _setup(ch)[0]
    per = [pr.patch(vols[vi][0], vols[vi][1], vols[vi][2][..., weight_channel], m, c, PATCH, C, order, keep_dark) for vi, m, c in params]
    return [np.stack([s[k] for s in per]) for k in range(3)]


def _bits_equal(got, want, what):
    for g, r, name in zip(got, want, 'Xyw'):
        g = g.cpu().numpy()
        assert g.dtype == np.float16 and g.shape == r.shape, (what, name)
        bad = g.view(np.uint16) != r.view(np.uint16)
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _flat(M):
    return [float(v) for v in np.asarray(M).reshape(-1)]


def _outside_fraction(vi, m, c):
    return 1.0 - pr.nearest(pr.coordinates(m, c, PATCH), SHAPES[vi])[1].mean()


CONFIGS = [(1, 2), (3, 5), (1, 5), (3, 2)]


@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('ch,C', CONFIGS)
def test_identity_with_a_snapped_centre(ch, C, order):
    corners = [(5, 4, 2), (9, 15, -1), (12, 8, 4)]                   # the boxes touch the far faces; x of the second volume is narrower than the patch
    vis = [0, 1, 0]
    params = [(vi, _flat(np.eye(3)), pr.snapped_centre(np.eye(3), k, PATCH)) for vi, k in zip(vis, corners)]
    got = _dataset(ch, C, order, keep_dark=True).batch([0, 1, 2], params)
    assert got[0].shape == (3, ch) + PATCH and got[1].shape == got[2].shape == (3, C) + PATCH
    _bits_equal(got, _reference(ch, C, order, params, keep_dark=True), 'identity')
    vols = _setup(ch)[0]
    for b in (0, 2):                                                 # inside the volume: the plain crop
        crop = pr.crop(vols[0][0], vols[0][1], vols[0][2][..., 0], corners[b], PATCH, C)
        _bits_equal([t[b] for t in got], crop, 'identity vs the plain crop')
    b, inner = 1, (slice(None), slice(None), slice(None), slice(1, 23))      # the second volume: its 22 columns, zero padding either side
    crop = pr.crop(vols[1][0], vols[1][1], vols[1][2][..., 0], (9, 15, 0), (8, 16, 22), C)
    _bits_equal([t[b][inner] for t in got], crop, 'identity vs the plain crop, narrow volume')
    assert all(float(t[b][..., 0].abs().max()) == 0 and float(t[b][..., 23].abs().max()) == 0 for t in got)


@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('ch,C', CONFIGS)
def test_signed_permutations(ch, C, order):
    vols = _setup(ch)[0]
    ds = _dataset(ch, C, order, keep_dark=True)
    fits = 0
    for M0, M1 in zip(PERMS, PERMS[1:] + PERMS[:1]):
        corner = (1, 3, 2)
        Ms, vis = (M0, M1, M1), (0, 1, 0)
        params = [(vi, _flat(M), pr.snapped_centre(M, corner, PATCH)) for vi, M in zip(vis, Ms)]
        got = ds.batch([0, 1, 2], params)
        _bits_equal(got, _reference(ch, C, order, params, keep_dark=True), 'signed permutation')
        for b, (vi, M) in enumerate(zip(vis, Ms)):                  # where the box lies inside the volume: transpose / flip of the crop
            perm = [int(np.argmax(np.abs(M[a]))) for a in range(3)]
            if any(corner[a] + PATCH[perm[a]] > SHAPES[vi][a] for a in range(3)):
                continue
            fits += 1
            image, mask, weight = vols[vi]
            X = np.moveaxis(pr.LUT[pr.transform_crop(image, M, corner, PATCH)], -1, 0)
            k = pr.transform_crop(mask, M, corner, PATCH)
            y = np.stack([np.where(k == cls, pr.LUT[255], pr.LUT[0]) for cls in range(C)])
            w = np.stack([pr.LUT[pr.transform_crop(weight[..., 0], M, corner, PATCH)]] * C)
            _bits_equal([t[b] for t in got], (X, y, w), 'signed permutation vs transpose / flip')
    assert fits >= 4


@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('ch,C', CONFIGS)
def test_rotated_patches(ch, C, order):
    # partly outside: the padding branch and the gather both run
    M = _flat(pr.rotation((1, 2, 3), 37.0, 1.25))
    params = [(0, M, [3.0, 20.0, 5.0]), (1, M, [14.0, 2.0, 19.0]), (0, M, [3.0, 20.0, 5.0])]
    for vi, m, c in params[:2]:
        assert 0.10 <= _outside_fraction(vi, m, c) <= 0.90
    ds = _dataset(ch, C, order)
    _bits_equal(ds.batch([0, 1, 2], params), _reference(ch, C, order, params), 'rotated, partly outside')
    # fully inside
    M = _flat(pr.rotation((3, 1, 2), 61.0, 0.5))
    params = [(0, M, [10.0, 12.0, 14.0]), (1, M, [8.5, 15.25, 11.0]), (0, M, [9.0, 11.5, 13.0])]
    for vi, m, c in params:
        assert _outside_fraction(vi, m, c) == 0.0
    got = ds.batch([0, 1, 2], params)
    _bits_equal(got, _reference(ch, C, order, params), 'rotated, fully inside')
    again = ds.batch([0, 1, 2], params)                              # repeatability: the same descriptors give the same bits
    assert all(torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize('order', [0, 1])
@pytest.mark.parametrize('ch,C', CONFIGS[:2])
def test_ties_round_half_to_even(ch, C, order):
    """Identity with an integer centre and an even patch: every coordinate is an exact .5 tie."""
    params = [(0, _flat(np.eye(3)), [10.0, 12.0, 14.0]), (1, _flat(np.eye(3)), [8.0, 15.0, 11.0]), (0, _flat(-np.eye(3)), [10.0, 12.0, 14.0])]
    p = pr.coordinates(params[0][1], params[0][2], PATCH)
    assert np.all(p - np.floor(p) == 0.5)
    r = np.rint(p)
    assert np.all(r % 2 == 0) and (r < p).any() and (r > p).any()    # half to even: some ties go down, some up
    _bits_equal(_dataset(ch, C, order).batch([0, 1, 2], params), _reference(ch, C, order, params), 'ties')


@pytest.mark.parametrize('ch,C', CONFIGS[:2])
def test_dark_rule_and_class_ids_beyond_C(ch, C):
    vols = _setup(ch)[0]
    corner = (5, 4, 2)                                               # source y = 4 .. 19 crosses the dark slab y = 9 .. 12
    params = [(0, _flat(np.eye(3)), pr.snapped_centre(np.eye(3), corner, PATCH))] * 3
    X, y, w = [t.cpu().numpy() for t in _dataset(ch, C, 0).batch([0, 1, 2], params)]
    Xk, yk, wk = [t.cpu().numpy() for t in _dataset(ch, C, 0, keep_dark=True).batch([0, 1, 2], params)]
    _bits_equal([torch.from_numpy(a) for a in (X, y, w)], _reference(ch, C, 0, params), 'dark rule')
    dark = np.zeros(PATCH, bool)
    dark[:, 5:9] = True
    assert np.all(y[:, :, dark] == 0) and np.all(w[:, :, dark] == 0) and np.array_equal(X, Xk)
    assert wk[:, :, dark].max() > 0 and yk[:, :, dark].max() == 1 and np.array_equal(y[:, :, ~dark], yk[:, :, ~dark])
    if ch > 1:
        assert X[:, 1:][:, :, dark].max() > 0                       # only channel 0 decides
    k = vols[0][1][tuple(slice(o, o + s) for o, s in zip(corner, PATCH))]
    assert (k >= C).any() and np.all(yk[0][:, k >= C] == 0) and np.all(yk[0].sum(0)[k < C] == 1)
    assert wk[0][:, k >= C].max() > 0                                # the weight does not depend on the class id


@pytest.mark.parametrize('order', [0, 1])
def test_strided_weight_channel(order):
    """Channel 1 of the [Z, Y, X, 2] weight volume through the element stride equals a contiguous copy of it."""
    from interactive_unet import loader
    vols = _setup(1)[0]
    M = _flat(pr.rotation((3, 1, 2), 61.0, 0.5))
    params = [(0, M, [10.0, 12.0, 14.0]), (1, M, [8.5, 15.25, 11.0]), (0, _flat(np.eye(3)), [3.5, 20.5, 5.5])]
    strided = _dataset(1, 2, order, weight_channel=1).batch([0, 1, 2], params)
    copies = loader.volume_annotations_from_arrays([(i, m, np.ascontiguousarray(w[..., 1])) for i, m, w in vols])
    plain = loader.VolumeDataset(copies, 2, patch_size=PATCH, count=3, order=order).batch([0, 1, 2], params)
    assert all(torch.equal(a, b) for a, b in zip(strided, plain))
    _bits_equal(strided, _reference(1, 2, order, params, weight_channel=1), 'strided weight')
    other = _dataset(1, 2, order, weight_channel=0).batch([0, 1, 2], params)
    assert not torch.equal(other[2], strided[2])


def test_get_volume_loader():
    from interactive_unet import loader
    vols = _setup(1)[1]

    def epoch(ld):
        return [tuple(t.clone() for t in b) for b in ld]
    mk = lambda seed, **kw: loader.get_volume_loader(num_classes=2, batch_size=2, patch_size=PATCH, count=5, volumes=vols,
                                                     generator=torch.Generator().manual_seed(seed), **kw)
    a, b, c = epoch(mk(5)), epoch(mk(5)), epoch(mk(6))
    assert len(mk(5)) == 3 and len(a) == 3 and a[0][0].shape == (2, 1) + PATCH and a[0][1].shape == a[0][2].shape == (2, 2) + PATCH
    assert a[2][0].shape[0] == 1 and a[0][0].dtype == torch.float16
    assert all(torch.equal(u, v) for p, q in zip(a, b) for u, v in zip(p, q))
    assert not all(torch.equal(p[0], q[0]) for p, q in zip(a, c))
    assert all(p[2].max() > 0 for p in a)
    val = mk(7, set_type='val', augment=False, shuffle=False)
    assert val.dataset.weight_channel == 1 and mk(5).dataset.weight_channel == 0
    first, second = epoch(val), epoch(val)
    assert len(first) == 3 and all(torch.equal(u, v) for p, q in zip(first, second) for u, v in zip(p, q))
    train = mk(7)
    assert not all(torch.equal(p[0], q[0]) for p, q in zip(epoch(train), epoch(train)))        # new patches every epoch


def test_train_model_from_annotation_volumes(tmp_path, monkeypatch):
    """trainer.train_model(dim=3) with no loaders injected: the image volume is read from data/image_volumes/<name>.zarr, the
    annotation volumes from data/{mask,weight}_volumes/<name>.npy, batches come from the patch producer (augmented for training, a
    fixed set for validation), checkpoint and history appear."""
    from interactive_unet import trainer, utils, loader
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(9)
    for sub in ('image_volumes', 'mask_volumes', 'weight_volumes'):
        os.makedirs(os.path.join('data', sub))
    zz, yy, xx = np.meshgrid(*[np.arange(32)] * 3, indexing='ij')
    truth = ((zz - 16) ** 2 + (yy - 14) ** 2 + (xx - 18) ** 2 < 100).astype(np.uint8)
    vol = np.clip(np.where(truth == 1, 190, 70) + rng.normal(0, 10, truth.shape), 1, 255).astype(np.uint8)
    weight = np.zeros((32, 32, 32, 2), np.uint8)
    weight[12, :, :, 0] = weight[:, 15, :, 0] = 255                 # annotated slices: training
    weight[:, :, 20, 1] = 255                                       # validation
    utils.create_multiscale_zarr(vol, os.path.join('data', 'image_volumes', 'a.zarr'), chunk_size=16, shard_size=32)
    np.save(os.path.join('data', 'mask_volumes', 'a.npy'), truth)
    np.save(os.path.join('data', 'weight_volumes', 'a.npy'), weight)
    vols = loader.load_volume_annotations()
    assert len(vols) == 1 and vols[0][0].shape == (32, 32, 32, 1) and vols[0][0].is_cuda and vols[0][2].shape == (32, 32, 32, 2)
    assert np.array_equal(vols[0][0][..., 0].cpu().numpy(), vol)
    trainer.train_model(1e-3, 2, 2, 1, 2, 'MCC + CE', 'U-Net', 'mit_b0', False, dim=3, patch_size=16, patches_per_epoch=4)
    assert os.path.isfile('model/model.ckpt')
    rows = list(csv.DictReader(open(glob.glob('model/history/*/version_0/metrics.csv')[0])))
    train = [float(r['train/Loss']) for r in rows if r['train/Loss']]
    val = [float(r['val/Loss']) for r in rows if r['val/Loss']]
    assert len(train) == 2 and len(val) == 2 and np.isfinite(train + val).all()
