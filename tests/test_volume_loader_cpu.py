"""The 3-D patch batch producer without a GPU: the numpy restatement of iunet_patch_batch's arithmetic
(tests/patch_ref.py) against plain crops, transposes and flips -- which pins the row / column convention of `m` independently of the
restatement's own formula -- and the host side of interactive_unet.loader: parameter draws, candidates, shape checks, and
trainer.train_model's refusal of a patch the network cannot pool."""
import numpy as np
import pytest
import torch

from tests import patch_ref as pr

SHAPE, PATCH = (30, 32, 34), (4, 6, 8)


@pytest.fixture(scope='module')
def volume():
    return pr.make_volume(np.random.default_rng(3), SHAPE, ch=2, classes=3)


def _equal(got, want):
    return all(g.dtype == np.float16 and g.shape == w.shape and np.array_equal(g.view(np.uint16), w.view(np.uint16)) for g, w in zip(got, want))


def test_identity_with_a_snapped_centre_is_a_plain_crop(volume):
    image, mask, weight = volume
    corner = (5, 7, 9)
    c = pr.snapped_centre(np.eye(3), corner, PATCH)
    want = pr.crop(image, mask, weight[..., 0], corner, PATCH, 3)
    for order in (0, 1):
        got = pr.patch(image, mask, weight[..., 0], np.eye(3), c, PATCH, 3, order)
        assert got[0].shape == (2,) + PATCH and got[1].shape == (3,) + PATCH
        assert _equal(got, want), order


def test_signed_permutations_are_transposes_and_flips_of_the_crop(volume):
    image, mask, weight = volume
    perms = pr.signed_permutations()
    assert len(perms) == 48 and len({M.tobytes() for M in perms}) == 48
    corner = (11, 3, 6)
    for M in perms:
        c = pr.snapped_centre(M, corner, PATCH)
        X = np.moveaxis(pr.LUT[pr.transform_crop(image, M, corner, PATCH)], -1, 0)
        k = pr.transform_crop(mask, M, corner, PATCH)
        y = np.stack([np.where(k == cls, pr.LUT[255], pr.LUT[0]) for cls in range(3)])
        w = np.stack([pr.LUT[pr.transform_crop(weight[..., 1], M, corner, PATCH)]] * 3)
        got0 = pr.patch(image, mask, weight[..., 1], M, c, PATCH, 3, 0)
        got1 = pr.patch(image, mask, weight[..., 1], M, c, PATCH, 3, 1)
        assert _equal(got0, (X, y, w)), M
        assert _equal(got1, got0), M                   # integer sources: both orders read the same voxel


def _cpu_dataset(volumes, **kw):
    from interactive_unet import loader
    return loader.VolumeDataset(loader.volume_annotations_from_arrays(volumes, device='cpu'), **kw)


def test_draw_patch_params(volume):
    from interactive_unet import loader
    image, mask, weight = volume
    cands = loader.patch_candidates(torch.from_numpy(mask), torch.from_numpy(weight[..., 0]))
    patch = (8, 16, 24)
    for mode, augment in (('random', True), ('grid', True), ('random', False)):
        a = [loader.draw_patch_params(SHAPE, patch, cands, torch.Generator().manual_seed(11), sampling_mode=mode, augment=augment) for _ in range(2)]
        assert a[0] == a[1] and len(a[0][0]) == 9 and len(a[0][1]) == 3
        gen = torch.Generator().manual_seed(12)
        seen = set()
        for _ in range(40):
            m, c = loader.draw_patch_params(SHAPE, patch, cands, gen, sampling_mode=mode, scale=(0.5, 1.0), augment=augment)
            M = np.array(m).reshape(3, 3)
            seen.add(M.tobytes())
            if mode == 'random' and augment:
                s2 = (M @ M.T)[0, 0]
                assert np.abs(M @ M.T - s2 * np.eye(3)).max() <= 1e-6 and 0.5 <= np.sqrt(s2) <= 1.0
            else:
                assert any(np.array_equal(M, P) for P in pr.signed_permutations()) and (augment or np.array_equal(M, np.eye(3)))
                p = pr.coordinates(m, c, patch)
                assert np.array_equal(p, np.rint(p))
                assert all(p[a].min() >= 0 and p[a].max() <= SHAPE[a] - 1 for a in range(3))      # the patch fits: moved inside
        assert len(seen) == 1 if not augment else len(seen) == 40 if mode == 'random' else 6 < len(seen) <= 48
    with pytest.raises(ValueError, match='sampling_mode'):
        loader.draw_patch_params(SHAPE, patch, cands, None, sampling_mode='spiral')


def test_every_training_patch_holds_an_annotation():
    """Annotations on three planes only and no dark voxel: the centre rule puts an annotated voxel on a voxel of every patch."""
    rng = np.random.default_rng(5)
    shape = (40, 48, 56)
    image, mask, _ = pr.make_volume(rng, shape)
    weight = np.zeros(shape + (2,), np.uint8)
    weight[10, :, :, 0] = 255
    weight[:, 20, :, 0] = 200
    weight[:, :, 30, 0] = 90
    ds = _cpu_dataset([(image, mask, weight)], num_classes=2, patch_size=16, count=200, generator=torch.Generator().manual_seed(1))
    assert len(ds) == 200
    for _ in range(len(ds)):
        vi, m, c = ds.draw()
        _, y, w = pr.patch(image, mask, weight[..., 0], m, c, ds.patch, 2, 1)
        assert vi == 0 and w.max() > 0 and y.max() > 0


def test_patch_candidates_are_the_slicers_over_annotated_voxels(volume):
    from interactive_unet import loader
    from interactive_unet.slicer import Slicer
    _, mask, weight = volume
    w = np.where(np.random.default_rng(2).random(SHAPE) < 0.1, weight[..., 0], 0).astype(np.uint8)
    w[mask == 2] = 0                                            # a class that is nowhere annotated is no candidate
    cands, probs = loader.patch_candidates(torch.from_numpy(mask), torch.from_numpy(w))
    # the reference's function on the volume with every unannotated voxel set aside as class 255, that class dropped
    ref_c, ref_p = Slicer(SHAPE).get_origin_candidates(np.where(w > 0, mask, 255))
    ref_c, ref_p = ref_c[:-1], ref_p[:-1] / ref_p[:-1].sum()
    assert len(cands) == len(ref_c) == 2
    for a, b in zip(cands, ref_c):
        assert np.array_equal(a.numpy(), b)
    assert np.allclose(np.asarray(probs), ref_p, rtol=1e-12, atol=0)


def test_train_model_refuses_a_patch_the_network_cannot_pool(tmp_path, monkeypatch):
    from interactive_unet import trainer
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: pytest.fail('the GPU was touched before the refusal'))
    with pytest.raises(ValueError, match=r'2\*\*\(levels-1\) = 8'):
        trainer.train_model(dim=3, patch_size=20)
    with pytest.raises(ValueError, match='patch_size'):
        trainer.train_model(dim=3, patch_size=(16, 16, 12))


def test_volume_dataset_refuses_mismatched_shapes(volume):
    from interactive_unet import loader
    image, mask, weight = volume
    with pytest.raises(ValueError, match='annotation volumes'):
        loader.volume_annotations_from_arrays([(image, mask[:-1], weight)], device='cpu')
    with pytest.raises(ValueError, match='annotation volumes'):
        loader.volume_annotations_from_arrays([(image, mask, weight[..., :1])], device='cpu')
    good = loader.volume_annotations_from_arrays([(image[..., 0], mask, weight)], device='cpu')
    assert good[0][0].shape == SHAPE + (1,) and good[0][0].dtype == torch.uint8
    with pytest.raises(ValueError, match='annotation volumes'):
        loader.VolumeDataset([(good[0][0], good[0][1][:, :-1].contiguous(), good[0][2])], 2)
    with pytest.raises(ValueError, match='image channels'):
        loader.VolumeDataset(good + loader.volume_annotations_from_arrays([(image, mask, weight)], device='cpu'), 2)
    with pytest.raises(ValueError, match='no annotated voxel'):
        loader.VolumeDataset([(good[0][0], good[0][1], torch.zeros_like(good[0][2]))], 2, patch_size=8, count=1, augment=False)
    ds = loader.VolumeDataset(good, 3, patch_size=(4, 6, 8), count=7, augment=False, generator=torch.Generator().manual_seed(0))
    assert len(ds) == 7 and ds.patch == (4, 6, 8) and len(ds._fixed) == 7


def test_patch_batch_refuses_bad_arguments_before_any_launch():
    """Argument validation answers with a status and a message, no GPU needed; the descriptor mirror has the library's size."""
    import ctypes
    import os
    from interactive_unet import _native as nv, loader
    if not os.path.isfile(nv.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    l = nv.lib()
    assert l.iunet_patch_desc_bytes() == ctypes.sizeof(loader.PatchDesc)
    buf = (ctypes.c_int * 64)()
    good = dict(descs=buf, B=2, ch=1, C=2, SZ=8, SY=8, SX=8, order=1, lut=buf, X=buf, y=buf, w=buf, stream=None)
    for change, word in ((dict(descs=None), b'null'), (dict(lut=None), b'null'), (dict(w=None), b'null'), (dict(B=0), b'B 0'),
                         (dict(ch=0), b'channels 0'), (dict(ch=5), b'channels 5'), (dict(C=0), b'classes 0'), (dict(C=17), b'classes 17'),
                         (dict(SZ=0), b'patch 0 x'), (dict(SY=-1), b'x -1 x'), (dict(SX=0), b'x 0'), (dict(order=2), b'order 2'),
                         (dict(order=-1), b'order -1'), (dict(B=8192, SZ=8), b'grid limit')):
        rc = l.iunet_patch_batch(*{**good, **change}.values())
        assert rc < 0 and word in l.iunet_last_error(), (change, l.iunet_last_error())
