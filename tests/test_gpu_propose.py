"""The slice proposal on the device: iunet_uncertainty_volume bit for bit and iunet_plane_scores exactly
against the definition tests/propose_ref.py, and the host layer interactive_unet/propose.py end to end -- on a planted blob and on a
real prediction of the 3-D net."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import propose_ref as pr
from tests.volume_inputs import offset_copy, random_pred, random_slicer

E = np.eye(3)
VOLUMES = ((9, 10, 13), (17, 31, 70), (5, 7, 67), (6, 9, 40))   # ragged on every axis; rows longer than a wave; one brick row of long rows;
                                                               # rows of whole 16-byte slots at 2 and 16 classes (the staging's aligned path)
CLASSES = (2, 3, 5, 16)                                  # 3 and 5: a row's byte count is no multiple of any load width


def _sparse(shape, ch, seed, zero_share):
    rng = np.random.default_rng(seed)
    v = rng.integers(1, 256, tuple(shape) + (ch,), dtype=np.uint8)
    v[rng.random(v.shape) < zero_share] = 0
    return v


def _uncertainty(pd, wd, imd, g, want_u=True, want_bricks=True):
    """The entry point itself; outputs start from a pattern, so an element left unwritten shows."""
    from interactive_unet import _native as nv
    Z, Y, X, C = pd.shape
    u = torch.full((Z, Y, X), 77, dtype=torch.uint8, device='cuda') if want_u else None
    bricks = torch.full([-(-n // g) for n in (Z, Y, X)], -1, dtype=torch.int32, device='cuda') if want_bricks else None
    nv.call('iunet_uncertainty_volume', nv.ptr(pd), Z, Y, X, C, nv.ptr(wd), 0 if wd is None else wd.shape[3], nv.ptr(imd),
            0 if imd is None else imd.shape[3], g, nv.ptr(u), nv.ptr(bricks), nv.stream())
    return u, bricks


@pytest.mark.parametrize('C', CLASSES)
@pytest.mark.parametrize('shape', VOLUMES)
def test_uncertainty_volume_is_the_definition(shape, C):
    pred = random_pred(shape, C, C + shape[2])
    pd = torch.tensor(pred).cuda()
    never, tie = (pred.max(-1) == 0).mean(), (pr.uncertainty(pred) == 255).mean()
    assert 0.03 < never < 0.2 and 0.03 < tie < 0.25, (never, tie)
    for wch in (0, 1, 2):
        weight = _sparse(shape, wch, 1 + wch, 0.7) if wch else None
        wd = None if weight is None else torch.tensor(weight).cuda()
        for ich in (0, 1, 3):
            image = _sparse(shape, ich, 4 + ich, 0.2) if ich else None
            imd = None if image is None else torch.tensor(image).cuda()
            want = pr.uncertainty(pred, weight, image)
            assert want.any()
            for g in pr.BRICKS:
                want_b = pr.brick_sums(want, g).astype(np.int64)
                u, bricks = _uncertainty(pd, wd, imd, g)
                assert np.array_equal(u.cpu().numpy(), want), (wch, ich, g)
                assert np.array_equal(bricks.cpu().numpy().astype(np.int64), want_b), (wch, ich, g)
                u_only, none = _uncertainty(pd, wd, imd, g, want_bricks=False)
                assert none is None and torch.equal(u_only, u), (wch, ich, g)
                none, b_only = _uncertainty(pd, wd, imd, g, want_u=False)
                assert none is None and torch.equal(b_only, bricks), (wch, ich, g)
                u2, b2 = _uncertainty(pd, wd, imd, g)                                      # a repeated launch
                assert torch.equal(u2, u) and torch.equal(b2, bricks), (wch, ich, g)


@pytest.mark.parametrize('shape,xs', (((128, 128, 129), 128), ((128, 128, 257), 256), ((128, 128, 272), 256)))
def test_uncertainty_volume_on_wide_runs(shape, xs):
    """Volumes of 2048 brick runs at brick 4: the launch keeps runs of 128 and 256 voxels (it halves them, down to 64, only while the grid
    has fewer workgroups than that); the last run holds a single voxel, or 16 (rows of whole 16-byte slots: the staging's aligned path).  The larger bricks take runs of 64 on the same volumes."""
    pred, weight, image = random_pred(shape, 2, 1), _sparse(shape, 1, 2, 0.7), _sparse(shape, 1, 3, 0.2)
    assert (shape[0] // 4) * (shape[1] // 4) * -(-shape[2] // xs) == 2048
    pd, wd, imd = (torch.tensor(t).cuda() for t in (pred, weight, image))
    for w, wdev, im, imdev in ((None, None, None, None), (weight, wd, image, imd)):
        want = pr.uncertainty(pred, w, im)
        for g in pr.BRICKS:
            u, bricks = _uncertainty(pd, wdev, imdev, g)
            assert np.array_equal(u.cpu().numpy(), want), g
            assert np.array_equal(bricks.cpu().numpy().astype(np.int64), pr.brick_sums(want, g).astype(np.int64)), g


def test_uncertainty_volume_on_an_unaligned_volume():
    """Volumes that start at an odd byte: the 16-byte grid of the loads is the address's, not the row's."""
    shape, C = (9, 10, 13), 3
    pred, weight, image = random_pred(shape, C, 2), _sparse(shape, 2, 3, 0.7), _sparse(shape, 1, 4, 0.2)
    want = pr.uncertainty(pred, weight, image)
    shifted = lambda a, by: offset_copy(torch.tensor(a).cuda(), by)
    for by in (1, 7, 15):
        u, bricks = _uncertainty(shifted(pred, by), shifted(weight, (by + 3) % 16), shifted(image, (by + 6) % 16), 4)
        assert np.array_equal(u.cpu().numpy(), want), by
        assert np.array_equal(bricks.cpu().numpy().astype(np.int64), pr.brick_sums(want, 4).astype(np.int64)), by


# ---- plane scores ----------------------------------------------------------------------------------------------------------
SCORE_VOLUMES = ((20, 24, 28), (17, 31, 22))
WIDTHS = (13, 16, 70)


def _geometries(shape):
    """name -> (a, b, origin)."""
    c = np.array([s // 2 for s in shape], dtype=float)
    g = {f'axes {p}': (E[p[0]], E[p[1]], c) for p in ((1, 2), (2, 1), (0, 2), (0, 1), (2, 0), (1, 0))}
    s = random_slicer(shape, 3)
    o = np.asarray(s.origin, dtype=float)
    for axis, (a, b) in enumerate(((s.v, s.w), (s.u, s.w), (s.u, s.v))):
        g[f'random {axis}'] = (np.asarray(a, float), np.asarray(b, float), o)
    a, b, _ = g['random 0']
    g['mostly outside'] = (np.array([0.6, 0.8, 0.0]), E[2], np.array([-1.5, shape[1] / 2, shape[2] - 3.0]))    # z >= 0 from r_i = 3, x <= dim - 1 up to r_j = 2
    g['outside'] = (a, b, np.array([-100.0, 5.0, 400.0]))
    g['half-integer'] = (E[1], E[2], c + 0.5)
    g['half-integer, one axis'] = (E[2], E[0], c + np.array([0.0, 0.5, 0.0]))
    g['faces'] = (E[1], E[2], np.array([0.0, shape[1] - 1.0, shape[2] - 1.0]))           # samples exactly on z = 0 and y, x = dim - 1
    g['top face'] = (E[1], E[2], np.array([shape[0] - 1.0, 6.0, 6.0]))
    return g


def _scores(ud, planes, sw, slack=0):
    from interactive_unet import _native as nv
    planes = np.ascontiguousarray(planes, dtype=np.float64).reshape(-1, 9)
    P = planes.shape[0]
    gd = torch.from_numpy(planes).cuda()
    need = nv.lib().iunet_plane_scores_ws_bytes(P, sw)
    ws = torch.empty(need + slack, dtype=torch.uint8, device='cuda')
    out = torch.full((P, 2), -7, dtype=torch.int64, device='cuda')
    nv.call('iunet_plane_scores', nv.ptr(ud), ud.shape[0], ud.shape[1], ud.shape[2], nv.ptr(gd), P, sw, pr.default_start(sw), nv.ptr(ws),
            need + slack, nv.ptr(out), nv.stream())
    return out.cpu().numpy()


@pytest.mark.parametrize('shape', SCORE_VOLUMES)
def test_plane_scores_are_the_definition(shape):
    from interactive_unet import _native as nv
    u = np.random.default_rng(shape[0]).integers(0, 256, shape, dtype=np.uint8)
    ud = torch.tensor(u).cuda()
    geoms = _geometries(shape)
    planes = np.array([np.stack(g) for g in geoms.values()])
    for sw in WIDTHS:
        want = pr.score_planes(u, planes, sw)
        got = _scores(ud, planes, sw)
        assert got.dtype == np.int64 and np.array_equal(got, want), sw
        assert np.array_equal(_scores(ud, planes, sw, slack=24), want), sw                 # a repeated launch, a larger workspace
        names = list(geoms)
        assert want[names.index('outside')].tolist() == [0, 0]
        assert 0 < want[names.index('mostly outside')][1] < 0.5 * sw * sw
        if sw == 13:
            assert want[names.index('faces')][1] == 7 * 7 and want[names.index('half-integer')][1] == 13 * 13
        for k, name in enumerate(names):
            assert np.array_equal(_scores(ud, planes[k:k + 1], sw), want[k:k + 1]), (name, sw)          # each alone: P = 1
            # the score is the sum of the slab gather's single plane at order 0
            a, b, o = geoms[name]
            slab = torch.empty((1, sw, sw), dtype=torch.uint8, device='cuda')
            nv.call('iunet_slab_gather', nv.ptr(ud), shape[0], shape[1], shape[2], (ctypes.c_double * 12)(*a, *b, *np.cross(a, b), *o), 1, sw,
                    pr.default_start(sw), 0, 0, nv.ptr(slab), nv.stream())
            assert int(slab.sum(dtype=torch.int64)) == want[k][0], (name, sw)
    # many planes in one launch: the geometries again, origins jittered
    rng = np.random.default_rng(1)
    many = np.array([planes[k % len(planes)] for k in range(300)])
    many[:, 2] += rng.uniform(-2, 2, (300, 3))
    for sw in (16, 70):
        assert np.array_equal(_scores(ud, many, sw), pr.score_planes(u, many, sw)), sw


def test_plane_scores_count_the_slab_gathers_samples():
    """plane_scores applies the plane point, the inside test and the order-0 sample of csrc/volume_rules.h as slab_gather does: on a
    volume without zero bytes its (score, inside) is the sum and the number of non-zero bytes of that plane."""
    from tests import test_gpu_slab as ts
    shape, sw = ts.SAMPLER_SHAPE, ts.SAMPLER_WIDTH
    u = ts._volume(shape, 3)
    assert u.all() and pr.default_start(sw) == ts.sr.default_start(sw)
    ud = torch.tensor(u).cuda()
    for name in ts.SAMPLER_GEOMETRIES:
        a, b, n, o = ts._geometries(shape)[name]
        plane = ts._gather(ud, (a, b, n, o), 1, sw, 0)[0]
        got = _scores(ud, np.stack([a, b, o])[None], sw)
        assert got.tolist() == [[int(plane.sum(dtype=torch.int64)), int((plane != 0).sum())]] and 0 < got[0, 1] < sw * sw, name


# ---- the host layer end to end ---------------------------------------------------------------------------------------------
BLOB_SHAPE, BLOB_CENTRE, BLOB_RADIUS = (32, 40, 48), (20, 12, 30), 5
BLOB_KW = dict(slice_width=16, brick=8, candidates=4, orientations=4)


def _blob():
    z, y, x = np.meshgrid(*[np.arange(n) for n in BLOB_SHAPE], indexing='ij')
    ball = (z - BLOB_CENTRE[0]) ** 2 + (y - BLOB_CENTRE[1]) ** 2 + (x - BLOB_CENTRE[2]) ** 2 <= BLOB_RADIUS ** 2
    pred = np.zeros(BLOB_SHAPE + (2,), dtype=np.uint8)
    pred[..., 0] = 255
    pred[ball] = (128, 127)
    return pred, np.where(ball, 255, 0).astype(np.uint8)


def _gen(seed=11):
    return torch.Generator().manual_seed(seed)


def _same(p, q):
    return (len(p) == len(q) and all(set(f) == set(h) == {'rot_vec', 'origin', 'score', 'inside', 'sampling_axis'} and
                                     np.array_equal(f['rot_vec'], h['rot_vec']) and np.array_equal(f['origin'], h['origin']) and
                                     (f['score'], f['inside'], f['sampling_axis']) == (h['score'], h['inside'], h['sampling_axis'])
                                     for f, h in zip(p, q)))


def test_host_layer_on_the_planted_blob():
    from interactive_unet import propose
    from interactive_unet.slicer import Slicer
    pred, weight = _blob()
    pd, wd = torch.tensor(pred).cuda(), torch.tensor(weight).cuda()
    image = _sparse(BLOB_SHAPE, 1, 3, 0.3)[..., 0]
    imd = torch.tensor(image).cuda()
    for g in pr.BRICKS:
        u, bricks = propose.uncertainty(pd, image=imd, brick=g)
        un, bn = propose.uncertainty(pred, image=image, brick=g)
        assert u.is_cuda and u.dtype == torch.uint8 and bricks.is_cuda and np.array_equal(u.cpu().numpy(), un)
        assert np.array_equal(bricks.cpu().numpy().astype(np.int64), bn.astype(np.int64)) and bn.any()
        assert np.array_equal(propose.candidate_origins(bricks, g, BLOB_SHAPE, 6), propose.candidate_origins(bn, g, BLOB_SHAPE, 6))
    planes = np.array([[E[1], E[2], [20.0, 12.0, 30.0]], [E[0], E[2], [19.5, 11.5, 27.5]]])
    got = propose.score_planes(u, planes, 16)
    assert got.is_cuda and got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), propose.score_planes(un, planes, 16))
    for kw in (dict(), dict(image=(imd, image)), dict(sampling_mode='grid'), dict(sampling_mode='grid', sampling_axis='z', axis=2)):
        dev_kw = {k: (v[0] if isinstance(v, tuple) else v) for k, v in kw.items()}
        host_kw = {k: (v[1] if isinstance(v, tuple) else v) for k, v in kw.items()}
        found = propose.propose_slices(BLOB_SHAPE, pd, generator=_gen(), **BLOB_KW, **dev_kw)
        assert found and found[0]['score'] > 0 and _same(found, propose.propose_slices(BLOB_SHAPE, pred, generator=_gen(), **BLOB_KW, **host_kw)), kw
    assert propose.propose_slices(BLOB_SHAPE, pd, weight=wd, generator=_gen(), **BLOB_KW) == []
    s, t = Slicer(list(BLOB_SHAPE)), Slicer(list(BLOB_SHAPE))
    assert _same(propose.next_slice(s, pd, generator=_gen(), **BLOB_KW), propose.next_slice(t, pred, generator=_gen(), **BLOB_KW))
    assert np.array_equal(s.u, t.u) and np.array_equal(s.w, t.w) and np.array_equal(s.origin, t.origin)
    for bad in (dict(weight=weight), dict(image=wd.cpu()), dict(weight=wd[:, :, ::2]), dict(weight=wd.float())):        # mixed, host, strided, dtype
        with pytest.raises(ValueError):
            propose.uncertainty(pd, **bad)
    with pytest.raises(ValueError):
        propose.score_planes(u[:, :, ::2], planes, 16)


def test_host_layer_on_a_real_prediction():
    from interactive_unet import predict, propose
    from interactive_unet.slicer import Slicer
    from interactive_unet.unet import UNet
    from oracle import unet_ref
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = UNet(dim=3, levels=4, base=32, pretrained=False, infer_dtype='fp16')
    m.load_named(unet_ref.init_params(dim=3, levels=4, base=32, seed=3, randomize_bn=True))
    m = m.cuda().eval()
    shape = (32, 32, 32)
    vol = np.random.default_rng(5).integers(0, 256, shape, dtype=np.uint8)
    pd = predict.predict_volume_array(m, torch.tensor(vol).cuda(), input_size=32, num_classes=2)
    pred = pd.cpu().numpy()
    assert pd.shape == shape + (2,) and pred.max(-1).min() >= 15                        # predicted everywhere: the largest byte is >= 255 / 16
    kw = dict(slice_width=32, brick=8, candidates=8, orientations=4)
    found = propose.propose_slices(shape, pd, generator=_gen(5), **kw)
    assert len(found) == 32 and found[0]['score'] > 0
    assert _same(found, propose.propose_slices(shape, pred, generator=_gen(5), **kw))
    # the overlay of the best axis-aligned plane: get_slice(u, order=0) shows the proposal's uncertainty.  Width 64 in a 32^3 volume: the
    # plane leaves the volume along both of its axes, so get_slice's crop ends at the volume's faces and cuts nothing the score counts.
    s = Slicer(list(shape))
    found = propose.next_slice(s, pd, slice_width=64, brick=8, candidates=8, sampling_mode='grid', sampling_axis='x')
    assert len(found) == 8 and s.sampling_axis == 'x' and found[0]['inside'] == 31 * 31                # (a full brick's centre is a half-integer: 31 samples per axis)
    u, _ = propose.uncertainty(pd)
    shown = s.get_slice(u, slice_width=64, order=0)
    assert shown.is_cuda and int(shown.sum(dtype=torch.int64)) == found[0]['score'] > 0
    assert int(s.get_slice(u.cpu().numpy(), slice_width=64, order=0).astype(np.int64).sum()) == found[0]['score']
