"""The oblique slab on the device: iunet_slab_gather and iunet_slab_paste bit for bit against the definition
tests/slab_ref.py, and the host layer on top of them -- Slicer.get_slab / paste_slab, predict.predict_slab, predict_slice_3d,
update_predicted_volume -- with the 3-D net."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import slab_ref as sr
from tests.volume_inputs import random_slicer

E = np.eye(3)
VOLUMES = ((20, 24, 28), (17, 31, 22))
SLABS = ((8, 16), (5, 13))


def _volume(shape, seed):
    return np.random.default_rng(seed).integers(1, 256, shape, dtype=np.uint8)       # no zeros: a zero is a sample outside


def _geom12(geom):
    return (ctypes.c_double * 12)(*[float(t) for v in geom for t in v])


def _slice_plane(vd, geom, sw, order):
    """iunet_slice_gather's plane of (a, b, origin) with the whole volume as its crop box."""
    from interactive_unet import _native as nv
    a, b, _, o = geom
    plane = torch.full((sw, sw), 55, dtype=torch.uint8, device='cuda')
    nv.call('iunet_slice_gather', nv.ptr(vd), vd.shape[0], vd.shape[1], vd.shape[2], (ctypes.c_double * 9)(*a, *b, *o), nv.int_array((0, 0, 0)),
            nv.int_array(vd.shape), sw, sr.default_start(sw), order, nv.ptr(plane), nv.stream())
    return plane


def _gather(vd, geom, T, sw, order):
    from interactive_unet import _native as nv
    out = torch.empty((T, sw, sw), dtype=torch.uint8, device='cuda')
    nv.call('iunet_slab_gather', nv.ptr(vd), vd.shape[0], vd.shape[1], vd.shape[2], _geom12(geom), T, sw, sr.default_start(sw),
            sr.default_start(T), order, nv.ptr(out), nv.stream())
    return out


def _geometries(shape):
    """name -> (a, b, n, origin)."""
    c = np.array([s // 2 for s in shape], dtype=float)
    g = {f'axes {p}': (E[p[0]], E[p[1]], E[p[2]], c) for p in ((1, 2, 0), (2, 1, 0), (0, 2, 1), (0, 1, 2), (2, 0, 1), (1, 0, 2))}
    s = random_slicer(shape, 3)
    for axis in range(3):
        g[f'random {axis}'] = sr.slicer_geometry(s, axis)
    a, b, n, o = g['random 0']
    g['mostly outside'] = (a, b, n, np.array([-3.0, shape[1] / 2, shape[2] / 2]))
    g['outside'] = (a, b, n, np.array([-100.0, 5.0, 400.0]))
    g['half-integer'] = (E[1], E[2], E[0], c + 0.5)
    g['half-integer, one axis'] = (E[2], E[0], E[1], c + np.array([0.0, 0.5, 0.0]))
    g['edge'] = (E[1], E[2], E[0], np.array([0.0, shape[1] - 1.0, shape[2] - 1.0]))      # the planes z = 0 and x, y = dim - 1 exactly
    return g


@pytest.mark.parametrize('shape', VOLUMES)
def test_gather_is_the_restatement(shape):
    vol = _volume(shape, 1)
    vd = torch.tensor(vol).cuda()
    for name, geom in _geometries(shape).items():
        for T, sw in SLABS:
            for order in (0, 1):
                want = sr.gather(vol, geom, T, sw, order)
                got = _gather(vd, geom, T, sw, order)
                again = _gather(vd, geom, T, sw, order)
                assert np.array_equal(got.cpu().numpy(), want), (name, T, sw, order)
                assert torch.equal(got, again), (name, T, sw, order)
                if name == 'outside':
                    assert not want.any()
                if name == 'mostly outside':
                    assert 0.5 < (want == 0).mean() < 1.0
                if name.startswith('random') and (T, sw) == (5, 13) and shape == VOLUMES[0]:
                    assert want.all()                                               # fully inside
                if name.startswith('axes') and order == 1:
                    assert np.array_equal(want, sr.gather(vol, geom, T, sw, 0))
                # the centre plane is iunet_slice_gather's with the whole volume as its crop box
                assert torch.equal(got[T // 2], _slice_plane(vd, geom, sw, order)), (name, T, sw, order)


SAMPLER_SHAPE, SAMPLER_WIDTH = (9, 17, 70), 70           # two ragged 64-lane groups per row of samples
SAMPLER_GEOMETRIES = ('random 0', 'half-integer', 'edge', 'mostly outside')


def test_the_sampler_is_one_rule_for_slab_and_slice():
    """The plane point, the inside test and the order-0 / order-1 samplers are written once (csrc/volume_rules.h): slab_gather (64 lanes
    along j, 4 rows per workgroup, the whole volume) and slice_gather (16 x 16 tiles, a crop that is the whole volume) give the same bytes."""
    shape, sw = SAMPLER_SHAPE, SAMPLER_WIDTH
    vol = _volume(shape, 3)
    assert vol.all() and sr.default_start(1) == 0
    vd = torch.tensor(vol).cuda()
    for name in SAMPLER_GEOMETRIES:
        geom = _geometries(shape)[name]
        for order in (0, 1):
            slab = _gather(vd, geom, 1, sw, order)[0]
            assert torch.equal(slab, _slice_plane(vd, geom, sw, order)), (name, order)
            assert np.array_equal(slab.cpu().numpy(), sr.gather(vol, geom, 1, sw, order)[0]), (name, order)
            assert 0 < int((slab != 0).sum()) < sw * sw, (name, order)        # the plane is wider than the volume: samples on both sides of its faces


def test_get_slab_on_a_resident_volume():
    shape = VOLUMES[0]
    vol = _volume(shape, 2)
    vd = torch.tensor(vol).cuda()
    s = random_slicer(shape, 5)
    for axis in range(3):
        for order in (0, 1):
            got = s.get_slab(vd, axis=axis, slice_width=16, depth=8, order=order)
            assert got.is_cuda and got.dtype == torch.uint8
            assert np.array_equal(got.cpu().numpy(), sr.gather(vol, sr.slicer_geometry(s, axis), 8, 16, order))
            assert np.array_equal(got.cpu().numpy(), s.get_slab(vol, axis=axis, slice_width=16, depth=8, order=order))
    with pytest.raises(NotImplementedError):
        s.get_slab(vd, order=3)
    with pytest.raises(NotImplementedError):
        s.get_slab(vd.float())


def _probs(T, sw, C, seed):
    p = np.random.default_rng(seed).random((T, sw, sw, C), dtype=np.float32)
    p[0, 0, 0], p[-1, -1, -1], p[T // 2, sw // 2, sw // 2] = 0.0, 1.0, 1.0 / 255
    return p


def _pattern(shape, C):
    z, y, x, c = np.meshgrid(*[np.arange(n) for n in shape + (C,)], indexing='ij')
    return ((7 * z + 3 * y + x + 11 * c) % 251).astype(np.uint8)


@pytest.mark.parametrize('C', (2, 5))
@pytest.mark.parametrize('shape', VOLUMES)
def test_paste_is_the_restatement(shape, C):
    from interactive_unet import _native as nv
    from interactive_unet.slicer import Slicer
    dest = _pattern(shape, C)
    for name, geom in _geometries(shape).items():
        if name == 'outside' or name.startswith('axes (2') or name.startswith('axes (1, 0'):
            continue
        for T, sw in SLABS:
            probs = _probs(T, sw, C, T + C)
            pd = torch.tensor(probs).cuda()
            for k_lo, k_hi, border in ((0, T, 0), (1, T - 2, 3), (T // 2, T // 2 + 1, (sw - 1) // 2)):
                want = sr.paste(dest, probs, geom, k_lo, k_hi, border)
                # the host layer's tight box, through a slicer that carries this geometry
                s = Slicer(list(shape))
                a, b, n, o = geom
                s.u, s.v, s.w, s.origin = n, a, b, o                             # axis 0: plane vectors (v, w), normal u
                tight = s.slab_paste_box(shape, 0, sw, T, (k_lo, k_hi), border)
                for lo, length in (((0, 0, 0), shape), tight):
                    vd = torch.tensor(dest).cuda()
                    nv.call('iunet_slab_paste', nv.ptr(vd), shape[0], shape[1], shape[2], C, _geom12(geom), nv.int_array(lo),
                            nv.int_array(length), nv.ptr(pd), T, sw, sr.default_start(sw), sr.default_start(T), k_lo, k_hi, border,
                            nv.stream())
                    assert np.array_equal(vd.cpu().numpy(), want), (name, T, sw, k_lo, k_hi, border, tuple(lo))
                vd = torch.tensor(dest).cuda()
                assert s.paste_slab(pd, vd, axis=0, planes=(k_lo, k_hi), border=border) is vd
                assert np.array_equal(vd.cpu().numpy(), want), (name, T, sw, k_lo, k_hi, border)
                if name == 'random 0' and border == 0:
                    assert (want != dest).any()


def test_paste_bytes_are_normalize_quantize_at_weight_one():
    from interactive_unet import _native as nv
    shape, T, sw, C = VOLUMES[0], 8, 16, 2
    probs = _probs(T, sw, C, 9)
    pd = torch.tensor(probs).cuda()
    ones = torch.ones(T * sw * sw, dtype=torch.float32, device='cuda')
    q = torch.empty((T, sw, sw, C), dtype=torch.uint8, device='cuda')
    nv.call('iunet_normalize_quantize', nv.ptr(pd), nv.ptr(ones), nv.ptr(q), T * sw * sw, C, 1e-3, nv.stream())
    q = q.cpu().numpy()
    assert np.array_equal(q, sr.quantize(probs))
    geom = (E[1], E[2], E[0], np.array([s // 2 for s in shape], dtype=float))
    vd = torch.zeros(shape + (C,), dtype=torch.uint8, device='cuda')
    nv.call('iunet_slab_paste', nv.ptr(vd), shape[0], shape[1], shape[2], C, _geom12(geom), nv.int_array((0, 0, 0)),
            nv.int_array(shape), nv.ptr(pd), T, sw, sr.default_start(sw), sr.default_start(T), 0, T, 0, nv.stream())
    z0, y0, x0 = shape[0] // 2 - 4, shape[1] // 2 - 8, shape[2] // 2 - 8
    assert np.array_equal(vd.cpu().numpy()[z0:z0 + T, y0:y0 + sw, x0:x0 + sw], q)


# ---- end to end with the 3-D net ------------------------------------------------------------------------------------------
VSHAPE = (24, 40, 44)


@pytest.fixture(scope='module')
def model():
    from interactive_unet.unet import UNet
    from oracle import unet_ref
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = UNet(dim=3, levels=4, base=32, pretrained=False)
    m.load_named(unet_ref.init_params(dim=3, levels=4, base=32, seed=3, randomize_bn=True))
    return m.cuda().eval()


def _infer(eng, slab):
    """The engine's forward on slab bytes, in predict_slab's output layout."""
    T, S, C = slab.shape[0], slab.shape[1], eng.ncls
    vox = T * S * S
    probs = torch.empty((T, S, S, C), dtype=torch.float32, device='cuda')
    cls = torch.empty((T, S, S), dtype=torch.uint8, device='cuda')
    eng.infer(slab.contiguous(), (vox, vox, S * S, S, 1), 1, T, S, S, probs=probs, cls=cls, out_strides=(vox * C, 1, S * S * C, S * C, C))
    return cls, probs


@pytest.mark.parametrize('T,S', ((8, 32), (16, 16)))
def test_predict_slab_is_the_engines_forward_on_the_slab(model, T, S):
    from interactive_unet import predict
    from interactive_unet.slicer import Slicer
    vol = _volume(VSHAPE, 4)
    vd = torch.tensor(vol).cuda()
    s = random_slicer(VSHAPE, 6)
    for axis, order in ((0, 1), (2, 0)):
        slab, cls, probs = predict.predict_slab(model, vd, s, slice_width=S, depth=T, axis=axis, order=order)
        assert slab.shape == (T, S, S) and slab.dtype == torch.uint8 and cls.shape == (T, S, S) and cls.dtype == torch.uint8
        assert probs.shape == (T, S, S, 2) and probs.dtype == torch.float32 and slab.is_cuda and cls.is_cuda and probs.is_cuda
        want = sr.gather(vol, sr.slicer_geometry(s, axis), T, S, order)
        assert np.array_equal(slab.cpu().numpy(), want)
        cls2, probs2 = _infer(model.engine('eval'), torch.tensor(want).cuda())
        assert torch.equal(probs, probs2) and torch.equal(cls, cls2)
        assert (probs.sum(-1) - 1).abs().max().item() < 1e-5
    # an axis-aligned slab inside the volume is the plain crop
    s = Slicer(list(VSHAPE))
    s.u, s.v, s.w = E[0], E[1], E[2]
    s.origin = np.array([12.0, 20.0, 22.0])
    z0, y0, x0 = 12 - T // 2, 20 - S // 2, 22 - S // 2
    crop = vd[z0:z0 + T, y0:y0 + S, x0:x0 + S]
    slab, cls, probs = predict.predict_slab(model, vd, s, slice_width=S, depth=T)
    assert torch.equal(slab, crop)
    cls2, probs2 = _infer(model.engine('eval'), crop)
    assert torch.equal(probs, probs2) and torch.equal(cls, cls2)


def test_predict_slice_3d_from_a_checkpoint(model, tmp_path, monkeypatch):
    from interactive_unet import predict
    monkeypatch.chdir(tmp_path)
    os.makedirs('model')
    model.save_checkpoint(os.path.join('model', 'model.ckpt'))
    T, S = 8, 32
    vd = torch.tensor(_volume(VSHAPE, 4)).cuda()
    s = random_slicer(VSHAPE, 7)
    _, cls, probs = predict.predict_slab(model, vd, s, slice_width=S, depth=T)
    rgb = predict.predict_slice_3d(vd, s, slice_width=S, depth=T)
    assert isinstance(rgb, np.ndarray) and rgb.shape == (S, S, 3) and rgb.dtype == np.uint8
    mid = cls[T // 2].cpu().numpy()
    assert np.array_equal(rgb, predict.COLORS[mid + 1])
    assert len(np.unique(mid)) == 2                                                # both colours occur: the comparison says something
    pr = predict.predict_slice_3d(vd, s, slice_width=S, depth=T, return_probabilities=True, model=model)
    assert pr.shape == (1, S, S, 2) and np.array_equal(pr[0], probs[T // 2].cpu().numpy())
    with pytest.raises(ValueError):
        predict.predict_slice_3d(vd, s, slice_width=S, depth=12, model=model)


def test_update_predicted_volume_pastes_the_core(model):
    from interactive_unet import predict
    T, S, C = 8, 32, 2
    vd = torch.tensor(_volume(VSHAPE, 4)).cuda()
    s = random_slicer(VSHAPE, 8)
    _, _, probs = predict.predict_slab(model, vd, s, slice_width=S, depth=T, axis=1)
    dest = _pattern(VSHAPE, C)
    geom = sr.slicer_geometry(s, 1)
    for kw, (margin, border) in ((dict(), (T // 4, S // 4)), (dict(margin=0, border=0), (0, 0)), (dict(margin=3, border=5), (3, 5))):
        pred = torch.tensor(dest).cuda()
        assert predict.update_predicted_volume(pred, probs, s, axis=1, **kw) is pred
        want = sr.paste(dest, probs.cpu().numpy(), geom, margin, T - margin, border)
        assert np.array_equal(pred.cpu().numpy(), want), kw
        assert (want != dest).any()
