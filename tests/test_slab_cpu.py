"""The oblique slab without a GPU: the definition tests/slab_ref.py against the slicer's own plane, plain
crops and Slicer.get_slice; the paste's coverage; the host layer's numpy path, boxes and refusals; the entry points' argument checks."""
import ctypes
import os
import warnings

import numpy as np
import pytest

from tests import slab_ref as sr

SHAPE = (40, 48, 56)
E = np.eye(3)


def _volume(shape=SHAPE, seed=5):
    return np.random.default_rng(seed).integers(1, 256, shape, dtype=np.uint8)       # no zeros: a zero is a sample outside


def _slicer(seed, shape=SHAPE):
    """A random orientation with the origin within +-3 voxels of the centre (np.random.seed(seed), randomize(), then the origin)."""
    from interactive_unet.slicer import Slicer
    np.random.seed(seed)
    s = Slicer(list(shape))
    s.randomize()
    s.origin = np.array(shape) / 2 + np.random.uniform(-3, 3, 3)
    return s


@pytest.mark.parametrize('seed', range(4))
def test_centre_plane_coordinates_are_the_slicers(seed):
    s = _slicer(seed)
    for axis in range(3):
        for T, sw in ((8, 24), (5, 13), (1, 7)):
            c = sr.coords(sr.slicer_geometry(s, axis), T, sw)
            assert c.shape == (3, T, sw, sw) and c.dtype == np.float64
            assert np.array_equal(c[:, T // 2], s.get_interpolation_coords(slice_width=sw)[axis]), (axis, T, sw)
            assert np.array_equal(s.get_slab_coords(axis, sw, T), c), (axis, T, sw)


def test_axis_aligned_slab_is_the_plain_crop():
    vol = _volume()
    o, T, sw = np.array([20.0, 24.0, 28.0]), 8, 16
    z0, y0, x0 = 20 - 4, 24 - 8, 28 - 8
    crops = {(1, 2, 0): vol[z0:z0 + T, y0:y0 + sw, x0:x0 + sw],                                 # (a, b, n) as axis numbers
             (2, 1, 0): vol[z0:z0 + T, y0:y0 + sw, x0:x0 + sw].transpose(0, 2, 1),
             (0, 2, 1): vol[20 - 8:20 + 8, 24 - 4:24 + 4, x0:x0 + sw].transpose(1, 0, 2),
             (0, 1, 2): vol[20 - 8:20 + 8, y0:y0 + sw, 28 - 4:28 + 4].transpose(2, 0, 1)}
    for (ia, ib, inn), want in crops.items():
        for order in (0, 1):
            got = sr.gather(vol, (E[ia], E[ib], E[inn], o), T, sw, order)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (ia, ib, inn, order)


@pytest.mark.parametrize('order', (0, 1))
def test_centre_plane_against_get_slice(order):
    """get_slice samples the bounding-box crop volume[lo:hi], hi = ceil(max coordinate): every pixel with a coordinate above hi - 1
    comes out 0 there.  The slab keeps the real bytes on those and equals get_slice on all the others.  (Cut pixels at slice width 24
    for seeds 0 .. 3: 19, 13, 42, 66 of 576.)"""
    vol = _volume()
    for seed in range(4):
        s = _slicer(seed)
        T, sw = 8, 24
        c = sr.coords(sr.slicer_geometry(s, 0), T, sw)[:, T // 2]
        hi = np.minimum(np.ceil(c.max(axis=(1, 2))).astype(int), np.array(SHAPE))
        kept = np.all(c <= (hi - 1)[:, None, None], axis=0)
        mine = sr.gather(vol, sr.slicer_geometry(s, 0), T, sw, order)[T // 2]
        ref = s.get_slice(vol, axis=0, slice_width=sw, order=order)
        print(f'seed {seed}, order {order}: {int((~kept).sum())} of {kept.size} pixels cut by the crop')
        assert np.array_equal(mine[kept], ref[kept])
        assert not ref[~kept].any()
        assert (~kept).sum() <= 0.15 * kept.size
        assert mine[~kept].all()                                                    # inside the volume: the real (non-zero) bytes
        # the plane leaves the volume: hi is the shape, the crop's cut is the volume's own edge
        wide = sr.gather(vol, sr.slicer_geometry(s, 0), T, 64, order)[T // 2]
        assert np.array_equal(wide, s.get_slice(vol, axis=0, slice_width=64, order=order))
        assert not wide.all() and wide.any()


def _random_probs(T, sw, C, seed=0):
    return np.random.default_rng(seed).random((T, sw, sw, C), dtype=np.float32)


def test_quantize_truncates_the_fp32_product():
    p = np.array([0.0, 1.0, 0.5, 1 / 255, np.float32(0.99999994), 0.2], dtype=np.float32)
    assert sr.quantize(p).tolist() == [0, 255, 127, 1, 254, 51]


@pytest.mark.parametrize('seed,k_lo,k_hi,border', [(0, 0, 8, 0), (1, 2, 6, 4), (2, 3, 4, 7), (3, 0, 5, 1)])
def test_paste_covers_the_kept_region_exactly_once(seed, k_lo, k_hi, border):
    """Independent statement of the kept region: a voxel belongs to it iff, among the samples of the slab extended by a ring of two
    samples on every side, the one nearest to it (Euclidean, the vectors being orthonormal) is a kept one."""
    shape, T, sw, C = (20, 24, 28), 8, 16, 2
    s = _slicer(seed, shape)
    geom = sr.slicer_geometry(s, seed % 3)
    probs = _random_probs(T, sw, C, seed)
    dest = np.full(shape + (C,), 7, dtype=np.uint8)
    out = sr.paste(dest, probs, geom, k_lo, k_hi, border)
    keep, k, i, j = sr.paste_indices(shape, geom, (0, 0, 0), shape, T, sw, k_lo, k_hi, border)
    # brute force over the extended lattice
    a, b, n, o = geom
    rk, ri = np.arange(-2, T + 2) + sr.default_start(T), np.arange(-2, sw + 2) + sr.default_start(sw)
    pts = (o + rk[:, None, None, None] * n + ri[None, :, None, None] * a + ri[None, None, :, None] * b).reshape(-1, 3)
    kk, ii, jj = [t.reshape(-1) for t in np.meshgrid(np.arange(-2, T + 2), np.arange(-2, sw + 2), np.arange(-2, sw + 2), indexing='ij')]
    vox = np.stack(np.meshgrid(*[np.arange(n_) for n_ in shape], indexing='ij'), -1).reshape(-1, 3).astype(float)
    near = (-2.0 * vox @ pts.T + (pts ** 2).sum(-1)[None]).argmin(1)                  # |vox - pts|^2 less the voxel's own |vox|^2
    want_keep = ((kk[near] >= k_lo) & (kk[near] < k_hi) & (ii[near] >= border) & (ii[near] < sw - border)
                 & (jj[near] >= border) & (jj[near] < sw - border)).reshape(shape)
    assert want_keep.any() and np.array_equal(keep, want_keep)
    # written exactly once, from the nearest sample; nothing else touched
    hits = np.zeros(shape, dtype=int)
    np.add.at(hits, np.nonzero(keep), 1)
    assert hits.max() == 1 and np.array_equal(hits == 1, keep)
    q = sr.quantize(probs)
    sel = near[keep.reshape(-1)]
    assert np.array_equal(out[keep], q[kk[sel], ii[sel], jj[sel]])
    assert (out[~keep] == 7).all()
    # the tight box of the host layer against the whole volume
    lo, length = s.slab_paste_box(shape, seed % 3, sw, T, (k_lo, k_hi), border)
    assert (lo >= 0).all() and (lo + length <= np.array(shape)).all()
    assert np.array_equal(sr.paste(dest, probs, geom, k_lo, k_hi, border, lo=lo, length=length), out)
    if border:
        assert np.prod(length) < np.prod(shape)


def test_paste_box_clips_and_may_be_empty():
    s = _slicer(0, (20, 24, 28))
    s.origin = np.array([200.0, 200.0, 200.0])
    lo, length = s.slab_paste_box((20, 24, 28), 0, 16, 8, (0, 8), 0)
    assert (length == 0).any() and (lo + length <= np.array([20, 24, 28])).all()
    dest = np.full((20, 24, 28, 2), 7, dtype=np.uint8)
    assert np.array_equal(sr.paste(dest, _random_probs(8, 16, 2), sr.slicer_geometry(s, 0)), dest)


@pytest.mark.parametrize('order', (0, 1))
def test_get_slab_numpy_path_is_the_restatement(order):
    vol = _volume()
    for seed in range(3):
        s = _slicer(seed)
        for axis in range(3):
            for T, sw in ((8, 24), (5, 13)):
                got = s.get_slab(vol, axis=axis, slice_width=sw, depth=T, order=order)
                assert got.dtype == np.uint8 and got.shape == (T, sw, sw)
                assert np.array_equal(got, sr.gather(vol, sr.slicer_geometry(s, axis), T, sw, order))
    with pytest.raises(ValueError):
        s.get_slab(vol, depth=0)


def _model(dim):
    from interactive_unet.unet import UNet
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return UNet(dim=dim, levels=4, base=32, pretrained=False)


def test_predict_slab_refusals_need_no_device():
    import torch
    from interactive_unet import predict
    from interactive_unet.slicer import Slicer
    s = Slicer([40, 48, 56])
    vol = torch.zeros((40, 48, 56), dtype=torch.uint8)
    with pytest.raises(ValueError, match='3-D network'):
        predict.predict_slab(_model(2), vol, s, slice_width=32, depth=8)
    m3 = _model(3)
    for T, S in ((12, 32), (8, 36), (0, 32), (4, 32)):
        with pytest.raises(ValueError, match='multiples of 8'):
            predict.predict_slab(m3, vol, s, slice_width=S, depth=T)
    for bad in (vol, vol.numpy(), vol.float(), vol[0]):                           # host tensors, arrays, other dtypes, other ranks
        with pytest.raises(ValueError, match='resident'):
            predict.predict_slab(m3, bad, s, slice_width=32, depth=8)
    with pytest.raises(ValueError, match='3-D network'):
        predict.predict_slice_3d(vol, s, slice_width=32, depth=8, model=_model(2))
    with pytest.raises(NotImplementedError):
        s.paste_slab(torch.zeros((8, 32, 32, 2)), torch.zeros((40, 48, 56, 2), dtype=torch.uint8))      # a host volume


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """Argument validation precedes every HIP call; a zero-length paste box is a no-op, not an error."""
    from interactive_unet import _native as nv
    if not os.path.isfile(nv.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    l = nv.lib()
    mem = (ctypes.c_double * 64)()
    buf = ctypes.c_void_p(ctypes.addressof(mem))                                      # never dereferenced: every call below stops before its launch
    geom = (ctypes.c_double * 12)(0, 1, 0, 0, 0, 1, 1, 0, 0, 4, 4, 4)

    def gather(vol=buf, Z=8, Y=8, X=8, g=geom, T=4, sw=8, order=1, out=buf):
        return l.iunet_slab_gather(vol, Z, Y, X, g, T, sw, -4, -2, order, out, None), l.iunet_last_error()
    for kw, word in ((dict(vol=None), b'null'), (dict(g=None), b'null'), (dict(out=None), b'null'), (dict(order=2), b'order'),
                     (dict(order=-1), b'order'), (dict(T=0), b'bad slab'), (dict(sw=0), b'bad slab'), (dict(T=65536), b'grid'),
                     (dict(sw=4 * 65535 + 1), b'grid'), (dict(Z=1 << 14, Y=1 << 14, X=1 << 14), b'volume'), (dict(Z=0), b'volume')):
        rc, msg = gather(**kw)
        assert rc < 0 and word in msg, (kw, msg)

    def paste(vol=buf, Z=8, Y=8, X=8, C=2, g=geom, lo=(0, 0, 0), ln=(8, 8, 8), probs=buf, T=4, sw=8, k_lo=0, k_hi=4, border=0):
        return (l.iunet_slab_paste(vol, Z, Y, X, C, g, nv.int_array(lo), nv.int_array(ln), probs, T, sw, -4, -2, k_lo, k_hi, border, None),
                l.iunet_last_error())
    for kw, word in ((dict(vol=None), b'null'), (dict(g=None), b'null'), (dict(probs=None), b'null'), (dict(T=0), b'bad slab'),
                     (dict(sw=0), b'bad slab'), (dict(C=0), b'classes'), (dict(C=17), b'classes'), (dict(Z=1 << 14, Y=1 << 14, X=1 << 14), b'volume'),
                     (dict(k_lo=2, k_hi=2), b'plane range'), (dict(k_hi=5), b'plane range'), (dict(k_lo=-1), b'plane range'),
                     (dict(border=4), b'border'), (dict(border=-1), b'border'), (dict(lo=(0, 0, 1)), b'box outside'),
                     (dict(lo=(-1, 0, 0)), b'box outside'), (dict(ln=(8, 9, 8)), b'box outside'), (dict(ln=(8, -1, 8)), b'box outside'),
                     (dict(Z=70000, ln=(65536, 8, 8)), b'grid')):
        rc, msg = paste(**kw)
        assert rc < 0 and word in msg, (kw, msg)
    assert l.iunet_slab_paste(buf, 8, 8, 8, 2, geom, None, nv.int_array((8, 8, 8)), buf, 4, 8, -4, -2, 0, 4, 0, None) < 0
    for ln in ((0, 8, 8), (8, 0, 8), (8, 8, 0), (0, 0, 0)):
        assert paste(ln=ln)[0] == 0, ln
