"""Distance transform and ball morphology on the device: iunet_edt_sq, iunet_edt_sq_mask and iunet_edt_select bit
for bit against the definition tests/morphology_ref.py (single seeds against the closed form), and the host layer
interactive_unet/morphology.py end to end -- on random, sparse, planted and degenerate volumes, on a real prediction of the 3-D net, and
once at volume scale, where d2 passes 2^32 bytes.  Every comparison is exact equality."""
import functools
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import morphology_ref as mr
from tests.test_morphology_cpu import blobs, holes_volume, lattice_axis, sparse_input
from tests.volume_inputs import offset_copy, random_pred

# ragged; a row; flat; one voxel; one axis longer than any workgroup, in turn along the row and along either column
SHAPES = {'ragged': (37, 41, 150), 'row': (1, 1, 300), 'flat': (33, 2, 65), 'one voxel': (1, 1, 1), 'long x': (3, 5, 2100),
          'long y': (3, 2100, 5), 'long z': (2100, 3, 5)}
SHAPE_NAMES = tuple(SHAPES)
KINDS = ('p50', 'p01', 'none', 'all', 'plane', 'blobs')


@functools.lru_cache(maxsize=None)
def _volume(kind, name):
    shape = SHAPES[name]
    seed = SHAPE_NAMES.index(name)
    if kind == 'p50':
        v = (np.random.default_rng(seed).random(shape) < 0.5).astype(np.uint8)
    elif kind == 'p01':
        v = (np.random.default_rng(10 + seed).random(shape) < 0.01).astype(np.uint8)
    elif kind == 'sparse':
        assert shape == (37, 41, 150)
        v = sparse_input().astype(np.uint8)
    elif kind == 'none':
        v = np.zeros(shape, np.uint8)
    elif kind == 'all':
        v = np.ones(shape, np.uint8)
    elif kind == 'plane':
        v = np.zeros(shape, np.uint8)
        v[0] = 1
    elif kind == 'blobs':
        v = blobs(shape, 20 + seed)
    else:
        v = random_pred(shape, int(kind), 30 + seed)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _want(kind, name, target, invert):
    """The definition's d2, computed once and shared."""
    d = mr.distance_sq(_volume(kind, name), target, invert)
    d.setflags(write=False)
    return d


def _edt(srcd, target, invert, want_d2=True, want_cls=True):
    """The entry point itself; outputs and workspace start from a pattern, so an element left unwritten shows."""
    from interactive_unet import _native as nv
    Z, Y, X = srcd.shape[:3]
    C = 1 if srcd.ndim == 3 else srcd.shape[3]
    d2 = torch.full((Z, Y, X), -7, dtype=torch.int32, device='cuda') if want_d2 else None
    cls = torch.full((Z, Y, X), 77, dtype=torch.uint8, device='cuda') if want_cls else None
    ws_bytes = nv.lib().iunet_edt_ws_bytes(Z, Y, X)
    assert ws_bytes == (8 * Z * Y * X + 15) // 16 * 16
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device='cuda') if want_d2 else None
    nv.call('iunet_edt_sq', nv.ptr(srcd), Z, Y, X, C, target, int(invert), nv.ptr(d2), nv.ptr(cls), nv.ptr(ws), ws_bytes if want_d2 else 0,
            nv.stream())
    return d2, cls


def _mask(prevd, r2, above):
    from interactive_unet import _native as nv
    Z, Y, X = prevd.shape
    d2 = torch.full((Z, Y, X), -7, dtype=torch.int32, device='cuda')
    ws_bytes = nv.lib().iunet_edt_ws_bytes(Z, Y, X)
    ws = torch.full((ws_bytes,), 0x5A, dtype=torch.uint8, device='cuda')
    nv.call('iunet_edt_sq_mask', nv.ptr(prevd), Z, Y, X, r2, int(above), nv.ptr(d2), nv.ptr(ws), ws_bytes, nv.stream())
    return d2


def _select(d2d, clsd, r2, above, only, value, alias=False, out=None):
    from interactive_unet import _native as nv
    Z, Y, X = d2d.shape
    out = out if out is not None else clsd if alias else torch.full((Z, Y, X), 55, dtype=torch.uint8, device='cuda')
    nv.call('iunet_edt_select', nv.ptr(d2d), nv.ptr(clsd), Z, Y, X, r2, int(above), only, value, nv.ptr(out), nv.stream())
    return out


def _check(kind, name, target, invert, want=None):
    v = _volume(kind, name)
    want = _want(kind, name, target, invert) if want is None else want
    srcd = torch.tensor(v).cuda()
    d2, cls = _edt(srcd, target, invert)
    where = (kind, name, target, invert)
    assert np.array_equal(d2.cpu().numpy(), want), where
    assert np.array_equal(cls.cpu().numpy(), mr.class_map(v)[0]), where
    return srcd, d2, cls


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', SHAPE_NAMES)
def test_class_maps(name, kind):
    for target in (0, 1):
        for invert in (False, True):
            _check(kind, name, target, invert)
    if kind == 'blobs':                                    # a class nobody has: no seed at all, every voxel a seed
        assert (_check(kind, name, 9, False)[1] == mr.INF).all() and not _check(kind, name, 9, True)[1].any()


def test_the_sparse_volume():
    """108 seeds in 37 x 41 x 150: rows and a whole plane without a seed (tests/test_morphology_cpu.py shows it has them)."""
    _, d2, _ = _check('sparse', 'ragged', 1, False)
    assert int(d2.max()) < mr.INF and int(d2.max()) > 100
    _check('sparse', 'ragged', 1, True)
    _check('sparse', 'ragged', 0, True)


@pytest.mark.parametrize('name', SHAPE_NAMES)
def test_one_seed_against_the_closed_form(name):
    shape = SHAPES[name]
    z, y, x = np.indices(shape)
    for at in ((0, 0, 0), tuple(n - 1 for n in shape)):
        v = np.zeros(shape, np.uint8)
        v[at] = 3
        want = ((z - at[0]) ** 2 + (y - at[1]) ** 2 + (x - at[2]) ** 2).astype(np.int32)
        d2, cls = _edt(torch.tensor(v).cuda(), 3, False)
        assert np.array_equal(d2.cpu().numpy(), want) and np.array_equal(cls.cpu().numpy(), v), (name, at)


def test_long_distances_from_one_seed_in_the_last_voxel():
    shape = (2, 2, 16384)
    v = np.zeros(shape, np.uint8)
    v[-1, -1, -1] = 1
    z, y, x = np.indices(shape)
    want = ((z - 1) ** 2 + (y - 1) ** 2 + (x - 16383) ** 2).astype(np.int32)
    assert want.max() == 16383 ** 2 + 2 > 2.6e8
    d2, _ = _edt(torch.tensor(v).cuda(), 1, False, want_cls=False)
    assert np.array_equal(d2.cpu().numpy(), want)


@pytest.mark.parametrize('C', (2, 5))
@pytest.mark.parametrize('name', ('ragged', 'flat', 'long y', 'one voxel'))
def test_predicted_volumes(name, C):
    pred = _volume(str(C), name)
    if name != 'one voxel':
        never, tie = (pred.max(-1) == 0).mean(), (np.sort(pred, axis=-1)[..., -1] == np.sort(pred, axis=-1)[..., -2]).mean()
        assert 0.03 < never < 0.2 and 0.1 < tie < 0.35, (never, tie)
    for target in (0, 1):
        for invert in (False, True):
            srcd, d2, cls = _check(str(C), name, target, invert)
    none, cls2 = _edt(srcd, 1, False, want_d2=False)                           # the class-map pass alone
    assert none is None and torch.equal(cls2, cls)
    d3, none = _edt(srcd, 1, True, want_cls=False)
    assert none is None and torch.equal(d3, d2)


def test_the_class_map_pass_alone_on_class_maps():
    for name in ('ragged', 'long x', 'one voxel'):
        v = _volume('blobs', name)
        none, cls = _edt(torch.tensor(v).cuda(), 1, False, want_d2=False)
        assert none is None and np.array_equal(cls.cpu().numpy(), v)


@pytest.mark.parametrize('above', (False, True))
@pytest.mark.parametrize('name', ('ragged', 'flat', 'long z'))
def test_seeds_from_a_distance_map(name, above):
    prev = _want('blobs', name, 1, True)                                       # the distance to the outside of class 1
    prevd = torch.tensor(prev).cuda()
    for r2 in (0, 1, 4, 9, 13, 2 ** 31 - 2):
        got = _mask(prevd, r2, above)
        assert np.array_equal(got.cpu().numpy(), mr.distance_sq_mask(prev, r2, above)), (name, r2, above)
    assert np.array_equal(prevd.cpu().numpy(), prev)
    inf = torch.full_like(prevd, mr.INF)                                       # INF > every r2: all seeds above, none below
    got = _mask(inf, 2 ** 31 - 2, above)
    assert bool((got == (0 if above else mr.INF)).all())


@pytest.mark.parametrize('name', ('ragged', 'flat', 'one voxel'))
def test_select(name):
    v = _volume('blobs', name)
    d2 = _want('blobs', name, 1, False)
    d2d, clsd = torch.tensor(d2).cuda(), torch.tensor(v).cuda()
    for r2 in (0, 2, 9):
        for above in (False, True):
            for only, value in ((-1, 1), (0, 7), (2, 0), (9, 4)):
                want = mr.select(d2, v, r2, above, only, value)
                where = (name, r2, above, only, value)
                assert np.array_equal(_select(d2d, clsd, r2, above, only, value).cpu().numpy(), want), where
                odd = torch.empty(clsd.numel() + 1, dtype=torch.uint8, device='cuda')[1:].view(clsd.shape).copy_(clsd)      # the narrow path
                assert np.array_equal(_select(d2d, odd, r2, above, only, value).cpu().numpy(), want), where
                alias = clsd.clone()
                assert _select(d2d, alias, r2, above, only, value, alias=True) is alias and np.array_equal(alias.cpu().numpy(), want), where


@pytest.mark.parametrize('shape', ((1, 1, 3), (1, 5, 821)))
def test_select_at_the_streaming_pass_edges(shape):
    """The cases of test_filter_at_the_streaming_pass_edges (tests/test_gpu_components.py) for the other caller of volume_select_kernel."""
    N = int(np.prod(shape))
    v = np.array([[[1, 0, 2]]], np.uint8) if N == 3 else np.random.default_rng(N).integers(0, 4, shape).astype(np.uint8)
    d2 = mr.distance_sq(v, 1, False)
    d2d, clsd = torch.tensor(d2).cuda(), torch.tensor(v).cuda()
    assert (N == 3 or (N == 4096 + 9 and N % 4)) and d2d.data_ptr() % 16 == 0 and clsd.data_ptr() % 4 == 0
    for r2, above, only, value in ((0, False, -1, 7), (1, False, 0, 7), (1, True, 2, 0), (2, True, -1, 4)):
        want, where = mr.select(d2, v, r2, above, only, value), (r2, above, only, value)
        assert (want != v).any()
        assert np.array_equal(_select(d2d, clsd, r2, above, only, value).cpu().numpy(), want), where
        out = offset_copy(torch.full(shape, 55, dtype=torch.uint8, device='cuda'), 1)
        assert np.array_equal(_select(offset_copy(d2d, 4), offset_copy(clsd, 1), r2, above, only, value, out=out).cpu().numpy(), want), where
        for alias in (clsd.clone(), offset_copy(clsd, 1)):
            assert _select(d2d, alias, r2, above, only, value, alias=True) is alias and np.array_equal(alias.cpu().numpy(), want), where


def test_repeated_launches_and_a_second_stream_give_the_same_bytes():
    for kind, name in (('p50', 'ragged'), ('5', 'ragged'), ('p01', 'long y')):
        srcd = torch.tensor(_volume(kind, name)).cuda()
        a = _edt(srcd, 1, False)
        b = _edt(srcd, 1, False)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        ma, mb = _mask(a[0], 4, True), _mask(b[0], 4, True)
        assert torch.equal(ma, mb)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            c = _edt(srcd, 1, False)
            mc = _mask(c[0], 4, True)
        side.synchronize()
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) and torch.equal(ma, mc)


@pytest.mark.parametrize('radius', (0, 1, 1.5, 3))
def test_the_operators_on_resident_volumes(radius):
    from interactive_unet import morphology
    for kind, name, targets in (('blobs', 'ragged', (1, 2)), ('2', 'flat', (0, 1)), ('5', 'ragged', (0, 3)), ('blobs', 'one voxel', (0,))):
        v = _volume(kind, name)
        vd = torch.tensor(v).cuda()
        for target in targets:
            for got, want in ((morphology.dilate(vd, target, radius), mr.dilate(v, target, radius)),
                              (morphology.erode(vd, target, radius), mr.erode(v, target, radius)),
                              (morphology.erode(vd, target, radius, 7), mr.erode(v, target, radius, 7)),
                              (morphology.opening(vd, target, radius, 7), mr.opening(v, target, radius, 7)),
                              (morphology.closing(vd, target, radius), mr.closing(v, target, radius))):
                assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), (kind, name, target, radius)
            if radius == 0:
                d = morphology.distance_sq(vd, target, True)
                assert d.is_cuda and d.dtype == torch.int32 and np.array_equal(d.cpu().numpy(), _want(kind, name, target, True))
                c = morphology.class_map(vd)
                assert c.is_cuda and np.array_equal(c.cpu().numpy(), mr.class_map(v)[0])
        assert np.array_equal(vd.cpu().numpy(), v)                             # the input is left alone


@pytest.mark.parametrize('conn', (6, 18, 26))
def test_fill_holes_on_resident_volumes(conn):
    from interactive_unet import morphology
    v = holes_volume()
    got = morphology.fill_holes(torch.tensor(v).cuda(), 1, conn)
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), mr.fill_holes(v, 1, conn))
    for kind, target in (('blobs', 0), ('blobs', 1), ('2', 0), ('5', 1)):      # target 0 of a predicted volume: never predicted is outside it
        v = _volume(kind, 'ragged')
        got = morphology.fill_holes(torch.tensor(v).cuda(), target, conn)
        assert np.array_equal(got.cpu().numpy(), mr.fill_holes(v, target, conn)), (kind, target)


def test_host_refusals_on_resident_volumes():
    from interactive_unet import morphology
    vd = torch.tensor(_volume('blobs', 'flat')).cuda()
    with pytest.raises(ValueError):
        morphology.distance_sq(vd[:, :, ::2])
    with pytest.raises(ValueError):
        morphology.opening(vd.to(torch.int32), 1, 1)
    with pytest.raises(ValueError, match='radius'):
        morphology.closing(vd, 1, -1)


def test_opening_then_closing_of_a_real_prediction():
    from interactive_unet import morphology, predict
    from interactive_unet.unet import UNet
    from oracle import unet_ref
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = UNet(dim=3, levels=4, base=32, pretrained=False)
    m.load_named(unet_ref.init_params(dim=3, levels=4, base=32, seed=3, randomize_bn=True))
    m = m.cuda().eval()
    shape = (40, 36, 44)
    vol = np.random.default_rng(5).integers(0, 256, shape, dtype=np.uint8)
    pd = predict.predict_volume_array(m, torch.tensor(vol).cuda(), input_size=32, num_classes=2)
    assert pd.shape == shape + (2,) and pd.dtype == torch.uint8
    pred = pd.cpu().numpy()
    for target in (1, 0):
        opened = morphology.opening(pd, target, 1.5, fill=1 - target)
        closed = morphology.closing(opened, target, 1.5)
        w_opened = mr.opening(pred, target, 1.5, fill=1 - target)
        assert opened.is_cuda and closed.is_cuda
        assert np.array_equal(opened.cpu().numpy(), w_opened) and np.array_equal(closed.cpu().numpy(), mr.closing(w_opened, target, 1.5))


def test_a_volume_whose_distance_map_passes_2_32_bytes():
    """1030 x 1024 x 1024: d2 is 4.32e9 bytes (about 14 GB with the source and the workspace).  The lattice z % 7 == y % 5 == x % 9 == 0
    bounds every squared distance by 3^2 + 2^2 + 4^2 = 29 -- once it is closed by the last plane of each axis: 1024 is no multiple of 5
    or 9 plus 1, and behind the last lattice plane (y = 1020, x = 1017) the open lattice leaves 3 and 6 voxels, up to 54 (the first run
    found 49; tests/test_morphology_cpu.py shows both figures on the far corner).  So a 48^3 crop extended by 6 voxels defines its
    interior (the crop argument there): three crops against the definition on the host -- at the origin, across linear index 2^30 where
    d2 crosses byte 2^32, at the far corner -- and no voxel above 29 anywhere, on the device."""
    shape = Z, Y, X = (1030, 1024, 1024)
    assert 4 * Z * Y * X > 2 ** 32 and (1024 * Y + 0) * X == 2 ** 30
    g = torch.Generator(device='cuda').manual_seed(23)
    src = torch.empty(shape, dtype=torch.uint8, device='cuda')
    on = lambda lo, hi, n, step: torch.tensor(lattice_axis(n, step)[lo:hi], device='cuda')
    yx = on(0, Y, Y, 5)[:, None] & on(0, X, X, 9)[None, :]
    for z0 in range(0, Z, 64):
        z1 = min(Z, z0 + 64)
        lattice = on(z0, z1, Z, 7)[:, None, None] & yx[None]
        src[z0:z1] = (lattice | (torch.rand((z1 - z0, Y, X), device='cuda', generator=g) < 0.01)).to(torch.uint8)
    del lattice
    d2, none = _edt(src, 1, False, want_cls=False)
    assert none is None
    top = int(d2.max())
    assert 0 < top <= 29, top
    for lo in ((0, 0, 0), (982, 0, 0), (982, 976, 976)):
        hi = tuple(a + 48 for a in lo)
        elo = tuple(max(0, a - 6) for a in lo)
        ehi = tuple(min(n, b + 6) for n, b in zip(shape, hi))
        ext = mr.distance_sq(src[elo[0]:ehi[0], elo[1]:ehi[1], elo[2]:ehi[2]].cpu().numpy(), 1, False)
        want = ext[lo[0] - elo[0]:hi[0] - elo[0], lo[1] - elo[1]:hi[1] - elo[1], lo[2] - elo[2]:hi[2] - elo[2]]
        got = d2[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].cpu().numpy()
        assert want.shape == (48, 48, 48) and np.array_equal(got, want), lo
    assert lo[0] <= 1024 < hi[0]                                               # the last two crops hold voxels on both sides of byte 2^32
