"""Connected components on the device: iunet_cc_label, iunet_cc_table and iunet_cc_filter bit for bit against the
definition tests/components_ref.py, and the host layer interactive_unet/components.py end to end -- on random, planted and adversarial
volumes and on a real prediction of the 3-D net.  The shapes follow the kernel's tile (components.TILE): ragged tiles on every axis,
three tiles per axis, one tile, one voxel."""
import functools
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import components_ref as cr
from tests.volume_inputs import offset_copy, random_pred

CONN = (6, 18, 26)


def _tile():
    from interactive_unet import components
    return components.TILE


def _shapes():
    tz, ty, tx = _tile()
    return {'ragged': (37, 41, 150), 'three tiles': (2 * tz + 3, 2 * ty + 1, 2 * tx + 5), 'row': (1, 1, 300), 'flat': (33, 2, 65),
            'one tile': (tz, ty, tx), 'one voxel': (1, 1, 1)}


SHAPE_NAMES = ('ragged', 'three tiles', 'row', 'flat', 'one tile', 'one voxel')


def _serpentine(shape):
    """A one-voxel-wide path: every second plane holds a boustrophedon over every second row, joined to the next one through one voxel."""
    Z, Y, X = shape
    plane = np.zeros((Y, X), np.uint8)
    for j in range(0, Y, 2):
        plane[j, :] = 1
        if j + 1 < Y:
            plane[j + 1, -1 if (j // 2) % 2 == 0 else 0] = 1
    last = (Y - 1) // 2 * 2                                        # the path ends on the last full row, at the end its turn points to
    end = (last, X - 1 if (last // 2) % 2 == 0 else 0)
    v = np.zeros(shape, np.uint8)
    v[0::2] = plane
    v[1::2, end[0], end[1]] = 1
    return v


def _straddle(shape):
    """(volume, components at 6 / 18 / 26): two voxels that touch only across the corner where eight tiles meet, their mirror image across
    another such corner, and an object whose first voxel lies in the last tile while the rest of it runs through earlier tiles."""
    tz, ty, tx = _tile()
    v = np.zeros(shape, np.uint8)
    v[tz - 1, ty - 1, tx - 1] = v[tz, ty, tx] = 1
    v[tz - 1, ty, tx] = v[tz, ty - 1, tx - 1] = 2                   # the anti-diagonal pair of the same corner, of another class
    v[2 * tz, 2 * ty, 2 * tx + 1] = 3                               # the first voxel: in the last tile
    v[2 * tz + 1, 2 * ty, :] = 3
    v[2 * tz + 1, :, 0] = 3
    v[2 * tz + 2, 0, :] = 3
    return v, {6: 5, 18: 5, 26: 3}


@functools.lru_cache(maxsize=None)
def _volume(kind, name):
    shape = _shapes()[name]
    seed = SHAPE_NAMES.index(name)
    if kind == 'p50':
        v = (np.random.default_rng(seed).random(shape) < 0.5).astype(np.uint8)
    elif kind == 'p25':
        v = (np.random.default_rng(10 + seed).random(shape) < 0.25).astype(np.uint8)
    elif kind == 'four':
        v = np.random.default_rng(20 + seed).integers(0, 4, shape).astype(np.uint8)
    elif kind == 'full':
        v = np.full(shape, 200, np.uint8)
    elif kind == 'checker':
        v = (np.indices(shape).sum(axis=0) % 2).astype(np.uint8)
    elif kind == 'serpentine':
        v = _serpentine(shape)
    elif kind == 'straddle':
        v = _straddle(shape)[0]
    else:
        v = random_pred(shape, int(kind), 30 + seed)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _want(kind, name, conn, bg):
    """The definition's (labels, K, cls, sizes, classes, first), computed once and shared."""
    labels, K, cls = cr.label(_volume(kind, name), conn, bg)
    out = (labels, K, cls) + cr.table(labels, cls, K)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _label(srcd, conn, bg, want_cls=True):
    """The entry point itself; outputs start from a pattern, so an element left unwritten shows."""
    from interactive_unet import _native as nv
    Z, Y, X = srcd.shape[:3]
    C = 1 if srcd.ndim == 3 else srcd.shape[3]
    labels = torch.full((Z, Y, X), -7, dtype=torch.int32, device='cuda')
    cls = torch.full((Z, Y, X), 77, dtype=torch.uint8, device='cuda') if want_cls else None
    count = torch.full((1,), -5, dtype=torch.int32, device='cuda')
    ws_bytes = nv.lib().iunet_cc_ws_bytes(Z, Y, X)
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device='cuda')
    nv.call('iunet_cc_label', nv.ptr(srcd), Z, Y, X, C, conn, -1 if bg is None else bg, nv.ptr(labels), nv.ptr(cls), nv.ptr(count), nv.ptr(ws),
            ws_bytes, nv.stream())
    return labels, int(count.item()), cls


def _table(labels, cls, K):
    from interactive_unet import _native as nv
    Z, Y, X = labels.shape
    sizes = torch.full((K + 1,), -3, dtype=torch.int32, device='cuda')
    classes = torch.full((K + 1,), 99, dtype=torch.uint8, device='cuda')
    first = torch.full((K + 1,), -9, dtype=torch.int32, device='cuda')
    nv.call('iunet_cc_table', nv.ptr(labels), nv.ptr(cls), Z, Y, X, K, nv.ptr(sizes), nv.ptr(classes), nv.ptr(first), nv.stream())
    return sizes, classes, first


def _filter(labels, cls, K, keep, fill, alias=False, out=None):
    from interactive_unet import _native as nv
    Z, Y, X = labels.shape
    out = out if out is not None else cls if alias else torch.full((Z, Y, X), 55, dtype=torch.uint8, device='cuda')
    nv.call('iunet_cc_filter', nv.ptr(labels), nv.ptr(cls), Z, Y, X, K, nv.ptr(keep), fill, nv.ptr(out), nv.stream())
    return out


def _check(kind, name, conn, bg):
    """label (with and without cls, launched twice) and table of one volume against the definition; returns the definition's numbers."""
    v = _volume(kind, name)
    w_labels, w_K, w_cls, w_sizes, w_classes, w_first = _want(kind, name, conn, bg)
    srcd = torch.tensor(v).cuda()
    labels, K, cls = _label(srcd, conn, bg)
    where = (kind, name, conn, bg)
    assert K == w_K, where
    assert np.array_equal(labels.cpu().numpy(), w_labels), where
    assert np.array_equal(cls.cpu().numpy(), w_cls), where
    labels2, K2, none = _label(srcd, conn, bg, want_cls=False)                            # a repeated launch, cls not asked for
    assert none is None and K2 == K and torch.equal(labels2, labels), where
    sizes, classes, first = _table(labels, cls, K)
    sizes, classes, first = sizes.cpu().numpy(), classes.cpu().numpy(), first.cpu().numpy()
    assert np.array_equal(sizes, w_sizes) and np.array_equal(classes, w_classes) and np.array_equal(first, w_first), where
    assert int(sizes.sum()) == int((w_labels > 0).sum()) and sizes[0] == 0 and first[0] == -1 and (np.diff(first[1:]) > 0).all(), where
    return w_K, w_sizes


@pytest.mark.parametrize('conn', CONN)
@pytest.mark.parametrize('name', SHAPE_NAMES)
def test_random_binary_volumes(name, conn):
    K, sizes = _check('p50', name, conn, 0)
    if name == 'ragged':                                   # supercritical: one giant component across every seam, thousands of small ones
        assert sizes.max() >= 0.4 * np.prod(_shapes()[name]) and (K >= 1000 or conn != 6), (K, sizes.max())   # (at 18 / 26 the giant one takes nearly all)
    K, sizes = _check('p25', name, conn, 0)
    if name == 'ragged' and conn == 6:                     # subcritical: many small components
        assert K >= 10000 and sizes.max() < 1000, (K, sizes.max())


@pytest.mark.parametrize('conn', CONN)
@pytest.mark.parametrize('name', SHAPE_NAMES)
def test_random_four_class_maps(name, conn):
    K0, _ = _check('four', name, conn, 0)
    K1, _ = _check('four', name, conn, None)
    assert K1 >= K0
    if name == 'ragged' and conn == 6:
        assert K1 > 50000


@pytest.mark.parametrize('conn', CONN)
@pytest.mark.parametrize('name', SHAPE_NAMES)
def test_full_checkerboard_and_serpentine(name, conn):
    shape = _shapes()[name]
    assert _check('full', name, conn, 0)[0] == 1
    K, _ = _check('checker', name, conn, 0)
    K_all, _ = _check('checker', name, conn, None)
    if min(shape) >= 2:                                                     # a wrong offset set shows here
        assert K == (int(_volume('checker', name).sum()) if conn == 6 else 1) and K_all == (int(np.prod(shape)) if conn == 6 else 2)
    assert _check('serpentine', name, conn, 0)[0] == 1                      # the deepest union chains
    assert int(_volume('serpentine', name).sum()) >= max(shape)


@pytest.mark.parametrize('conn', CONN)
def test_objects_that_straddle_tiles(conn):
    _, want = _straddle(_shapes()['three tiles'])
    labels, K, _, _, _, first = _want('straddle', 'three tiles', conn, 0)
    assert K == want[conn]
    tz, ty, tx = _tile()
    Z, Y, X = _shapes()['three tiles']
    at = ((2 * tz) * Y + 2 * ty) * X + 2 * tx + 1
    assert at in first.tolist() and at // (Y * X) // tz == 2 and at // X % Y // ty == 2 and at % X // tx == 2
    _check('straddle', 'three tiles', conn, 0)


@pytest.mark.parametrize('C', (2, 3, 16))
@pytest.mark.parametrize('name', ('three tiles', 'flat', 'one voxel'))
def test_planted_predicted_volumes(name, C):
    pred = _volume(str(C), name)
    if name != 'one voxel':
        never, tie = (pred.max(-1) == 0).mean(), (np.sort(pred, axis=-1)[..., -1] == np.sort(pred, axis=-1)[..., -2]).mean()
        assert 0.03 < never < 0.2 and 0.1 < tie < 0.35, (never, tie)
    for conn in CONN:
        for bg in (0, None):
            _check(str(C), name, conn, bg)
    cls = _want(str(C), name, 6, 0)[2]
    assert np.array_equal(cls, pred.argmax(axis=-1))


def test_repeated_launches_and_a_second_stream_give_the_same_bytes():
    srcd = torch.tensor(_volume('p50', 'ragged')).cuda()
    pd = torch.tensor(_volume('3', 'three tiles')).cuda()
    for d, bg in ((srcd, 0), (pd, None)):
        a = _label(d, 26, bg)
        b = _label(d, 26, bg)
        assert a[1] == b[1] and torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
        ta, tb = _table(a[0], a[2], a[1]), _table(b[0], b[2], b[1])
        assert all(torch.equal(x, y) for x, y in zip(ta, tb))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            c = _label(d, 26, bg)
            tc = _table(c[0], c[2], c[1])
        side.synchronize()
        assert c[1] == a[1] and torch.equal(c[0], a[0]) and torch.equal(c[2], a[2]) and all(torch.equal(x, y) for x, y in zip(ta, tc))


@pytest.mark.parametrize('name', ('ragged', 'flat', 'one voxel'))
def test_filter(name):
    for kind, bg in (('four', 0), ('p50', 0), ('four', None)):
        labels, K, cls = _want(kind, name, 18, bg)[:3]
        ld, cd = torch.tensor(labels).cuda(), torch.tensor(cls).cuda()
        keep = (np.random.default_rng(K).random(K + 1) < 0.5).astype(np.uint8)
        kd = torch.tensor(keep).cuda()
        for fill in (0, 9):                                # equal to and different from the background
            want = cr.filter_components(labels, cls, keep, fill)
            assert np.array_equal(_filter(ld, cd, K, kd, fill).cpu().numpy(), want), (kind, bg, fill)
            # a byte-offset view: the narrow path
            odd = torch.empty(cd.numel() + 1, dtype=torch.uint8, device='cuda')[1:].view(cd.shape).copy_(cd)
            assert np.array_equal(_filter(ld, odd, K, kd, fill).cpu().numpy(), want), (kind, bg, fill)
            alias = cd.clone()
            assert _filter(ld, alias, K, kd, fill, alias=True) is alias and np.array_equal(alias.cpu().numpy(), want), (kind, bg, fill)


@pytest.mark.parametrize('shape', ((1, 1, 3), (1, 5, 821)))
def test_filter_at_the_streaming_pass_edges(shape):
    """The pass cc_filter shares with edt_select (volume_select_kernel): fewer voxels than one vector (3); one workgroup's 4096 and a tail
    that is no multiple of 4 (4105); labels 4 bytes and cls / out 1 byte off the 16-byte grid (one voxel per thread); out aliasing cls."""
    N = int(np.prod(shape))
    v = np.array([[[1, 0, 2]]], np.uint8) if N == 3 else np.random.default_rng(N).integers(0, 4, shape).astype(np.uint8)
    labels, K, cls = cr.label(v, 18, 0)
    keep = np.array([0, 0, 1], np.uint8) if N == 3 else (np.random.default_rng(K).random(K + 1) < 0.5).astype(np.uint8)   # 3: filled; none; kept
    ld, cd, kd = torch.tensor(labels).cuda(), torch.tensor(cls).cuda(), torch.tensor(keep).cuda()
    assert (N == 3 or (N == 4096 + 9 and N % 4)) and ld.data_ptr() % 16 == 0 and cd.data_ptr() % 4 == 0
    for fill in (0, 9):
        want = cr.filter_components(labels, cls, keep, fill)
        assert (want != cls).any()
        assert np.array_equal(_filter(ld, cd, K, kd, fill).cpu().numpy(), want), fill
        out = offset_copy(torch.full(shape, 55, dtype=torch.uint8, device='cuda'), 1)
        assert np.array_equal(_filter(offset_copy(ld, 4), offset_copy(cd, 1), K, kd, fill, out=out).cpu().numpy(), want), fill
        for alias in (cd.clone(), offset_copy(cd, 1)):
            assert _filter(ld, alias, K, kd, fill, alias=True) is alias and np.array_equal(alias.cpu().numpy(), want), fill


def test_remove_small_and_keep_largest_on_resident_volumes():
    from interactive_unet import components
    for kind, name in (('four', 'three tiles'), ('p25', 'ragged'), ('3', 'flat')):
        v = _volume(kind, name)
        vd = torch.tensor(v).cuda()
        for conn, bg in ((6, 0), (26, None)):
            labels, K, cls = components.label(vd, conn, bg)
            w_labels, w_K, w_cls = _want(kind, name, conn, bg)[:3]
            assert isinstance(K, int) and K == w_K and labels.is_cuda and cls.is_cuda
            assert np.array_equal(labels.cpu().numpy(), w_labels) and np.array_equal(cls.cpu().numpy(), w_cls)
            for got, want in zip(components.table(labels, cls, K), components.table(w_labels, w_cls, K)):
                assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
            for m, fill in ((2, None), (7, 5)):
                got = components.remove_small(vd, m, conn, bg, fill)
                assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), components.remove_small(v, m, conn, bg, fill))
            for n, per in ((1, True), (3, False), (2, True)):
                got = components.keep_largest(vd, n, per, conn, bg)
                assert got.is_cuda and np.array_equal(got.cpu().numpy(), components.keep_largest(v, n, per, conn, bg)), (kind, conn, bg, n, per)
    with pytest.raises(ValueError):
        components.label(vd[:, :, ::2])
    with pytest.raises(ValueError):
        components.table(labels, cls.cpu(), K)


def test_no_component_at_all():
    from interactive_unet import components
    for shape in ((5, 17, 70), (1, 1, 1)):
        v = np.full(shape, 4, np.uint8)
        vd = torch.tensor(v).cuda()
        labels, K, cls = _label(vd, 6, 4)
        assert K == 0 and not labels.any() and torch.equal(cls, vd)
        sizes, classes, first = _table(labels, cls, 0)
        assert sizes.tolist() == [0] and classes.tolist() == [0] and first.tolist() == [-1]
        keep = torch.zeros(1, dtype=torch.uint8, device='cuda')
        assert torch.equal(_filter(labels, cls, 0, keep, 9), vd)
        assert torch.equal(components.remove_small(vd, 3, background=4), vd) and torch.equal(components.keep_largest(vd, background=4), vd)
    pd = torch.zeros((5, 17, 70, 3), dtype=torch.uint8, device='cuda')      # never predicted anywhere
    labels, K, cls = _label(pd, 26, None)
    assert K == 0 and not labels.any() and not cls.any()


def test_components_of_a_real_prediction():
    from interactive_unet import components, predict
    from interactive_unet.unet import UNet
    from oracle import unet_ref
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = UNet(dim=3, levels=4, base=32, pretrained=False)
    m.load_named(unet_ref.init_params(dim=3, levels=4, base=32, seed=3, randomize_bn=True))
    m = m.cuda().eval()
    shape = (48, 40, 56)
    vol = np.random.default_rng(5).integers(0, 256, shape, dtype=np.uint8)
    pd = predict.predict_volume_array(m, torch.tensor(vol).cuda(), input_size=32, num_classes=2)
    assert pd.shape == shape + (2,) and pd.dtype == torch.uint8
    pred = pd.cpu().numpy()
    for conn, bg in ((6, 0), (26, None)):
        labels, K, cls = components.label(pd, conn, bg)
        w_labels, w_K, w_cls = cr.label(pred, conn, bg)
        assert K == w_K and K >= 1 and np.array_equal(labels.cpu().numpy(), w_labels) and np.array_equal(cls.cpu().numpy(), w_cls)
