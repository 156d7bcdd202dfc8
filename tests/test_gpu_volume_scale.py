"""The resident-volume kernels at volume scale.

Part A: connected components (csrc/components.hip) at the sizes where its launch policy changes -- several counts per thread in
scan_kernel, several chunks per workgroup in table_kernel, several tiles per workgroup in tile_kernel and seam_kernel, labels next to
INT_MAX -- against tests/components_ref.py directly or through the tiled closed form of tests/volume_scale_ref.py.
Part B: every resident-volume entry point on arrays whose flat element index passes 2^31 and whose byte offset passes 2^32, against its
definition evaluated on host crops (dyadic geometries: the crop's definition is the volume's, tests/test_volume_scale_cpu.py).

tests/test_volume_scale_cpu.py shows by arithmetic that every shape here lies past its threshold.  The host never holds a large array:
inputs are made on the device, only crops travel.  Outputs start from a pattern.  Every comparison is exact.  A test frees what it
allocated; the two module-wide arrays (V8, V8C: 4.4 GB each) live from their first use to the end of the module.  No test here is
skipped for lack of memory: an allocation that fails is a failure."""
import ctypes
import gc
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import multiscale_ref as mr
from oracle import predict_ref, slicer_ref
from tests import components_ref as cr
from tests import patch_ref
from tests import propose_ref as pr
from tests import slab_ref as sr
from tests import volume_scale_ref as vs
from tests.test_gpu_components import _filter, _label, _table
from tests.volume_inputs import random_pred


def _free():
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _wall_time_and_peak(request):
    """Prints what DESIGN.md section 4.1 records: the test's wall time and the peak allocation while it ran (module-wide arrays included)."""
    _free()
    torch.cuda.reset_peak_memory_stats()
    torch.cuda.synchronize()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    dt = time.time() - t0
    print(f'\nvolume scale: {request.node.name}: {dt:.2f} s, peak {torch.cuda.max_memory_allocated() / 1e9:.2f} GB allocated')
    _free()


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


# ---- Part A ------------------------------------------------------------------------------------------------------------------
def _direct(v, conn, bg, table=cr.table):
    """label, cls, count, table and filter of the host volume v against the definition itself."""
    w_labels, w_K, w_cls = cr.label(v, conn, bg)
    w_sizes, w_classes, w_first = table(w_labels, w_cls, w_K)
    srcd = torch.from_numpy(v).cuda()
    labels, K, cls = _label(srcd, conn, bg)
    assert K == w_K
    assert np.array_equal(labels.cpu().numpy(), w_labels) and np.array_equal(cls.cpu().numpy(), w_cls)
    sizes, classes, first = (t.cpu().numpy() for t in _table(labels, cls, K))
    assert np.array_equal(sizes, w_sizes) and np.array_equal(classes, w_classes) and np.array_equal(first, w_first)
    keep = (np.random.default_rng(K).random(K + 1) < 0.5).astype(np.uint8)
    out = _filter(labels, cls, K, torch.from_numpy(keep).cuda(), 9)
    assert np.array_equal(out.cpu().numpy(), cr.filter_components(w_labels, w_cls, keep, 9))
    del srcd, labels, cls, out
    return w_K, w_sizes


@pytest.mark.parametrize('kind,conn,bg', (('p50', 6, 0), ('p50', 26, 0), ('four', 6, None)))
def test_components_across_the_scan_and_table_thresholds(kind, conn, bg):
    """A.1: 2154 chunks -- three counts per thread of scan_kernel, two chunks per workgroup of table_kernel."""
    rng = np.random.default_rng(41)
    if kind == 'p50':                                      # supercritical: a giant component with millions of runs through the table pass
        v = (rng.random(vs.A1_SHAPE) < 0.5).astype(np.uint8)
    else:                                                  # every class subcritical: millions of components, the workgroup's hash table overflows
        v = rng.integers(0, 4, vs.A1_SHAPE).astype(np.uint8)
    K, sizes = _direct(v, conn, bg)
    n = int(np.prod(vs.A1_SHAPE))
    if kind == 'p50':
        assert sizes.max() >= 0.4 * n and (K >= 50000 or conn != 6), (K, sizes.max())
    else:
        assert K >= n // 4 and sizes.max() < 10000, (K, sizes.max())      # far more labels than the 1024 slots of a workgroup's table


@pytest.mark.parametrize('conn', (6, 26))
def test_components_of_a_column_of_more_tiles_than_the_grid(conn):
    """A.2: 1 048 580 tiles in a column -- the workgroups of tile_kernel and seam_kernel take a second tile."""
    v = (np.random.default_rng(42).random(vs.A2_COLUMN) < 0.5).astype(np.uint8)
    K, sizes = _direct(v, conn, 0, table=vs.table_fast)
    assert K > vs.A2_COLUMN[0] // 8 and sizes.max() < 64


def _tiled(block, n, conn, bg, separator, chunk, seed):
    """label, cls, count, table and filter of n copies of `block` against the tiled closed form, `chunk` copies at a time."""
    t = vs.Tiled(block, conn, bg, separator, device='cuda')
    src = t.volume(n)
    planes = t.bz + 1
    labels, K, cls = _label(src, conn, bg)
    del src
    assert K == t.count(n), (K, t.count(n))
    for i0 in range(0, n, chunk):
        i1 = min(i0 + chunk, n)
        assert torch.equal(labels[i0 * planes:i1 * planes], t.labels(i0, i1)), (i0, i1)
        assert torch.equal(cls[i0 * planes:i1 * planes], t.cls(i0, i1)), (i0, i1)
    for got, want in zip(_table(labels, cls, K), t.table(n)):
        assert torch.equal(got, want)
    keep = torch.randint(0, 2, (K + 1,), dtype=torch.uint8, device='cuda', generator=_gen(seed))
    fill = torch.tensor(9, dtype=torch.uint8, device='cuda')
    out = _filter(labels, cls, K, keep, 9)
    for i0 in range(0, n, chunk):
        i1 = min(i0 + chunk, n)
        lab, c = t.labels(i0, i1).long(), t.cls(i0, i1)
        assert torch.equal(out[i0 * planes:i1 * planes], torch.where((lab > 0) & (keep[lab] == 0), fill, c)), (i0, i1)
    del labels, cls, out, keep, lab, c
    return t, K


@pytest.mark.parametrize('conn', (6, 26))
@pytest.mark.parametrize('bg', (0, None))
def test_components_of_a_thin_volume_of_more_tiles_than_the_grid(bg, conn):
    """A.2: the same number of tiles, two across x: 136 M voxels, the tiled closed form."""
    Z, Y, X = vs.A2_THIN
    block = np.random.default_rng(43).integers(0, 3, (vs.A2_THIN_BZ, Y, X)).astype(np.uint8)
    n = vs.copies(vs.A2_THIN, vs.A2_THIN_BZ)
    t, K = _tiled(block, n, conn, bg, 0 if bg == 0 else 3, n, 1)
    assert K >= n


@pytest.mark.parametrize('bg', (0, None))
def test_components_of_a_predicted_volume_past_2_32_bytes(bg):
    """A.3: uint8 [700, 1201, 1301, 4] -- the class of voxel v is read at byte 4 v, up to 4.37e9."""
    Z, Y, X, C = vs.A3_SHAPE
    block = random_pred((vs.A3_BZ, Y, X), C, 44)
    t, K = _tiled(block, vs.copies(vs.A3_SHAPE, vs.A3_BZ), 18, bg, 0, 35, 2)
    assert np.array_equal(t.cls_B.cpu().numpy(), cr.class_map(block, bg)[0]) and K > 0


@pytest.mark.parametrize('bg', (0, None))
def test_components_next_to_the_cap(bg):
    """A.4: 2^31 - 65536 voxels.  Roots, `first` entries and (int)v + 1 come within 2^17 of INT_MAX; under background None the last
    plane is a component whose first voxel is 2^31 - 131072."""
    Z, Y, X = vs.A4_SHAPE
    block = (np.random.default_rng(45).random((vs.A4_BZ, Y, X)) < 0.25).astype(np.uint8)        # subcritical at connectivity 6
    n = vs.copies(vs.A4_SHAPE, vs.A4_BZ)
    t, K = _tiled(block, n, 6, bg, 0 if bg == 0 else 2, 64, 3)
    last = int(t.table(n)[2][-1])
    assert last > 2 ** 31 - 2 ** 22 and (bg == 0 or last == Z * Y * X - Y * X)


# ---- Part B ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def v8():
    v = torch.randint(0, 256, vs.V8_SHAPE, dtype=torch.uint8, device='cuda', generator=_gen(11))
    yield v
    del v
    _free()


@pytest.fixture(scope='module')
def v8c():
    """Random bytes; about a tenth of the voxels all-zero (never predicted)."""
    v = torch.randint(0, 256, vs.V8C_SHAPE, dtype=torch.uint8, device='cuda', generator=_gen(12))
    predicted = torch.randint(0, 10, vs.V8C_SHAPE[:3], dtype=torch.uint8, device='cuda', generator=_gen(13)) > 0
    v *= predicted[..., None].to(torch.uint8)
    del predicted
    yield v
    del v
    _free()


def _nonzero(vol):
    flat = vol.view(-1)
    return sum(int(torch.count_nonzero(flat[i:i + 2 ** 28])) for i in range(0, flat.numel(), 2 ** 28))


def _far(vol):
    """(host crop of the last CROP planes, rows and columns, its offset)."""
    off = vs.far_offset(vol.shape)
    return vol[off[0]:, off[1]:, off[2]:].cpu().numpy(), off


def _near(vol):
    return vol[:vs.CROP, :vs.CROP, :vs.CROP].cpu().numpy()


def _total(vol, dtype=torch.int64):
    """The sum of a large array, 2^28 elements at a time (torch converts a whole operand to the accumulator's type first)."""
    flat = vol.view(-1)
    return sum(flat[i:i + 2 ** 28].sum(dtype=dtype).item() for i in range(0, flat.numel(), 2 ** 28))


def test_gather_block_past_the_far_faces(v8):
    from interactive_unet import _native as nv
    S = 96
    far, off = _far(v8)
    corners = ((tuple(int(n) - 64 for n in vs.V8_SHAPE), far, off), ((-32, -32, -32), _near(v8), np.zeros(3, np.int64)))
    for (i0, j0, k0), crop, o in corners:
        out = torch.full((S, S, S), 77, dtype=torch.uint8, device='cuda')
        nv.call('iunet_gather_block', nv.ptr(v8), *vs.V8_SHAPE, i0, j0, k0, S, nv.ptr(out), nv.stream())
        p = [int(i0 - o[0]), int(j0 - o[1]), int(k0 - o[2])]
        want = predict_ref.get_padded_block(crop, *p, *[q + S for q in p])
        assert want.shape == (S, S, S) and np.array_equal(out.cpu().numpy(), want), (i0, j0, k0)


def test_blend_and_quantise_past_2_31_elements():
    from interactive_unet import _native as nv
    Z, Y, X, C = vs.VF_SHAPE
    S = 32
    pred = torch.zeros(vs.VF_SHAPE, dtype=torch.float32, device='cuda')
    weight = torch.zeros((Z, Y, X), dtype=torch.float32, device='cuda')
    window = predict_ref.gaussian_3d(S)
    rng = np.random.default_rng(14)
    zm, rest = divmod(2 ** 30, Y * X)                        # the voxel whose first class is element 2^31 of pred
    ym, xm = divmod(rest, X)
    assert 8 <= zm < Z - 8 and 8 <= ym < Y - 8 and 8 <= xm < X - 8
    blocks = (((0, 0, 0, 20, 32, 28), (12, 0, 4)), ((Z - 20, Y - 32, X - 28, Z, Y, X), (0, 0, 0)),
              ((zm - 8, ym - 8, xm - 8, zm + 8, ym + 8, xm + 8), (3, 16, 9)))
    boxes, nonzero, sums = [], 0, np.zeros(2)
    for blk, lo in blocks:
        e = [blk[3 + a] - blk[a] for a in range(3)]
        P = (1.0 - rng.random((S, S, S, C), dtype=np.float32)).astype(np.float32)              # (0, 1]: every contribution shows
        Pd, wd = torch.from_numpy(P).cuda(), torch.from_numpy(window).cuda()
        nv.call('iunet_blend_accumulate', nv.ptr(pred), nv.ptr(weight), nv.ptr(Pd), nv.ptr(wd), Z, Y, X, C, S, nv.int_array(blk),
                nv.int_array(lo + tuple(l + n for l, n in zip(lo, e))), nv.stream())
        torch.cuda.synchronize()
        loc = tuple(slice(l, l + n) for l, n in zip(lo, e))
        box = tuple(slice(blk[a], blk[3 + a]) for a in range(3))
        w_pred = np.zeros(tuple(e) + (C,), np.float32)
        w_pred += P[loc] * window[loc][..., None]
        w_weight = window[loc].copy()
        assert np.array_equal(pred[box].cpu().numpy(), w_pred) and np.array_equal(weight[box].cpu().numpy(), w_weight), blk
        boxes.append((box, w_pred, w_weight))
        nonzero += int(np.prod(e))
        sums += (w_pred.sum(dtype=np.float64), w_weight.sum(dtype=np.float64))
    # nothing else was touched
    assert _nonzero(pred) == nonzero * C and _nonzero(weight) == nonzero
    assert _total(pred, torch.float64) == pytest.approx(sums[0], rel=1e-12)
    assert _total(weight, torch.float64) == pytest.approx(sums[1], rel=1e-12)
    out = torch.full(vs.VF_SHAPE, 77, dtype=torch.uint8, device='cuda')
    nv.call('iunet_normalize_quantize', nv.ptr(pred), nv.ptr(weight), nv.ptr(out), Z * Y * X, C, 1e-3, nv.stream())
    total = 0
    for box, w_pred, w_weight in boxes:
        want = (255 * w_pred / np.maximum(w_weight, np.float32(1e-3))[..., None]).astype('uint8')
        assert want.any() and np.array_equal(out[box].cpu().numpy(), want)
        total += int(want.sum(dtype=np.int64))
    for z0, z1 in ((0, 2), (zm - 1, zm + 2), (Z - 2, Z)):      # whole planes at the start, across element 2^31 and at the end
        got = out[z0:z1].cpu().numpy()
        for box, _, _ in boxes:
            if box[0].start < z1 and box[0].stop > z0:
                got[max(box[0].start, z0) - z0:min(box[0].stop, z1) - z0, box[1], box[2]] = 0
        assert not got.any(), (z0, z1)
    assert _total(out) == total                              # every other byte was written, with 0
    del pred, weight, out


def test_zoom_of_a_volume_past_2_32_bytes(v8c):
    from interactive_unet import utils
    Z, Y, X, C = vs.V8C_SHAPE
    B = 128
    dst = torch.full((Z // 2, Y // 2, X // 2, C // 2), 7, dtype=torch.uint8, device='cuda')
    utils.resize_volume(v8c, dst, scale=0.5, block_size=B)
    nb = [-(-n // B) for n in (Z, Y, X)]
    rng = np.random.default_rng(15)
    picks = [(0, 0, 0), tuple(n - 1 for n in nb), (nb[0] - 1, 0, nb[2] - 2)] + [tuple(int(rng.integers(0, n)) for n in nb) for _ in range(2)]
    for bi, bj, bk in picks:
        blk = v8c[bi * B:(bi + 1) * B, bj * B:(bj + 1) * B, bk * B:(bk + 1) * B].cpu().numpy()
        want = mr.zoom_nearest(blk, 0.5)
        h = B // 2
        got = dst[bi * h:bi * h + want.shape[0], bj * h:bj * h + want.shape[1], bk * h:bk * h + want.shape[2]].cpu().numpy()
        assert want.size and np.array_equal(got, want), (bi, bj, bk)
    del dst


def _slice_gather(vd, a, b, o, sw, order):
    """iunet_slice_gather with the bounding-box crop of interactive_unet/slicer.py."""
    from interactive_unet import _native as nv
    start = sr.default_start(sw)
    ends = np.array([start, start + sw - 1], dtype=float)
    corners = a[:, None, None] * ends[None, :, None] + b[:, None, None] * ends[None, None, :] + o[:, None, None]
    shape = np.array(vd.shape)
    lo = np.minimum(np.maximum(np.floor(corners.min(axis=(1, 2))).astype(int), 0), shape)
    hi = np.minimum(np.ceil(corners.max(axis=(1, 2))).astype(int), shape)
    out = torch.full((sw, sw), 77, dtype=torch.uint8, device='cuda')
    nv.call('iunet_slice_gather', nv.ptr(vd), *[int(n) for n in shape], (ctypes.c_double * 9)(*a, *b, *o), nv.int_array(lo),
            nv.int_array(np.maximum(hi - lo, 0)), sw, start, order, nv.ptr(out), nv.stream())
    return out, lo


@pytest.mark.parametrize('order', (0, 1))
def test_slice_gather_at_the_far_corner(v8, order):
    crop, off = _far(v8)
    sw = vs.SLAB[1]
    p, q, r = vs.SLAB_VECTORS
    o = vs.far_origin(vs.V8_SHAPE, (20, 24, 18))
    for name, (a, b, n) in (('a b', (p, q, r)), ('b n', (q, r, p)), ('n a', (r, p, q))):          # three oblique planes through one point
        got, lo = _slice_gather(v8, a, b, o, sw, order)
        assert (lo >= off).all(), name                       # the crop box lies in the host crop
        want = slicer_ref.get_slice(crop, n, a, b, o - off, axis=0, slice_width=sw, order=order)
        assert np.array_equal(got.cpu().numpy(), want), name
        assert want.any() and (want == 0).any(), name       # inside and outside the volume


def test_slice_scatter_onto_the_far_faces(v8c):
    from interactive_unet import _native as nv
    Z, Y, X, C = vs.V8C_SHAPE
    sw = 64
    a, b, n, o = vs.slab_geometries(vs.V8C_SHAPE)['oblique']
    data = np.random.default_rng(16).integers(0, 256, (sw, sw, C), dtype=np.uint8)
    crop, off = _far(v8c)
    coords = slicer_ref.interpolation_coords(n, a, b, o, sw)[0]
    idx = np.round(coords).reshape(3, -1).astype(int)
    assert (idx.min(axis=1) >= off).all() and (idx.max(axis=1) > np.array([Z, Y, X])).any()      # clipped onto the far faces only
    clipped = np.stack([np.clip(idx[x], 0, (Z, Y, X)[x] - 1) for x in range(3)], axis=1)
    assert len(np.unique(clipped, axis=0)) < sw * sw         # duplicate targets: the last pixel wins
    before = _total(v8c)
    ws = torch.empty(int(nv.lib().iunet_slice_scatter_workspace_bytes(sw)), dtype=torch.uint8, device='cuda')
    dd = torch.from_numpy(data).cuda()
    nv.call('iunet_slice_scatter', nv.ptr(v8c), Z, Y, X, C, (ctypes.c_double * 9)(*a, *b, *o), sw, sr.default_start(sw), nv.ptr(dd), nv.ptr(ws),
            nv.stream())
    want = slicer_ref.update_volume(data, crop.copy(), n, a, b, o - off, axis=0)
    assert (want != crop).any() and np.array_equal(_far(v8c)[0], want)
    assert _total(v8c) - before == int(want.sum(dtype=np.int64)) - int(crop.sum(dtype=np.int64))      # no byte outside the crop changed its sum


@pytest.mark.parametrize('order', (0, 1))
def test_slab_gather_at_the_far_corner(v8, order):
    from interactive_unet import _native as nv
    crop, off = _far(v8)
    T, sw = vs.SLAB
    for name, geom in vs.slab_geometries(vs.V8_SHAPE).items():
        c = sr.coords(geom, T, sw)
        assert all(c[x].min() >= off[x] + 1 for x in range(3)) and any(c[x].max() > vs.V8_SHAPE[x] for x in range(3)), name
        out = torch.full((T, sw, sw), 77, dtype=torch.uint8, device='cuda')
        nv.call('iunet_slab_gather', nv.ptr(v8), *vs.V8_SHAPE, (ctypes.c_double * 12)(*[float(t) for v in geom for t in v]), T, sw,
                sr.default_start(sw), sr.default_start(T), order, nv.ptr(out), nv.stream())
        want = sr.gather(crop, vs.shifted(geom, off), T, sw, order)
        assert np.array_equal(out.cpu().numpy(), want), name
        assert want.any() and (want == 0).any(), name


def test_slab_paste_at_the_far_corner(v8c):
    from interactive_unet import _native as nv
    Z, Y, X, C = vs.V8C_SHAPE
    T, sw = vs.SLAB
    probs = np.random.default_rng(17).random((T, sw, sw, C), dtype=np.float32)
    pd = torch.from_numpy(probs).cuda()
    for name, geom in vs.slab_geometries(vs.V8C_SHAPE).items():
        crop, off = _far(v8c)
        past = 2 ** 32 // (Y * X * C) + 1 - int(off[0])
        lo, length = off + 8, np.array([vs.CROP - 8] * 3)
        before = _total(v8c)
        nv.call('iunet_slab_paste', nv.ptr(v8c), Z, Y, X, C, (ctypes.c_double * 12)(*[float(t) for v in geom for t in v]), nv.int_array(lo),
                nv.int_array(length), nv.ptr(pd), T, sw, sr.default_start(sw), sr.default_start(T), 1, T, 1, nv.stream())
        want = sr.paste(crop, probs, vs.shifted(geom, off), 1, T, 1, lo=lo - off, length=length)
        assert (want != crop).any() and np.array_equal(_far(v8c)[0], want), name
        assert (want[past:] != crop[past:]).any(), name      # planes that lie past byte 2^32 are written
        assert _total(v8c) - before == int(want.sum(dtype=np.int64)) - int(crop.sum(dtype=np.int64)), name


def _uncertainty_torch(p, w, im):
    """propose_ref.uncertainty restated with torch on the device, in integers: the two largest bytes of a voxel are its largest byte and
    the largest of the pairwise minima."""
    ch = [p[..., c] for c in range(p.shape[-1])]
    b1 = torch.amax(p, dim=-1)
    b2 = torch.zeros_like(b1)
    for i in range(len(ch)):
        for j in range(i + 1, len(ch)):
            b2 = torch.maximum(b2, torch.minimum(ch[i], ch[j]))
    u = torch.where(b1 > 0, 255 - (b1 - b2), torch.zeros_like(b1))
    u[(w > 0).any(dim=-1)] = 0
    u[im[..., 0] == 0] = 0
    return u


def test_uncertainty_volume_past_2_32_bytes(v8c):
    from interactive_unet import _native as nv
    Z, Y, X, C = vs.V8C_SHAPE
    weight = torch.randint(0, 256, (Z, Y, X, 2), dtype=torch.uint8, device='cuda', generator=_gen(18))
    weight *= torch.randint(0, 10, (Z, Y, X, 2), dtype=torch.uint8, device='cuda', generator=_gen(19)) >= 7       # 70 % zeros
    image = torch.randint(0, 5, (Z, Y, X, 1), dtype=torch.uint8, device='cuda', generator=_gen(20))              # 20 % dark
    plane = Y * X * C
    slabs = ((0, 4), (2 ** 31 // plane // 4 * 4, 2 ** 31 // plane // 4 * 4 + 4), (2 ** 32 // plane // 4 * 4, 2 ** 32 // plane // 4 * 4 + 4),
             (Z - 4, Z))
    assert all(z0 % 4 == 0 and z0 * plane <= edge < z1 * plane for (z0, z1), edge in zip(slabs[1:3], (2 ** 31, 2 ** 32))) and Z % 32
    u8 = None
    for g in (4, 32):                                        # 32: ragged bricks on every axis
        nb = [-(-n // g) for n in (Z, Y, X)]
        u = torch.full((Z, Y, X), 77, dtype=torch.uint8, device='cuda')
        bricks = torch.full(nb, -1, dtype=torch.int32, device='cuda')
        nv.call('iunet_uncertainty_volume', nv.ptr(v8c), Z, Y, X, C, nv.ptr(weight), 2, nv.ptr(image), 1, g, nv.ptr(u), nv.ptr(bricks),
                nv.stream())
        b64 = bricks.to(torch.int64) & 0xffffffff
        if g == 4:                                           # the definition itself on brick-aligned slabs
            for z0, z1 in slabs:
                want = pr.uncertainty(v8c[z0:z1].cpu().numpy(), weight[z0:z1].cpu().numpy(), image[z0:z1].cpu().numpy())
                assert want.any() and np.array_equal(u[z0:z1].cpu().numpy(), want), (z0, z1)
                assert np.array_equal(b64[z0 // g:-(-z1 // g)].cpu().numpy(), pr.brick_sums(want, g).astype(np.int64)), (z0, z1)
            u8 = u
        else:
            assert torch.equal(u, u8)
        # the torch restatement over the whole volume, a hundred planes at a time
        for z0 in range(0, Z, 100):
            z1 = min(z0 + 100, Z)
            assert torch.equal(u[z0:z1], _uncertainty_torch(v8c[z0:z1], weight[z0:z1], image[z0:z1])), (z0, z1)
        padded = torch.zeros([n * g for n in nb], dtype=torch.uint8, device='cuda')
        padded[:Z, :Y, :X] = u
        want_b = padded.view(nb[0], g, nb[1], g, nb[2], g).sum(dim=(1, 3, 5), dtype=torch.int64)
        assert torch.equal(b64, want_b), g
        assert int(b64.sum()) == _total(u) > 0
        del padded, want_b, b64, bricks
    del u, u8, weight, image


def test_plane_scores_at_both_corners_in_one_launch(v8):
    from interactive_unet import _native as nv
    sw = vs.SLAB[1]
    far, off = _far(v8)
    near = _near(v8)
    planes, want = [], []
    for name, (a, b, _, o) in vs.slab_geometries(vs.V8_SHAPE).items():
        c = pr.plane_coords((a, b, o), sw)
        assert all(c[x].min() >= off[x] for x in range(3)), name
        planes.append((a, b, o))
        want.append(pr.plane_score(far, (a, b, o - off), sw))
    for name, (a, b, _, o) in vs.origin_geometries().items():
        c = pr.plane_coords((a, b, o), sw)
        assert all(c[x].max() <= vs.CROP - 1 for x in range(3)), name
        planes.append((a, b, o))
        want.append(pr.plane_score(near, (a, b, o), sw))
    want = np.array(want, dtype=np.int64)
    assert (want[:, 1] > 0).all() and (want[:, 1] < sw * sw).all() and (want[:, 0] > 0).all()
    geoms = np.ascontiguousarray(planes, dtype=np.float64).reshape(-1, 9)
    P = geoms.shape[0]
    need = nv.lib().iunet_plane_scores_ws_bytes(P, sw)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    out = torch.full((P, 2), -7, dtype=torch.int64, device='cuda')
    gd = torch.from_numpy(geoms).cuda()
    nv.call('iunet_plane_scores', nv.ptr(v8), *vs.V8_SHAPE, nv.ptr(gd), P, sw, pr.default_start(sw), nv.ptr(ws),
            need, nv.ptr(out), nv.stream())
    assert np.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize('order', (0, 1))
def test_patches_near_the_far_corner(v8, order):
    """The volume is image, mask and weight at once (read only): a mask byte >= C sets no channel."""
    from interactive_unet import _native as nv
    from interactive_unet.loader import PatchDesc
    assert nv.lib().iunet_patch_desc_bytes() == ctypes.sizeof(PatchDesc)
    crop, off = _far(v8)
    Z, Y, X = vs.V8_SHAPE
    C, ch = 2, 1
    centre = vs.patch_centre(vs.V8_SHAPE)
    poses = list(vs.PATCH_POSES.items())
    descs = (PatchDesc * len(poses))()
    for d, (name, m) in zip(descs, poses):
        p = patch_ref.coordinates(m.reshape(-1), centre, vs.PATCH)
        assert all(p[x].min() >= off[x] + 1 for x in range(3)) and any(p[x].max() > vs.V8_SHAPE[x] for x in range(3)), name
        d.image = d.mask = d.weight = v8.data_ptr()
        d.wstride, d.Z, d.Y, d.X, d.keep_dark = 1, Z, Y, X, 0
        d.m[:] = [float(t) for t in m.reshape(-1)]
        d.c[:] = [float(t) for t in centre]
    B = len(poses)
    raw = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).cuda()
    lut = torch.from_numpy(patch_ref.LUT.copy()).cuda()
    X16, y16, w16 = (torch.full((B, n) + vs.PATCH, 3.0, dtype=torch.float16, device='cuda') for n in (ch, C, C))
    nv.call('iunet_patch_batch', nv.ptr(raw), B, ch, C, *vs.PATCH, order, nv.ptr(lut), nv.ptr(X16), nv.ptr(y16), nv.ptr(w16), nv.stream())
    got = [t.cpu().numpy() for t in (X16, y16, w16)]
    for k, (name, m) in enumerate(poses):
        want = patch_ref.patch(crop, crop, crop, m.reshape(-1), centre - off, vs.PATCH, C, order)
        for g, w in zip(got, want):
            assert np.array_equal(g[k].view(np.uint16), w.view(np.uint16)), name
        assert want[0].any() and (want[0] == 0).any() and want[1].any() and want[2].any(), name
