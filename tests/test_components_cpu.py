"""Connected components without a GPU: the definition tests/components_ref.py against scipy.ndimage.label's own
numbering and on hand-made voxels; the host layer's numpy path against the definition; remove_small / keep_largest; the host refusals
and the entry points' argument checks through the built library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import components_ref as cr
from tests.volume_inputs import random_pred

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONN = (6, 18, 26)
SHAPES = ((37, 41, 150), (33, 2, 65), (1, 1, 300))


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('conn', CONN)
def test_the_restatement_is_scipys_numbering_on_binary_inputs(shape, conn):
    for p, seed in ((0.5, 0), (0.25, 1)):
        b = (np.random.default_rng(seed).random(shape) < p).astype(np.uint8)
        want, k = ndimage.label(b, structure=ndimage.generate_binary_structure(3, cr.RANK[conn]))
        labels, K, cls = cr.label(b, conn, 0)
        assert K == k and labels.dtype == np.int32 and np.array_equal(labels, want) and np.array_equal(cls, b)


def test_two_voxels_by_face_edge_and_corner():
    for other, joined in (((0, 0, 1), (6, 18, 26)), ((0, 1, 0), (6, 18, 26)), ((1, 0, 0), (6, 18, 26)), ((0, 1, 1), (18, 26)),
                          ((1, 0, 1), (18, 26)), ((1, 1, 0), (18, 26)), ((1, 1, 1), (26,))):
        for flip in (False, True):
            v = np.zeros((2, 2, 2), np.uint8)
            v[0, 0, 0] = v[other] = 1
            v = v[:, :, ::-1].copy() if flip else v            # the anti-diagonals too
            for conn in CONN:
                labels, K, _ = cr.label(v, conn, 0)
                assert K == (1 if conn in joined else 2), (other, flip, conn)
                assert sorted(labels[v > 0].tolist()) == ([1, 1] if conn in joined else [1, 2])


def test_two_classes_side_by_side_and_background():
    v = np.array([[[1, 1, 2, 2, 0, 1]]], np.uint8)
    labels, K, cls = cr.label(v, 6, 0)
    assert labels.tolist() == [[[1, 1, 2, 2, 0, 3]]] and K == 3 and np.array_equal(cls, v)
    labels, K, _ = cr.label(v, 6, None)
    assert labels.tolist() == [[[1, 1, 2, 2, 3, 4]]] and K == 4
    assert cr.label(v, 6, -1)[0].tolist() == labels.tolist()
    labels, K, _ = cr.label(v, 6, 1)
    assert labels.tolist() == [[[0, 0, 1, 1, 2, 0]]] and K == 2
    sizes, classes, first = cr.table(*cr.label(v, 6, 0)[::2], 3)
    assert sizes.tolist() == [0, 2, 2, 1] and classes.tolist() == [0, 1, 2, 1] and first.tolist() == [-1, 0, 2, 5]


def test_the_all_zero_voxel_and_the_argmax_tie():
    pred = np.zeros((1, 1, 5, 3), np.uint8)
    pred[0, 0, 0] = (9, 9, 3)          # a tie at the top: the lowest index
    pred[0, 0, 1] = (0, 0, 0)          # never predicted: no component, class map 0
    pred[0, 0, 2] = (1, 7, 7)
    pred[0, 0, 3] = (0, 200, 7)
    pred[0, 0, 4] = (0, 0, 1)
    labels, K, cls = cr.label(pred, 6, None)
    assert cls.tolist() == [[[0, 0, 1, 1, 2]]] and labels.tolist() == [[[1, 0, 2, 2, 3]]] and K == 3
    labels, K, cls = cr.label(pred, 6, 0)
    assert cls.tolist() == [[[0, 0, 1, 1, 2]]] and labels.tolist() == [[[0, 0, 1, 1, 2]]] and K == 2


def _volumes():
    rng = np.random.default_rng(3)
    yield 'binary', (rng.random((9, 20, 70)) < 0.5).astype(np.uint8)
    yield 'four classes', rng.integers(0, 4, (9, 20, 70)).astype(np.uint8)
    yield 'all background', np.zeros((3, 4, 5), np.uint8)
    yield 'one voxel', np.ones((1, 1, 1), np.uint8)
    for C in (2, 3, 16):
        yield f'pred {C}', random_pred((9, 10, 13), C, C)


@pytest.mark.parametrize('conn', CONN)
def test_the_numpy_path_is_the_definition(conn):
    from interactive_unet import components
    for name, v in _volumes():
        for bg in (0, -1, None, 2):
            labels, K, cls = components.label(v, conn, bg)
            want = cr.label(v, conn, bg)
            assert labels.dtype == np.int32 and cls.dtype == np.uint8 and isinstance(K, int), name
            assert K == want[1] and np.array_equal(labels, want[0]) and np.array_equal(cls, want[2]), (name, bg)
            got = components.table(labels, cls, K)
            for g, w, dt in zip(got, cr.table(labels, cls, K), (np.int32, np.uint8, np.int32)):
                assert g.dtype == dt and np.array_equal(g, w), (name, bg)
            keep = np.random.default_rng(K).random(K + 1) < 0.5
            for fill in (0, 7):
                assert np.array_equal(components.filter_components(labels, cls, K, keep, fill), cr.filter_components(labels, cls, keep, fill))


def test_remove_small_and_keep_largest():
    from interactive_unet import components
    #            a run of 3, of 1, of 3 (class 1), of 2 (class 2), of 3 (class 2)
    v = np.array([[[1, 1, 1, 0, 1, 0, 1, 1, 1, 2, 2, 0, 2, 2, 2]]], np.uint8)
    assert components.remove_small(v, 3).tolist() == [[[1, 1, 1, 0, 0, 0, 1, 1, 1, 0, 0, 0, 2, 2, 2]]]
    assert components.remove_small(v, 2, fill=9).tolist() == [[[1, 1, 1, 0, 9, 0, 1, 1, 1, 2, 2, 0, 2, 2, 2]]]
    assert components.remove_small(v, 0).tolist() == v.tolist() and components.remove_small(v, 4).max() == 0
    # every class labelled: the zeros are components too, and the default fill is 0
    assert components.remove_small(v, 3, background=None).tolist() == [[[1, 1, 1, 0, 0, 0, 1, 1, 1, 0, 0, 0, 2, 2, 2]]]
    assert components.remove_small(v, 3, background=2, fill=None).tolist() == [[[1, 1, 1, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2]]]
    # of the two runs of 3 of class 1 the first (the smaller label) is the largest; per class: class 2 keeps its run of 3
    assert components.keep_largest(v).tolist() == [[[1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 2]]]
    assert components.keep_largest(v, per_class=False).tolist() == [[[1, 1, 1] + [0] * 12]]
    assert components.keep_largest(v, n=2, per_class=False).tolist() == [[[1, 1, 1, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0]]]
    assert components.keep_largest(v, n=2).tolist() == [[[1, 1, 1, 0, 0, 0, 1, 1, 1, 2, 2, 0, 2, 2, 2]]]
    assert components.keep_largest(v, n=0, fill=5).tolist() == [[[5, 5, 5, 0, 5, 0, 5, 5, 5, 5, 5, 0, 5, 5, 5]]]
    assert components.keep_largest(np.zeros((2, 2, 2), np.uint8)).max() == 0
    for name, vol in _volumes():
        for conn, bg in ((6, 0), (26, None), (18, 1)):
            for m in (1, 2, 5):
                assert np.array_equal(components.remove_small(vol, m, conn, bg), cr.remove_small(vol, m, conn, bg)), (name, conn, bg, m)
            for n, per in ((1, True), (1, False), (3, True), (2, False)):
                assert np.array_equal(components.keep_largest(vol, n, per, conn, bg, fill=3), cr.keep_largest(vol, n, per, conn, bg, fill=3))


def test_largest_flags_on_torch_tables_are_the_numpy_ones():
    """The resident path's plumbing (torch sorts), on the host."""
    from interactive_unet import components
    rng = np.random.default_rng(5)
    for K in (0, 1, 7, 200):
        sizes = np.concatenate([[0], rng.integers(1, 6, K)]).astype(np.int32)         # many equal sizes
        classes = np.concatenate([[0], rng.integers(0, 4, K)]).astype(np.uint8)
        for n in (0, 1, 3):
            for per in (True, False):
                want = components.largest_flags(sizes, classes, n, per)
                got = components.largest_flags(torch.from_numpy(sizes), torch.from_numpy(classes), n, per)
                assert got.dtype == torch.uint8 and np.array_equal(got.numpy().astype(bool), want), (K, n, per)


def test_tile_is_the_kernels():
    from interactive_unet import components
    text = open(os.path.join(ROOT, 'interactive-unet_amd', 'csrc', 'components.hip')).read()
    m = re.search(r'CC_TZ = (\d+), CC_TY = (\d+), CC_TX = (\d+)', text)
    assert m and tuple(int(g) for g in m.groups()) == components.TILE


def test_host_refusals_need_no_device():
    from interactive_unet import components
    v = np.zeros((4, 5, 6), np.uint8)
    pred = np.zeros((4, 5, 6, 3), np.uint8)
    for bad in (v.astype(np.int32), v[0], pred[..., :1], np.zeros((4, 5, 6, 17), np.uint8), v[:, :, ::2], np.zeros((0, 5, 6), np.uint8),
                torch.from_numpy(v), v.tolist(), None):
        with pytest.raises(ValueError):
            components.label(bad)
        with pytest.raises(ValueError):
            components.remove_small(bad, 2)
        with pytest.raises(ValueError):
            components.keep_largest(bad)
    for conn in (0, 4, 8, 27):
        with pytest.raises(ValueError, match='connectivity'):
            components.label(v, conn)
    for bg in (-2, 256, 0.5, 'a'):
        with pytest.raises(ValueError, match='background'):
            components.label(v, 6, bg)
    for fill in (-1, 256, 1.5):
        with pytest.raises(ValueError, match='fill'):
            components.remove_small(v, 2, fill=fill)
        with pytest.raises(ValueError, match='fill'):
            components.keep_largest(v, fill=fill)
    with pytest.raises(ValueError, match='min_size'):
        components.remove_small(v, -1)
    with pytest.raises(ValueError):
        components.keep_largest(v, n=-1)
    labels = np.zeros((4, 5, 6), np.int32)
    for bad_l, bad_c in ((labels.astype(np.int64), v), (labels, v.astype(np.int8)), (labels[1:], v), (labels, torch.from_numpy(v)),
                         (torch.from_numpy(labels), torch.from_numpy(v)), (labels[:, :, ::2], v[:, :, ::2])):
        with pytest.raises(ValueError):
            components.table(bad_l, bad_c, 0)
        with pytest.raises(ValueError):
            components.filter_components(bad_l, bad_c, 0, np.ones(1, bool), 0)
    with pytest.raises(ValueError, match='count'):
        components.table(labels, v, -1)
    with pytest.raises(ValueError, match='keep'):
        components.filter_components(labels, v, 2, np.ones(2, bool), 0)


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """Argument validation precedes every HIP call."""
    from interactive_unet import _native as nv
    if not os.path.isfile(nv.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    l = nv.lib()
    mem = (ctypes.c_double * 64)()
    buf = ctypes.c_void_p(ctypes.addressof(mem))                                      # never dereferenced: every call below stops before its launch
    odd = ctypes.c_void_p(ctypes.addressof(mem) + 2)

    need = l.iunet_cc_ws_bytes
    a16 = lambda n: (n + 15) // 16 * 16
    assert need(1, 1, 1) == 16 + 16 + 16 and need(37, 41, 150) == a16(4 * 227550) + a16(227550) + a16(4 * 56)
    assert need(1024, 1024, 1024) == 5 * 2 ** 30 + 4 * 2 ** 18 and need(1, 1, 2 ** 31 - 1) > 0
    assert need(0, 4, 4) == 0 and need(4, -1, 4) == 0 and need(4, 4, 0) == 0 and need(2048, 1024, 1024) == 0 and need(2 ** 16, 2 ** 15, 1) == 0

    def lab(src=buf, Z=8, Y=8, X=8, C=1, conn=6, bg=0, labels=buf, cls=None, count=buf, ws=buf, ws_bytes=None):
        ws_bytes = need(Z, Y, X) if ws_bytes is None else ws_bytes
        return l.iunet_cc_label(src, Z, Y, X, C, conn, bg, labels, cls, count, ws, ws_bytes, None), l.iunet_last_error()
    for kw, word in ((dict(src=None), b'null'), (dict(labels=None), b'null'), (dict(count=None), b'null'), (dict(ws=None), b'null'),
                     (dict(Z=0), b'dimension'), (dict(Y=-3), b'dimension'), (dict(X=0), b'dimension'),
                     (dict(Z=2048, Y=1024, X=1024, ws_bytes=1 << 40), b'voxels'), (dict(C=0), b'classes'), (dict(C=17), b'classes'),
                     (dict(conn=0), b'connectivity'), (dict(conn=8), b'connectivity'), (dict(conn=27), b'connectivity'),
                     (dict(bg=-2), b'background'), (dict(bg=256), b'background'), (dict(ws_bytes=need(8, 8, 8) - 1), b'workspace'),
                     (dict(ws_bytes=0), b'workspace'), (dict(ws_bytes=-1), b'workspace'), (dict(labels=odd), b'aligned')):
        rc, msg = lab(**kw)
        assert rc < 0 and word in msg, (kw, msg)
    assert b'null' in lab(src=None, Z=0, Y=0, X=0, C=0, conn=0, labels=None, count=None, ws=None, ws_bytes=0)[1]

    def tab(labels=buf, cls=buf, Z=8, Y=8, X=8, K=3, sizes=buf, classes=buf, first=buf):
        return l.iunet_cc_table(labels, cls, Z, Y, X, K, sizes, classes, first, None), l.iunet_last_error()
    for kw, word in ((dict(labels=None), b'null'), (dict(cls=None), b'null'), (dict(sizes=None), b'null'), (dict(classes=None), b'null'),
                     (dict(first=None), b'null'), (dict(Z=0), b'dimension'), (dict(X=-1), b'dimension'),
                     (dict(Z=2048, Y=1024, X=1024), b'voxels'), (dict(K=-1), b'components'), (dict(K=513), b'components'),
                     (dict(sizes=odd), b'aligned')):
        rc, msg = tab(**kw)
        assert rc < 0 and word in msg, (kw, msg)
    assert b'null' in tab(None, None, 0, 0, 0, 0, None, None, None)[1]

    def fil(labels=buf, cls=buf, Z=8, Y=8, X=8, K=3, keep=buf, fill=0, out=buf):
        return l.iunet_cc_filter(labels, cls, Z, Y, X, K, keep, fill, out, None), l.iunet_last_error()
    for kw, word in ((dict(labels=None), b'null'), (dict(cls=None), b'null'), (dict(keep=None), b'null'), (dict(out=None), b'null'),
                     (dict(Y=0), b'dimension'), (dict(Z=2048, Y=1024, X=1024), b'voxels'), (dict(K=-1), b'components'),
                     (dict(fill=-1), b'fill'), (dict(fill=256), b'fill'), (dict(labels=odd), b'aligned')):
        rc, msg = fil(**kw)
        assert rc < 0 and word in msg, (kw, msg)
    assert b'null' in fil(None, None, 0, 0, 0, 0, None, 0, None)[1]
