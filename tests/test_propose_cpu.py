"""The slice proposal without a GPU: the definition tests/propose_ref.py on hand-made voxels, against a second
statement of the brick sums, against the slab's gather and the slicer's own coordinates; the host layer's numpy path against the
definition; the planted-blob case; the host refusals and the entry points' argument checks."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import propose_ref as pr
from tests import slab_ref as sr
from tests.volume_inputs import random_pred

E = np.eye(3)
VOXELS = (((255, 0), 0), ((128, 127), 254), ((100, 100), 255), ((0, 0), 0), ((10, 200, 200), 255), ((7, 0, 0), 248))


def _sparse(shape, ch, seed, zero_share=0.7):
    rng = np.random.default_rng(seed)
    v = rng.integers(1, 256, tuple(shape) + ((ch,) if ch else ()), dtype=np.uint8)
    v[rng.random(v.shape) < zero_share] = 0
    return v


@pytest.mark.parametrize('q,want', VOXELS)
def test_hand_made_voxels(q, want):
    assert pr.voxel_uncertainty(q) == want
    pred = np.array(q, dtype=np.uint8).reshape(1, 1, 1, -1)
    assert pr.uncertainty(pred).tolist() == [[[want]]]
    one, nil = np.full((1, 1, 1), 9, np.uint8), np.zeros((1, 1, 1), np.uint8)
    # annotated through either weight channel, or dark: 0; an empty weight and a bright image change nothing
    assert pr.voxel_uncertainty(q, weight=(9,)) == 0 and pr.voxel_uncertainty(q, weight=(0, 9)) == 0 and pr.voxel_uncertainty(q, weight=(9, 0)) == 0
    assert pr.voxel_uncertainty(q, dark=True) == 0 and pr.voxel_uncertainty(q, weight=(0, 0)) == want
    for w in (one, one[..., None], np.stack([one, nil], -1), np.stack([nil, one], -1)):
        assert pr.uncertainty(pred, weight=w).tolist() == [[[0]]]
    assert pr.uncertainty(pred, image=nil).tolist() == [[[0]]]
    assert pr.uncertainty(pred, image=np.stack([nil, one, one], -1)).tolist() == [[[0]]]          # channel 0 alone decides
    assert pr.uncertainty(pred, weight=np.stack([nil, nil], -1), image=np.stack([one, nil, nil], -1)).tolist() == [[[want]]]


def test_random_tie_and_zero_shares():
    pred = random_pred((9, 10, 13), 3, 0)
    u = pr.uncertainty(pred)
    never, tie = (pred.max(-1) == 0), (u == 255)
    assert 0.03 < never.mean() < 0.2 and 0.03 < tie.mean() < 0.2 and not u[never].any()
    for z, y, x in ((0, 0, 0), (8, 9, 12), (4, 5, 6), (3, 0, 11)):
        assert u[z, y, x] == pr.voxel_uncertainty(pred[z, y, x])


def test_brick_sums_on_a_ragged_volume():
    shape, g = (9, 10, 13), 4
    u = pr.uncertainty(random_pred(shape, 2, 1))
    want = np.zeros((3, 3, 4), dtype=np.int64)
    for z in range(shape[0]):
        for y in range(shape[1]):
            for x in range(shape[2]):
                want[z // g, y // g, x // g] += int(u[z, y, x])
    got = pr.brick_sums(u, g)
    assert got.dtype == np.uint32 and got.shape == (3, 3, 4) and np.array_equal(got, want) and want.min() > 0


def _slicer(seed, shape):
    """As tests/test_gpu_slab.py draws them."""
    from interactive_unet.slicer import Slicer
    np.random.seed(seed)
    s = Slicer(list(shape))
    s.randomize()
    s.origin = np.array(shape) / 2 + np.random.uniform(-1, 1, 3)
    return s


@pytest.mark.parametrize('seed', range(4))
def test_plane_score_is_the_slab_gathers_sum_and_the_slicers_points(seed):
    shape = (20, 24, 28)
    u = np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    s = _slicer(seed, shape)
    for axis in range(3):
        a, b, n, o = sr.slicer_geometry(s, axis)
        for sw in (13, 16):
            score, inside = pr.plane_score(u, (a, b, o), sw)
            assert score == int(sr.gather(u, (a, b, n, o), 1, sw, 0).astype(np.int64).sum()), (axis, sw)
            c = s.get_interpolation_coords(slice_width=sw)[axis]
            assert np.array_equal(pr.plane_coords((a, b, o), sw), c)
            hi = (np.array(shape) - 1.0)[:, None, None]
            assert inside == int(((c >= 0) & (c <= hi)).all(axis=0).sum()), (axis, sw)
            assert 0 < inside <= sw * sw and score > 0


def test_plane_wholly_outside_scores_nothing():
    u = np.full((20, 24, 28), 200, dtype=np.uint8)
    assert pr.plane_score(u, (E[1], E[2], np.array([-100.0, 5.0, 400.0])), 16) == (0, 0)
    assert pr.plane_score(u, (E[1], E[2], np.array([10.0, 12.0, 14.0])), 16) == (200 * 256, 256)
    # exactly on the faces: inside; a hair beyond: outside
    assert pr.plane_score(u, (E[1], E[2], np.array([19.0, 8.0, 8.0])), 16) == (200 * 256, 256)
    assert pr.plane_score(u, (E[1], E[2], np.array([19.0 + 1e-9, 8.0, 8.0])), 16) == (0, 0)


# ---- the production numpy path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', (2, 3, 16))
def test_numpy_uncertainty_is_the_definition(C):
    from interactive_unet import propose
    shape = (9, 10, 13)
    pred = random_pred(shape, C, C)
    for weight in (None, _sparse(shape, 0, 1), _sparse(shape, 1, 2), _sparse(shape, 2, 3)):
        for image in (None, _sparse(shape, 0, 4, 0.2), _sparse(shape, 3, 5, 0.2)):
            want = pr.uncertainty(pred, weight, image)
            for g in pr.BRICKS:
                u, bricks = propose.uncertainty(pred, weight, image, brick=g)
                assert u.dtype == np.uint8 and np.array_equal(u, want)
                assert bricks.dtype == np.uint32 and np.array_equal(bricks, pr.brick_sums(want, g))
            if weight is not None:
                assert (want == 0).mean() > (pr.uncertainty(pred) == 0).mean()


def test_numpy_score_planes_is_the_definition():
    from interactive_unet import propose
    shape = (20, 24, 28)
    u = np.random.default_rng(7).integers(0, 256, shape, dtype=np.uint8)
    s = _slicer(2, shape)
    planes = [(a, b, o) for axis in range(3) for a, b, _, o in (sr.slicer_geometry(s, axis),)]
    planes += [(E[1], E[2], np.array([-100.0, 5.0, 400.0])), (E[2], E[0], np.array([10.5, 11.5, 12.5])), (E[0], E[1], np.array([0.0, 23.0, 27.0]))]
    for sw in (13, 16, 70):
        got = propose.score_planes(u, np.array(planes), slice_width=sw)
        assert got.dtype == np.int64 and got.shape == (len(planes), 2)
        assert np.array_equal(got, pr.score_planes(u, planes, sw))
    assert got[3].tolist() == [0, 0]


def test_candidate_origins_rank_and_centre():
    from interactive_unet import propose
    shape, g = (9, 10, 13), 4
    bricks = np.zeros((3, 3, 4), dtype=np.uint32)
    bricks[2, 2, 3], bricks[0, 1, 2], bricks[1, 0, 0], bricks[0, 0, 1] = 50, 70, 50, 50              # three equal sums
    got = propose.candidate_origins(bricks, g, shape, 8)
    assert got.dtype == np.float64 and np.array_equal(got, pr.candidate_origins(bricks, g, shape, 8))
    # sum descending, equal sums by ascending flat index, zeros dropped; ragged bricks centred on their in-volume part
    assert got.tolist() == [[1.5, 5.5, 9.5], [1.5, 1.5, 5.5], [5.5, 1.5, 1.5], [8.0, 8.5, 12.0]]
    assert propose.candidate_origins(bricks, g, shape, 2).tolist() == got[:2].tolist()
    assert propose.candidate_origins(np.zeros((3, 3, 4), np.uint32), g, shape, 8).shape == (0, 3)
    rnd = np.random.default_rng(0).integers(0, 5, (5, 6, 7)).astype(np.uint32)                      # many ties
    assert np.array_equal(propose.candidate_origins(rnd, 8, (40, 48, 50), 64), pr.candidate_origins(rnd, 8, (40, 48, 50), 64))
    assert np.array_equal(propose.candidate_origins(torch.tensor(rnd.astype(np.int32)), 8, (40, 48, 50), 64),
                          pr.candidate_origins(rnd, 8, (40, 48, 50), 64))


# ---- the planted blob ------------------------------------------------------------------------------------------------------
BLOB_SHAPE, BLOB_CENTRE, BLOB_RADIUS = (32, 40, 48), (20, 12, 30), 5
BLOB_KW = dict(slice_width=16, brick=8, candidates=4, orientations=4)


def _blob():
    """Confident (255, 0) everywhere but a ball, which carries (128, 127); and a weight volume that covers the ball."""
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


def _restated(shape, pred, found, generator, weight=None, image=None, slice_width=256, axis=0, brick=8, candidates=32, orientations=8):
    """propose_slices in 'random' mode from the definition: the same draws, the definition's numbers."""
    from interactive_unet.slicer import Slicer
    u = pr.uncertainty(pred, weight, image)
    origins = pr.candidate_origins(pr.brick_sums(u, brick), brick, shape, candidates)
    s, planes, vecs = Slicer(list(shape)), [], []
    for o in origins:
        for _ in range(orientations):
            v = torch.randn(3, dtype=torch.float64, generator=generator).numpy()
            assert np.linalg.norm(v) >= 1e-4
            v = v / np.linalg.norm(v)
            s.update_orientation_vectors(v)
            a, b = ((s.v, s.w), (s.u, s.w), (s.u, s.v))[axis]
            planes.append((a, b, o))
            vecs.append(v)
    scores = pr.score_planes(u, planes, slice_width)
    want = [{'rot_vec': vecs[p], 'origin': planes[p][2], 'score': int(scores[p][0]), 'inside': int(scores[p][1]), 'sampling_axis': None}
            for p in pr.rank(scores)]
    return _same(found, want)


def test_propose_slices_on_the_planted_blob():
    from interactive_unet import propose
    pred, _ = _blob()
    found = propose.propose_slices(BLOB_SHAPE, pred, generator=_gen(), **BLOB_KW)
    assert len(found) == 16
    for f in found:
        assert (np.abs(f['origin'] - np.array(BLOB_CENTRE)) <= BLOB_RADIUS + 8 / 2).all(), f['origin']
        assert abs(np.linalg.norm(f['rot_vec']) - 1) < 1e-12 and 0 < f['inside'] <= 256 and f['sampling_axis'] is None
    assert found[0]['score'] > 0 and [f['score'] for f in found] == sorted((f['score'] for f in found), reverse=True)
    assert _same(found, propose.propose_slices(BLOB_SHAPE, pred, generator=_gen(), **BLOB_KW))      # the same seed: equal
    assert not _same(found, propose.propose_slices(BLOB_SHAPE, pred, generator=_gen(12), **BLOB_KW))
    assert _restated(BLOB_SHAPE, pred, found, _gen(), **BLOB_KW)
    for axis in (1, 2):
        assert _restated(BLOB_SHAPE, pred, propose.propose_slices(BLOB_SHAPE, pred, generator=_gen(), axis=axis, **BLOB_KW), _gen(), axis=axis, **BLOB_KW)


def test_propose_slices_on_random_bytes_with_weight_and_image():
    from interactive_unet import propose
    shape = (17, 31, 22)
    pred, weight, image = random_pred(shape, 3, 8), _sparse(shape, 2, 9, 0.9), _sparse(shape, 0, 10, 0.2)
    kw = dict(weight=weight, image=image, slice_width=13, brick=4, candidates=5, orientations=3)
    found = propose.propose_slices(shape, pred, generator=_gen(3), **kw)
    assert len(found) == 15 and _restated(shape, pred, found, _gen(3), **kw)


def test_a_proposal_is_a_plane_the_slicer_holds():
    """The score of a proposal is the definition's score of the plane a slicer holds after update_orientation_vectors(rot_vec)."""
    from interactive_unet import propose
    from interactive_unet.slicer import Slicer
    pred, _ = _blob()
    u = pr.uncertainty(pred)
    for mode, kw in (('random', {}), ('grid', {}), ('grid', dict(sampling_axis='y'))):
        found = propose.propose_slices(BLOB_SHAPE, pred, generator=_gen(), sampling_mode=mode, axis=1, **BLOB_KW, **kw)
        assert len(found) == {'random': 16, 'grid': 12}[mode] // (3 if kw else 1)
        for f in found:
            s = Slicer(list(BLOB_SHAPE))
            s.update_orientation_vectors(f['rot_vec'])
            assert pr.plane_score(u, (s.u, s.w, f['origin']), 16) == (f['score'], f['inside'])
            if mode == 'grid':
                assert f['sampling_axis'] in ('y' if kw else 'xyz') and f['rot_vec'].tolist() == E['xyz'.index(f['sampling_axis'])].tolist()


def test_nothing_left_to_propose_falls_back_to_randomize():
    from interactive_unet import propose
    from interactive_unet.slicer import Slicer
    pred, weight = _blob()
    assert propose.propose_slices(BLOB_SHAPE, pred, weight=weight, generator=_gen(), **BLOB_KW) == []
    assert propose.propose_slices(BLOB_SHAPE, pred, weight=np.stack([np.zeros_like(weight), weight], -1), generator=_gen(), **BLOB_KW) == []
    s = Slicer(list(BLOB_SHAPE))
    np.random.seed(4)
    assert propose.next_slice(s, pred, weight=weight, generator=_gen(), sampling_mode='grid', sampling_axis='z', **BLOB_KW) == []
    t = Slicer(list(BLOB_SHAPE))
    np.random.seed(4)
    t.randomize(sampling_mode='grid', sampling_axis='z')
    assert s.sampling_axis == 'z' and np.array_equal(s.rot_vec, t.rot_vec) and np.array_equal(s.origin, t.origin) and np.array_equal(s.w, t.w)


def test_next_slice_sets_the_slicer_to_the_best_proposal():
    from interactive_unet import propose
    from interactive_unet.slicer import Slicer
    pred, _ = _blob()
    s = Slicer(list(BLOB_SHAPE))
    found = propose.next_slice(s, pred, generator=_gen(), **BLOB_KW)
    assert _same(found, propose.propose_slices(BLOB_SHAPE, pred, generator=_gen(), **BLOB_KW))
    t = Slicer(list(BLOB_SHAPE))
    t.update_orientation_vectors(found[0]['rot_vec'])
    assert all(np.array_equal(getattr(s, k), getattr(t, k)) for k in ('rot_vec', 'rot_mat', 'u', 'v', 'w'))
    assert np.allclose(s.rot_vec, found[0]['rot_vec'], atol=1e-14) and np.array_equal(s.origin, found[0]['origin']) and s.sampling_axis == 'random'
    s.origin += 1.0                                                                     # the slicer owns its origin
    assert not np.array_equal(s.origin, found[0]['origin'])
    found = propose.next_slice(s, pred, generator=_gen(), sampling_mode='grid', sampling_axis='x', **BLOB_KW)
    assert s.sampling_axis == 'x' and len(found) == 4 and s.rot_vec.tolist() == [1.0, 0.0, 0.0] and np.array_equal(s.origin, found[0]['origin'])


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_host_refusals_need_no_device():
    from interactive_unet import propose
    pred, weight = _blob()
    ok = dict(generator=_gen(), **BLOB_KW)
    for bad in (pred.astype(np.float32), pred[..., 0], pred[..., :1], np.zeros(BLOB_SHAPE + (17,), np.uint8), pred[:, :, ::2],
                torch.from_numpy(pred), pred.tolist(), None):
        with pytest.raises(ValueError):
            propose.uncertainty(bad)
    for bad in (weight[1:], weight.astype(np.int32), np.stack([weight] * 3, -1), torch.from_numpy(weight), weight[:, ::2][:, :20]):
        with pytest.raises(ValueError):
            propose.uncertainty(pred, weight=bad)
    for bad in (weight[1:], weight.astype(np.float64), np.stack([weight] * 5, -1), torch.from_numpy(weight)):
        with pytest.raises(ValueError):
            propose.uncertainty(pred, image=bad)
    for g in (0, 2, 5, 64):
        with pytest.raises(ValueError, match='brick'):
            propose.uncertainty(pred, brick=g)
    u = np.zeros(BLOB_SHAPE, np.uint8)
    plane = np.array([[E[1], E[2], [4.0, 4.0, 4.0]]])
    for bad_u in (u.astype(np.int16), u[0], torch.from_numpy(u), u.tolist()):
        with pytest.raises(ValueError):
            propose.score_planes(bad_u, plane, 16)
    for bad_planes in (plane[0], plane[:, :2], np.zeros((0, 3, 3)), np.full((1, 3, 3), np.nan)):
        with pytest.raises(ValueError):
            propose.score_planes(u, bad_planes, 16)
    for sw in (0, 4097):
        with pytest.raises(ValueError, match='slice width'):
            propose.score_planes(u, plane, sw)
    with pytest.raises(ValueError, match='shape'):
        propose.propose_slices((32, 40, 47), pred, **ok)
    for kw in (dict(sampling_mode='spiral'), dict(sampling_mode='grid', sampling_axis='w'), dict(axis=3), dict(candidates=0), dict(orientations=0)):
        with pytest.raises(ValueError):
            propose.propose_slices(BLOB_SHAPE, pred, **{**ok, **kw})


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """Argument validation precedes every HIP call."""
    from interactive_unet import _native as nv
    if not os.path.isfile(nv.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    l = nv.lib()
    mem = (ctypes.c_double * 64)()
    buf = ctypes.c_void_p(ctypes.addressof(mem))                                      # never dereferenced: every call below stops before its launch

    def unc(pred=buf, Z=8, Y=8, X=8, C=2, weight=None, wch=0, image=None, ich=0, brick=8, u=buf, bricks=buf):
        return l.iunet_uncertainty_volume(pred, Z, Y, X, C, weight, wch, image, ich, brick, u, bricks, None), l.iunet_last_error()
    for kw, word in ((dict(pred=None), b'null'), (dict(u=None, bricks=None), b'null'), (dict(C=1), b'classes'), (dict(C=17), b'classes'),
                     (dict(weight=buf, wch=0), b'weight channels'), (dict(weight=buf, wch=3), b'weight channels'),
                     (dict(image=buf, ich=0), b'image channels'), (dict(image=buf, ich=5), b'image channels'), (dict(brick=0), b'brick'),
                     (dict(brick=12), b'brick'), (dict(brick=64), b'brick'), (dict(Z=0), b'volume'), (dict(X=-1), b'volume'),
                     (dict(Z=1 << 14, Y=1 << 14, X=1 << 14), b'volume'), (dict(Z=1 << 20, Y=1 << 20, X=1, brick=4), b'grid')):
        rc, msg = unc(**kw)
        assert rc < 0 and word in msg, (kw, msg)
    assert b'null' in unc(pred=None, Z=0, C=0, brick=0, u=None, bricks=None)[1]          # the all-zero call stops at the pointer check

    need = l.iunet_plane_scores_ws_bytes
    assert need(1, 1) == 8 and need(1, 64) == 4 * 8 and need(1, 65) == 2 * 5 * 8 and need(256, 256) == 256 * 4 * 16 * 8
    assert need(65535, 4096) == 65535 * 64 * 256 * 8
    assert need(0, 16) == 0 and need(65536, 16) == 0 and need(4, 0) == 0 and need(4, 4097) == 0

    def scores(u=buf, Z=8, Y=8, X=8, geoms=buf, P=2, sw=16, ws=buf, ws_bytes=None, out=buf):
        ws_bytes = need(P, sw) if ws_bytes is None else ws_bytes
        return l.iunet_plane_scores(u, Z, Y, X, geoms, P, sw, -(sw // 2), ws, ws_bytes, out, None), l.iunet_last_error()
    for kw, word in ((dict(u=None), b'null'), (dict(geoms=None), b'null'), (dict(ws=None), b'null'), (dict(out=None), b'null'),
                     (dict(Y=0), b'volume'), (dict(Z=1 << 14, Y=1 << 14, X=1 << 14), b'volume'), (dict(P=0), b'planes'),
                     (dict(P=65536), b'planes'), (dict(sw=0), b'slice width'), (dict(sw=4097), b'slice width'),
                     (dict(ws_bytes=need(2, 16) - 1), b'workspace'), (dict(ws_bytes=0), b'workspace'), (dict(ws_bytes=-1), b'workspace')):
        rc, msg = scores(**kw)
        assert rc < 0 and word in msg, (kw, msg)
    assert b'null' in scores(u=None, Z=0, P=0, sw=0, geoms=None, ws=None, out=None, ws_bytes=0)[1]
