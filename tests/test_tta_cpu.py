"""The symmetry ensemble without a GPU: the definition tests/tta_ref.py against hand-written facts and a per-voxel
Python loop, tta.members, the entry points' argument checks and the host refusals that need no device."""
import ctypes
import itertools
import os
import warnings

import numpy as np
import pytest

from tests import tta_ref as tr


def _index_volume(n):
    return np.arange(int(np.prod(n)), dtype=np.int64).reshape(n)


# ---- the restatement
def test_the_48_codes_are_distinct_and_invertible():
    A = _index_volume((3, 4, 5))
    seen = set()
    for sym in range(48):
        B = tr.forward(A, sym)
        perm, flips = tr.decode(sym)
        assert B.shape == tr.shape(A.shape, sym) == tuple(A.shape[perm[a]] for a in range(3))
        assert np.array_equal(tr.inverse(B, sym), A), sym
        seen.add((B.shape, B.tobytes()))
        # the pairing, voxel by voxel: B[t] = A[s], s[perm[a]] = m[a] - 1 - t[a] where bit a is set
        for t in itertools.product(*[range(m) for m in B.shape]):
            s = [0, 0, 0]
            for a in range(3):
                s[perm[a]] = B.shape[a] - 1 - t[a] if (sym & 7) >> a & 1 else t[a]
            assert B[t] == A[tuple(s)], (sym, t)
    assert len(seen) == 48
    assert tr.PERMS == ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def test_hand_written_codes():
    A = _index_volume((3, 4, 5))
    assert np.array_equal(tr.forward(A, 0), A)
    assert np.array_equal(tr.forward(A, 7), A[::-1, ::-1, ::-1])
    assert np.array_equal(tr.forward(A, 8 * 1), A.transpose(0, 2, 1))
    assert np.array_equal(tr.forward(A, 1), A[::-1]) and np.array_equal(tr.forward(A, 4), A[:, :, ::-1])
    assert np.array_equal(tr.forward(A, 8 * 3 + 1), A.transpose(1, 2, 0)[::-1])          # the flip acts on the OUTPUT axis
    # channels ride along
    Q = np.stack([tr.forward(A, 29), -tr.forward(A, 29)], axis=-1)
    assert np.array_equal(tr.inverse(Q, 29), np.stack([A, -A], axis=-1))


def test_ensemble_against_a_per_voxel_loop():
    n, C, syms = (2, 3, 4), 3, (0, 13, 47, 22, 5)
    rng = np.random.default_rng(0)
    Ps = [rng.random(n + (C,), dtype=np.float32) for _ in syms]
    qs = [tr.forward(P, sym) for P, sym in zip(Ps, syms)]
    mean, spread = tr.ensemble(qs, syms)
    assert mean.dtype == np.float32 and spread.dtype == np.float32 and mean.shape == n + (C,) and spread.shape == n
    r = np.float32(1) / np.float32(len(syms))
    for s in itertools.product(*[range(v) for v in n]):
        best = np.float32(0)
        for c in range(C):
            vals = [P[s + (c,)] for P in Ps]
            acc = vals[0]
            for v in vals[1:]:
                acc = np.float32(acc + v)
            assert mean[s + (c,)] == np.float32(acc * r)
            best = max(best, np.float32(max(vals) - min(vals)))
        assert spread[s] == best
    steps = tr.ensemble_steps(qs, syms)
    assert np.array_equal(steps[0][0], Ps[0]) and np.array_equal(steps[1][1], np.minimum(Ps[0], Ps[1]))
    # member order is part of the contract: some voxel's fp32 sum changes with it
    other = tr.ensemble(qs[::-1], syms[::-1])[0]
    assert np.allclose(other, mean, atol=1e-6) and np.array_equal(tr.ensemble(qs[::-1], syms[::-1])[1], spread)


def test_one_member_is_the_member_itself():
    P = np.random.default_rng(1).random((2, 3, 4, 3), dtype=np.float32)
    for sym in (0, 21):
        mean, spread = tr.ensemble([tr.forward(P, sym)], [sym])
        assert np.array_equal(mean, P) and not spread.any()


# ---- tta.members
def test_members():
    from interactive_unet import tta
    assert tta.members(None) is None
    assert tta.members('flips') == tuple(range(8)) and tta.members('planar') == tuple(range(16)) and tta.members('full') == tuple(range(48))
    assert tta.SETS == tr.SETS and tta.PERMS == tr.PERMS
    for name in tta.SETS:
        assert tta.members(name)[0] == 0                                      # the identity comes first
    assert all(tr.decode(s)[0][0] == 0 for s in tta.members('planar'))        # axis 0 stays in place
    assert tta.members([5, 0, 47]) == (5, 0, 47) and tta.members(np.array([3, 2])) == (3, 2) and tta.members((0,)) == (0,)
    for bad in ('mirror', '', [], (), [0, 0], [1, 2, 1], [48], [-1], [0.0], [True], ['flips'], 3, [None]):
        with pytest.raises(ValueError):
            tta.members(bad)
    for sym in range(48):
        assert tta.shape((3, 4, 5), sym) == tr.shape((3, 4, 5), sym)


# ---- through the library, no GPU
def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """Argument validation precedes every HIP call."""
    from interactive_unet import _native as nv
    if not os.path.isfile(nv.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    l = nv.lib()
    mem = (ctypes.c_double * 64)()
    buf = ctypes.c_void_p(ctypes.addressof(mem))                              # never dereferenced: every call below stops before its launch

    def block(src=buf, D=8, H=8, W=8, sym=0, out=buf):
        return l.iunet_sym_block(src, D, H, W, sym, out, None), l.iunet_last_error()
    for kw, word in ((dict(src=None), b'null'), (dict(out=None), b'null'), (dict(D=0), b'volume'), (dict(H=-1), b'volume'), (dict(W=0), b'volume'),
                     (dict(D=1 << 14, H=1 << 14, W=1 << 14), b'volume'), (dict(D=1 << 30, H=1 << 30, W=1 << 30), b'volume'),
                     (dict(sym=-1), b'symmetry'), (dict(sym=48), b'symmetry'),
                     (dict(D=1 << 11, H=1 << 11, W=1 << 11), b'grid'), (dict(D=1 << 11, H=1 << 11, W=1 << 11, sym=16 + 4), b'grid'),
                     (dict(D=1, H=1 << 20, W=1 << 20, sym=8), b'grid')):
        rc, msg = block(**kw)
        assert rc < 0 and word in msg, (kw, msg)
    assert b'null' in block(src=None, D=0, H=0, W=0, out=None)[1]              # the all-zero call stops at the pointer check

    def acc(q=buf, D=8, H=8, W=8, C=2, sym=0, index=0, count=2, inv=0.5, s=buf, mn=buf, mx=buf, mean=buf, spread=buf):
        return l.iunet_sym_accumulate(q, D, H, W, C, sym, index, count, inv, s, mn, mx, mean, spread, None), l.iunet_last_error()
    for kw, word in ((dict(q=None), b'null'), (dict(s=None), b'null'), (dict(mean=None, index=1), b'null'),
                     (dict(mn=None), b'all or none'), (dict(mx=None), b'all or none'), (dict(spread=None), b'all or none'),
                     (dict(mn=None, mx=None), b'all or none'), (dict(mn=None, spread=None), b'all or none'),
                     (dict(D=0), b'volume'), (dict(W=-3), b'volume'), (dict(D=1 << 14, H=1 << 14, W=1 << 14), b'volume'),
                     (dict(C=0), b'classes'), (dict(C=17), b'classes'), (dict(sym=-1), b'symmetry'), (dict(sym=48), b'symmetry'),
                     (dict(count=0), b'count'), (dict(count=49, index=3), b'count'), (dict(index=-1), b'index'), (dict(index=2), b'index'),
                     (dict(D=1 << 11, H=1 << 11, W=1 << 11), b'grid'), (dict(D=1, H=1 << 20, W=1 << 20, sym=8), b'grid'),
                     (dict(D=1 << 12, H=1 << 12, W=1 << 12, C=16, sym=40), b'grid')):
        rc, msg = acc(**kw)
        assert rc < 0 and word in msg, (kw, msg)
    assert b'null' in acc(q=None, D=0, H=0, W=0, C=0, index=0, count=0, inv=0.0, s=None, mn=None, mx=None, mean=None, spread=None)[1]
    # (whole arguments reach the launch only with a device: tests/test_gpu_tta.py)


# ---- the host layer's refusals that need no device
def _model(dim):
    from interactive_unet.unet import UNet
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return UNet(dim=dim, levels=4, base=32, pretrained=False)


def test_predict_refusals_need_no_device():
    import torch
    from interactive_unet import predict
    from interactive_unet.slicer import Slicer
    vol = np.zeros((40, 48, 56), dtype=np.uint8)
    with pytest.raises(ValueError, match='2-D model'):
        predict.predict_volume_array(_model(2), vol, input_size=32, tta='flips')
    with pytest.raises(ValueError, match='2-D model'):
        predict.predict_volume_array(_model(2), vol, input_size=32, tta=[0], return_spread=True)
    for m in (_model(2), _model(3)):
        with pytest.raises(ValueError, match='return_spread'):
            predict.predict_volume_array(m, vol, input_size=32, return_spread=True)
    for bad in ('mirrors', [], [0, 0], [48]):
        with pytest.raises(ValueError, match='tta'):
            predict.predict_volume_array(_model(3), vol, input_size=32, tta=bad)
        with pytest.raises(ValueError, match='tta'):
            predict.predict_slab(_model(3), torch.zeros((40, 48, 56), dtype=torch.uint8), Slicer([40, 48, 56]), slice_width=32, depth=8, tta=bad)
    with pytest.raises(ValueError, match='3-D network'):
        predict.predict_slab(_model(2), torch.zeros((40, 48, 56), dtype=torch.uint8), Slicer([40, 48, 56]), slice_width=32, depth=8, tta='planar')


def test_the_overlay_installs_the_module():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    try:
        import install_overlay
    finally:
        sys.path.pop(0)
    assert 'tta' in install_overlay.ADDED
