"""The case tables of tests/test_gpu_coarse_matrix.py without a GPU: the library's host-only row counts against their Python restatement, the
branches each table is there for, the numpy adjoint against F.interpolate, and, for every case, the conditions on the reference that make its
comparison legitimate (the margin of the probabilities around 0.5, the exact regimes of the head backward and of the dropout).  A table edit
that silently leaves a branch, or leaves the exact regime, fails here before anyone needs a GPU."""
import os

import numpy as np
import pytest
import torch

import tests.test_gpu_coarse_matrix as M


@pytest.fixture(scope='module')
def lib():
    from interactive_unet import _native
    if not os.path.isfile(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _native.lib()


def rows_of(nd, coarse, s):
    return -(-M.vox_of(M.fine_of(nd, coarse, s)) // M.UPL_PER)


# ---------------------------------------------------------------------------------------------------------------- launch arithmetic
def test_row_counts(lib):
    for nd, coarse, s, ncls, N in M.LOSS_TABLE:
        vox = M.vox_of(M.fine_of(nd, coarse, s))
        assert lib.iunet_dl_up_loss_num_parts(N, vox) == M.parts(N, vox, M.UPL_PER) == N * rows_of(nd, coarse, s)
        assert vox <= 6000
    for C, ncls, N, sp in M.HB_CASES:
        assert lib.iunet_dl_head_bwd_parts(N, M.vox_of(sp)) == M.parts(N, M.vox_of(sp), M.HB_PER)
    assert lib.iunet_dl_up_loss_num_parts(0, 5) < 0 and lib.iunet_dl_head_bwd_parts(3, 0) < 0          # refused, no launch


def test_loss_table_branches():
    for nd in (2, 3):
        rows = [r for r in M.LOSS_TABLE if r[0] == nd]
        vox = lambda r: M.vox_of(M.fine_of(*r[:3]))          # noqa: E731
        assert any(vox(r) > M.UPL_PER and vox(r) % M.UPL_PER != 0 and vox(r) % 256 != 0 for r in rows)          # several rows, the last ragged mid-iteration
        assert any(vox(r) > M.UPL_PER and vox(r) % M.UPL_PER == 0 for r in rows)                                # exactly full rows
        assert {2, 10} <= {r[3] for r in rows}                                                                 # case 2 and the default: arm
        assert any(1 in r[1] for r in rows)                                                                    # a coarse extent of 1
        assert any(r[4] == 3 for r in rows)
        cases = [c for c in M.LOSS_CASES if c[0] == nd]
        assert {c[5] for c in cases} == {'f32', 'f16'} and {c[6] for c in cases} == {False, True}
        assert {c[7] for c in cases} == set(M.metrics_ref.KINDS)
        for r in rows:
            assert {(c[5], c[6]) for c in cases if c[:5] == r} == set(M.CROSS)                                  # every row meets the whole crossing
    # the scale factors 1 and 64, dl_up_check's bounds, fit in 2-D alone (64^3 voxels are no quick test); resample_axis_corners is the same code per axis
    assert {1, 64} <= {r[2] for r in M.LOSS_TABLE if r[0] == 2}
    assert all(c[7] == 'dice_ce' for c in M.LOSS_CASES if c[:3] in M.TWO_ROW) and all(rows_of(*k) == 2 for k in M.TWO_ROW)
    assert len(M.LOSS_CASES) == 4 * len(M.LOSS_TABLE)


def test_head_bwd_and_dropout_and_pool_tables():
    vox = [M.vox_of(sp) for _, _, _, sp in M.HB_CASES]
    assert any(v < M.HB_PER and v % 256 for v in vox) and any(v > M.HB_PER and v % M.HB_PER and v % 256 for v in vox)
    assert {8, 256} <= {c for c, *_ in M.HB_CASES} and (256 // 8 + 1) * 80 > 256          # one plane; the reduce over several workgroups
    assert {2, 10} <= {k for _, k, *_ in M.HB_CASES} and {1, 3} <= {n for _, _, n, _ in M.HB_CASES}
    assert all(v % 256 for _, _, v in M.DROP_SHAPES) and {1, 3} <= {n for _, n, _ in M.DROP_SHAPES}
    n1 = [(N * C, C * C, C * Cb, N * Cb) for N, Cb, C in M.POOL_CASES]
    assert any(a > 256 and b > 256 and c > 256 and a % 256 and b % 256 and c % 256 for a, b, c, _ in n1)          # every kernel multi-workgroup, ragged
    assert any(a > b for a, b, _, _ in n1) and any(a < b for a, b, _, _ in n1)                                  # both arms of n1
    assert any(C > 256 for _, _, C in M.POOL_CASES)


# ---------------------------------------------------------------------------------------------------------------- the references
def axis_pairs():
    return sorted({(e, s) for nd, coarse, s, _, _ in M.LOSS_TABLE for e in coarse})


def test_numpy_adjoint_is_the_transpose_of_interpolate():
    """<up(a), b> = <a, adj(b)> in float64, for every (Ec, s) of the table (as the height and as the width of a 2-D grid)."""
    g = M.gen(41)
    for Ec, s in axis_pairs():
        for coarse in ((Ec, 3), (2, Ec)):
            a = torch.randn((2, 3) + coarse, generator=g, dtype=torch.float64)
            up = M.upsample64(a, 2, s)
            b = torch.randn(up.shape, generator=g, dtype=torch.float64)
            adj = M.adjoint2d(b.numpy(), *coarse)
            lhs, rhs = (up * b).sum().item(), float((a.numpy() * adj).sum())
            assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), (Ec, s, lhs, rhs)
            A = M.interp_matrix(coarse[0], coarse[0] * s)
            assert np.allclose(A.sum(1), 1.0, atol=1e-15) and A.min() >= 0


def test_dyadic_pair_has_exact_fp32_weights():
    Ec, s = M.DYADIC
    assert (2, (3, 7), 3, 5, 3) in M.LOSS_TABLE and (Ec * s - 1) % (Ec - 1) == 0 and (Ec * s - 1) // (Ec - 1) == 4
    i0, f = M.lerp_weights_f32(Ec, Ec * s)
    assert np.array_equal(f * 4, np.round(f * 4)) and f.min() >= 0 and f.max() < 1 and M.src_delta(Ec, Ec * s) == 0.0
    A = M.interp_matrix(Ec, Ec * s)
    assert np.array_equal(A[np.arange(Ec * s), i0], 1.0 - f.astype(np.float64))          # the fp32 weights ARE the exact ones
    assert M.src_delta(7, 21) > 0          # the height pair of the same row is not


def test_source_coordinate_error_is_small():
    """resample_axis_corners in numpy float32: f stays in [0, 1] and the weights are within src_delta (at most 1e-6 here) of the exact ones, for every pair."""
    for Ec, s in axis_pairs():
        i0, f = M.lerp_weights_f32(Ec, Ec * s)
        assert f.min() >= 0 and f.max() <= 1 and 0 <= i0.min() and i0.max() <= Ec - 1
        assert M.src_delta(Ec, Ec * s) <= 1e-6
        if Ec == 1 or s == 1:
            assert M.src_delta(Ec, Ec * s) == 0.0 and not f.any()


@pytest.mark.parametrize('nd,coarse,s,ncls,N', M.LOSS_TABLE)
def test_loss_logits_keep_the_margin(nd, coarse, s, ncls, N):
    lc, factor, _, _ = M.loss_logits(nd, coarse, s, ncls, N)
    p = torch.softmax(M.upsample64(lc, nd, s), 1)
    assert lc.dtype == torch.float32 and (p - 0.5).abs().min().item() >= M.MARGIN
    assert (p.max(1).values > 0.5).float().mean().item() >= M.DECIDED


@pytest.mark.parametrize('case', M.LOSS_CASES, ids=str)
def test_loss_reference_is_sound(case):
    nd, coarse, s, ncls, N, td, weighted, kind = case
    y, wt = M.loss_data(nd, coarse, s, ncls, N, td, weighted)
    T = M.TDTYPE[td][1]
    assert torch.equal(y.to(T).float(), y) and (wt is None or torch.equal(wt.to(T).float(), wt))          # both sides read the same numbers
    assert weighted == (wt is not None)
    if weighted:
        assert 0.2 < (wt == 0).float().mean().item() < 0.4 and wt[wt > 0].min().item() >= 0.5 and not bool(y[wt == 0].any())
    ref = M.loss_reference(*case)
    assert np.isfinite(ref['loss']) and all(np.isfinite(ref['rounded'])) and bool(torch.isfinite(ref['dcoarse']).all())
    assert ref['dcoarse'].abs().max().item() > 1e-6
    if nd == 2:          # the float64 adjoint of the float64 fine gradient is autograd's coarse gradient: the isolated check and the end-to-end one agree
        adj = M.adjoint2d(ref['dfine'].numpy(), *coarse)
        assert np.abs(adj - ref['dcoarse'].numpy()).max() <= 1e-12 * max(1.0, ref['dcoarse'].abs().max().item())
        # a fine index that one axis pass's window missed changes dcoarse by its weight x its input; the bound allows it 1e-5 of that at most
        Hf, Wf = M.fine_of(nd, coarse, s)
        assert max(M.worst_axis_factor(coarse[0], Hf), M.worst_axis_factor(coarse[1], Wf)) <= 1e-5
        print('share of the adjoint bound taken by the emulated fp32 weights:', M.check_adjoint_bound(ref['dfine'].numpy() * M.LSCALE, *coarse))


@pytest.mark.parametrize('C,ncls,N,sp', M.HB_CASES)
def test_head_bwd_is_exact(C, ncls, N, sp):
    M.check_head_bwd_exact(C, ncls, N, sp)


@pytest.mark.parametrize('p', M.DROP_P)
@pytest.mark.parametrize('C,N,vox', M.DROP_SHAPES)
def test_dropout_is_exact(C, N, vox, p):
    M.check_dropout_exact(C, N, vox, p)
    for T in M.DT.values():
        for mode in (0, 1):
            plain, masked = M.dropout_ref(C, N, vox, p, mode, False, T), M.dropout_ref(C, N, vox, p, mode, True, T)
            assert plain.dtype == T and not torch.equal(plain, masked)
    if p == 0.1:          # keep is inexact: the product is not representable in T somewhere, the one rounding matters
        scale, shift, y, mask = M.dropout_data(C, N, vox, p)
        prod = (y * M.keep_of(p))[mask.bool()]
        assert bool((prod.to(torch.float16).float() != prod).any())


def test_pool_reference_is_finite():
    for N, Cb, C in M.POOL_CASES:
        M.check_pool_conditioning(N, Cb, C)
        ref = M.pool_reference(N, Cb, C)
        assert all(bool(torch.isfinite(v).all()) for v in ref.values())
        assert ref['dwproj'].shape == (C, C) and ref['dwpool'].shape == (C, Cb) and ref['dxmean'].shape == (N, Cb)
