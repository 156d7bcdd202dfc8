"""The case tables of tests/test_gpu_decoder_matrix.py without a GPU: its Python restatements of the launch arithmetic against the library's
host-only functions, the branch each table row is there for, and, for every case, the conditions on the reference that make a bit-for-bit
comparison legitimate (partial-sum bounds, sum-of-squares bounds of the statistics rows, representability of the resampled operand).
A table edit that silently leaves a branch, or leaves the exact regime, fails here before anyone needs a GPU."""
import os

import pytest

import tests.test_gpu_decoder_matrix as M
from tests.test_gpu_kernel_matrix import dhw


@pytest.fixture(scope='module')
def lib():
    from interactive_unet import _native
    if not os.path.isfile(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _native.lib()


N3 = M.N3


# ---------------------------------------------------------------------------------------------------------------- launch arithmetic
def test_lk_forward_geometry(lib):
    seen = set()
    for kind, nd, cin, cout in M.LK_FWD:
        sp = M.GRID[nd]
        D, H, W = dhw(nd, sp)
        cols, groups, blocks = M.lk_fwd_geometry(kind, nd, N3, sp, cout)
        assert lib.iunet_lk_stats_parts(nd, kind, N3, D, H, W, cout) == blocks * M.lk_classes(nd, kind)
        per, share = M.gg_fwd_share(cols, blocks)
        assert blocks == 4 and min(share) > 0 and max(share) > 8 and cols % 16 != 0 and M.vox(sp) % 16 != 0          # blocks > 1, several tiles per wave, ragged
        seen.add((groups, (cout - 64 * (groups - 1)) // 16))
    assert seen == {(1, 3), (2, 1), (2, 4)}          # row groups > 1, with a short last group
    c = M.CAP
    D, H, W = dhw(c['nd'], c['sp'])
    cols, groups, blocks = M.lk_fwd_geometry(c['kind'], c['nd'], c['N'], c['sp'], c['cout'])
    assert lib.iunet_lk_stats_parts(c['nd'], c['kind'], c['N'], D, H, W, c['cout']) == 256 == blocks * 4
    assert M.gg_fwd_share(cols, blocks)[1][61:] == [0, 0, 0]          # empty blocks under the cap


def test_lk_wgrad_geometry(lib):
    for kind, nd, cin, cout in M.LK_WGRAD:
        sp = M.L2 if nd == 2 else M.L3
        D, H, W = dhw(nd, sp)
        per = M.lk_classes(nd, kind) * cout * M.lk_taps(nd, kind) * cin
        splits = M.lk_wgrad_splits(nd, kind, N3 * M.vox(sp), cin, cout)
        assert lib.iunet_lk_wgrad_slab_floats(nd, kind, N3, D, H, W, cin, cout) == splits * per and splits == 2
    h = M.LK_HALVED
    D, H, W = dhw(h['nd'], h['sp'])
    per = 4 * h['cout'] * 4 * h['cin']
    assert lib.iunet_lk_wgrad_slab_floats(h['nd'], h['kind'], h['N'], D, H, W, h['cin'], h['cout']) == per          # 3 splits halved to 1
    assert -(-h['N'] * M.vox(h['sp']) // 2048) == 3 and 3 * per > 8 << 20


def test_dl_geometry(lib):
    for nd, rate, taps, cin, cout in M.DL_FWD:
        sp = M.GRID[nd]
        D, H, W = dhw(nd, sp)
        assert lib.iunet_dl_num_taps(nd, rate, D, H, W) == len(M.dl_kept(nd, rate, sp)) == taps
        assert lib.iunet_dl_stats_parts(N3, D, H, W, cout) == M.gg_fwd_blocks(N3 * M.vox(sp), -(-cout // 64)) == 4
    assert {c for _, _, _, c, _ in M.DL_FWD} == {8, 24, 64} and {c for *_, c in M.DL_FWD} == {16, 80}          # Cin 8 and 24
    for nd in (2, 3):
        kept = sorted(t for _, t in M.DL_RATES[nd])
        assert kept[0] == 1 and kept[-1] == 3 ** nd and any(1 < t < 3 ** nd for t in kept)          # 1x1, all taps, partly pruned
        D, H, W = dhw(nd, M.GRID[nd])
        assert sum(lib.iunet_dl_num_taps(nd, r, D, H, W) for r in M.ASPP[nd]) == (14 if nd == 2 else 40) <= 96          # four branches, one tap table
    for nd, rate, cin, cout in M.DL_WGRAD:
        sp = M.GRID[nd]
        D, H, W = dhw(nd, sp)
        K = len(M.dl_kept(nd, rate, sp)) * cin
        splits = M.gg_wgrad_splits(N3 * M.vox(sp), cout * K)
        assert lib.iunet_dl_wgrad_slab_floats(nd, rate, N3, D, H, W, cin, cout) == splits * cout * K and splits == 2
        assert cout % 16 != 0 and K % 64 != 0          # Cout % 16 != 0 in the weight gradients
    h = M.DL_HALVED
    D, H, W = dhw(h['nd'], h['sp'])
    per = h['cout'] * 27 * h['cin']
    assert lib.iunet_dl_wgrad_slab_floats(h['nd'], h['rate'], h['N'], D, H, W, h['cin'], h['cout']) == 4 * per          # 8 splits halved to 4
    assert M.gg_wgrad_splits(h['N'] * M.vox(h['sp']), 1) == 8 and 8 * per > 8 << 20 >= 4 * per


def test_sf_geometry(lib):
    for nd in (2, 3):
        tsp = M.SF_T[nd]
        D, H, W = dhw(nd, tsp)
        cols = N3 * M.vox(tsp)
        assert lib.iunet_sf_stats_parts(N3, D, H, W) == M.sf_blocks(cols) == (15 if nd == 2 else 16) and cols % 64 in (28, 48)
        for cout in (24, 72):
            assert lib.iunet_sf_wgrad_slab_floats(N3, D, H, W, M.SF_K, cout) == 2 * cout * M.SF_K == M.gg_wgrad_splits(cols, cout * M.SF_K) * cout * M.SF_K
        for src, ssp in enumerate(M.SF_SRC[nd]):          # ratios 1/2, 1, 2 on every axis: dyadic weights
            assert all(2 * s == t * (4, 2, 1)[src] for s, t in zip(ssp, tsp))
    couts = {(dt, co) for _, dt, co in M.SF_GEMM}
    assert ('f32', 512) in couts and {('f16', 272), ('bf16', 272), ('f32', 272)} <= couts          # 17 row tiles; fp32 Cout 512: raised LDS
    assert (64 + 512) * 36 * 4 > 65536 >= (64 + 272) * 36 * 4


def test_refused_arguments_answer_without_a_gpu(lib):
    """The host functions refuse what the tables must not contain (a negative answer, no launch)."""
    assert lib.iunet_lk_stats_parts(2, 1, 3, 1, 13, 23, 40) < 0          # Cout no multiple of 16
    assert lib.iunet_lk_wgrad_slab_floats(2, 2, 3, 1, 13, 23, 16, 16) < 0          # kind 2 has no weight gradient
    assert lib.iunet_dl_num_taps(2, -1, 1, 13, 23) < 0


# ---------------------------------------------------------------------------------------------------------------- the exact regime
@pytest.mark.parametrize('kind,nd,cin,cout', M.LK_FWD)
def test_lk_fwd_is_exact(kind, nd, cin, cout):
    M.check_lk_fwd(kind, nd, N3, M.GRID[nd], cin, cout)


def test_lk_fwd_capped_is_exact():
    import torch
    c = M.CAP
    M.check_lk_fwd(c['kind'], c['nd'], c['N'], c['sp'], c['cin'], c['cout'], torch.float32)


def test_lk_wgrad_is_exact():
    for kind, nd, cin, cout in M.LK_WGRAD:
        M.check_lk_wgrad(kind, nd, N3, M.L2 if nd == 2 else M.L3, cin, cout)
    h = M.LK_HALVED
    M.check_lk_wgrad(h['kind'], h['nd'], h['N'], h['sp'], h['cin'], h['cout'])


@pytest.mark.parametrize('nd,rate,taps,cin,cout', M.DL_FWD)
def test_dl_fwd_is_exact(nd, rate, taps, cin, cout):
    M.check_dl_fwd(nd, N3, M.GRID[nd], cin, cout, rate)


def test_dl_aspp_and_wgrad_are_exact():
    for nd in (2, 3):
        M.check_aspp(nd, N3, M.GRID[nd])
    for nd, rate, cin, cout in M.DL_WGRAD:
        M.check_dl_wgrad(nd, N3, M.GRID[nd], cin, cout, rate, 8)
    h = M.DL_HALVED
    M.check_dl_wgrad(h['nd'], h['N'], h['sp'], h['cin'], h['cout'], h['rate'], 0, -1)


@pytest.mark.parametrize('act', [False, True])
@pytest.mark.parametrize('nd', [2, 3])
def test_sf_is_exact(nd, act):
    M.check_sf_B(nd, N3, act)
    for cout in sorted({co for n, _, co in M.SF_GEMM if n == nd}):
        M.check_sf_gemm(nd, N3, cout, act)
    for src in range(3):
        for C in (8, 24):
            M.check_sf_adjoint(nd, N3, C, src)
