"""The nearest-seed feature transform at volume scale (DESIGN.md sections 4.1 and 26): one case, 1030 x 1024 x 1024, where d2 and idx each
pass 2^32 bytes (4.32e9).  It holds about 22.7 GB of device memory: the source 1.08 GB, d2 and idx 4.32 GB each, the workspace 12.96 GB (the
columns' stacks 8.64, the second idx map 4.32), besides the slabs the input is generated in.  An allocation that fails is a failure."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import instances_ref as ir
from tests.test_morphology_cpu import lattice_axis


def test_a_volume_whose_feature_maps_pass_2_32_bytes():
    """The seeds are the closed lattice z % 7 == y % 5 == x % 9 == 0 (with the last plane of each axis), which bounds every squared distance
    by 3^2 + 2^2 + 4^2 = 29 (tests/test_morphology_cpu.py), and random seeds at p = 0.01.  So the nearest seeds of a 48^3 crop lie in the crop
    extended by 6 voxels, and the tie rule, lexicographic in (z, y, x), survives the translation: three crops against the definition on
    the host, its indices translated into volume coordinates -- at the origin, across linear index 2^30 where both maps cross byte 2^32,
    and at the far corner."""
    from interactive_unet import _native as nv
    shape = Z, Y, X = (1030, 1024, 1024)
    assert 4 * Z * Y * X > 2 ** 32 and (1024 * Y + 0) * X == 2 ** 30
    g = torch.Generator(device='cuda').manual_seed(26)
    src = torch.empty(shape, dtype=torch.uint8, device='cuda')
    on = lambda lo, hi, n, step: torch.tensor(lattice_axis(n, step)[lo:hi], device='cuda')
    yx = on(0, Y, Y, 5)[:, None] & on(0, X, X, 9)[None, :]
    for z0 in range(0, Z, 64):
        z1 = min(Z, z0 + 64)
        lattice = on(z0, z1, Z, 7)[:, None, None] & yx[None]
        src[z0:z1] = (lattice | (torch.rand((z1 - z0, Y, X), device='cuda', generator=g) < 0.01)).to(torch.uint8)
    del lattice
    d2 = torch.full(shape, -7, dtype=torch.int32, device='cuda')
    idx = torch.full(shape, -9, dtype=torch.int32, device='cuda')
    ws_bytes = nv.lib().iunet_edt_feature_ws_bytes(Z, Y, X)
    assert ws_bytes == 12 * Z * Y * X
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device='cuda')
    nv.call('iunet_edt_feature', nv.ptr(src), Z, Y, X, 1, 1, 0, nv.ptr(d2), nv.ptr(idx), None, nv.ptr(ws), ws_bytes, nv.stream())
    del ws
    top = int(d2.max())
    assert 0 < top <= 29, top
    assert int(idx.min()) >= 0 and int(idx.max()) == Z * Y * X - 1                # the far corner is a seed, and its own nearest
    for lo in ((0, 0, 0), (982, 0, 0), (982, 976, 976)):
        hi = tuple(a + 48 for a in lo)
        elo = tuple(max(0, a - 6) for a in lo)
        ehi = tuple(min(n, b + 6) for n, b in zip(shape, hi))
        ext = src[elo[0]:ehi[0], elo[1]:ehi[1], elo[2]:ehi[2]].cpu().numpy()
        w_d2, w_idx = ir.feature(ext, 1, False)
        inner = tuple(slice(a - e, b - e) for a, b, e in zip(lo, hi, elo))
        w_d2, w_idx = w_d2[inner], w_idx[inner]
        assert w_d2.shape == (48, 48, 48) and w_idx.min() >= 0
        z, y, x = np.unravel_index(w_idx.astype(np.int64), ext.shape)         # the seed in the extended crop -> in the volume
        w_idx = ((z + elo[0]).astype(np.int64) * Y + (y + elo[1])) * X + (x + elo[2])
        assert np.array_equal(d2[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].cpu().numpy(), w_d2), lo
        assert np.array_equal(idx[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].cpu().numpy().astype(np.int64), w_idx), lo
    assert lo[0] <= 1024 < hi[0]                                               # the last two crops hold voxels on both sides of byte 2^32
