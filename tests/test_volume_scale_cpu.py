"""tests/volume_scale_ref.py without a GPU: the shapes of tests/test_gpu_volume_scale.py lie on the far side of the
thresholds read out of csrc/components.hip and past 2^31 elements / 2^32 bytes while inside every entry point's limits; the tiled
closed form is components_ref.label of the concatenated volume; under the dyadic geometries a definition evaluated on a crop with the
shifted origin is the definition on the whole volume."""
import os
import re

import numpy as np
import pytest
import torch

from tests import components_ref as cr
from tests import patch_ref
from tests import propose_ref as pr
from tests import slab_ref as sr
from tests import volume_scale_ref as vs
from tests.volume_inputs import random_pred

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'interactive-unet_amd', 'csrc')


def _constants():
    """The launch-policy constants of csrc/components.hip, by name."""
    with open(os.path.join(CSRC, 'components.hip')) as f:
        src = f.read()

    def value(name):
        m = re.search(r'^constexpr[^;\n]*\b' + name + r'\s*=\s*([^,;]+)[,;]', src, re.M)
        assert m, name
        text = re.sub(r'(?<=[0-9a-fA-F])(ll|u)\b', '', m.group(1).strip())
        return int(eval(text, {'__builtins__': {}}, {}))                 # an integer literal or a shift of literals
    return {n: value(n) for n in ('CC_TZ', 'CC_TY', 'CC_TX', 'CC_CHUNK', 'CC_SCAN_THREADS', 'CC_TABLE_GRID', 'CC_MAX_TILE_GRID', 'CC_MAX_VOX')}


def _chunks(shape, k):
    return -(-int(np.prod(shape[:3], dtype=np.int64)) // k['CC_CHUNK'])


def _tiles(shape, k):
    return -(-shape[0] // k['CC_TZ']) * -(-shape[1] // k['CC_TY']) * -(-shape[2] // k['CC_TX'])


def test_part_a_shapes_cross_the_thresholds_of_components_hip():
    k = _constants()
    assert (k['CC_TZ'], k['CC_TY'], k['CC_TX']) == (4, 16, 64)           # the values the shapes were chosen for: a change re-opens the choice
    # A.1: scan_kernel per >= 3, table_kernel per >= 2, ragged against the tile on every axis
    nb = _chunks(vs.A1_SHAPE, k)
    assert -(-nb // k['CC_SCAN_THREADS']) >= 3 and -(-nb // k['CC_TABLE_GRID']) >= 2
    assert all(n % t for n, t in zip(vs.A1_SHAPE, (k['CC_TZ'], k['CC_TY'], k['CC_TX'])))
    # the largest volume of tests/test_gpu_components.py stays below both (the reason this file exists)
    assert _chunks((37, 41, 150), k) <= k['CC_SCAN_THREADS'] and _tiles((37, 41, 150), k) < k['CC_MAX_TILE_GRID']
    # A.2: more tiles than the tile grid, so tile_kernel and seam_kernel stride; the thin volume has two tiles across x
    for shape in (vs.A2_COLUMN, vs.A2_THIN):
        assert k['CC_MAX_TILE_GRID'] < _tiles(shape, k) < 2 * k['CC_MAX_TILE_GRID']      # some workgroups take two tiles, some one
        assert np.prod(shape, dtype=np.int64) <= k['CC_MAX_VOX']
    assert -(-vs.A2_THIN[2] // k['CC_TX']) == 2
    # A.3: under the cap in voxels, past 2^32 in bytes
    n3 = int(np.prod(vs.A3_SHAPE[:3], dtype=np.int64))
    assert n3 <= k['CC_MAX_VOX'] and n3 * vs.A3_SHAPE[3] > 2 ** 32 and 2 <= vs.A3_SHAPE[3] <= 16
    # A.4: within 2^17 of the cap, which is INT_MAX; table per at its largest
    n4 = int(np.prod(vs.A4_SHAPE, dtype=np.int64))
    assert k['CC_MAX_VOX'] == 2 ** 31 - 1 and 0 <= k['CC_MAX_VOX'] - n4 < 2 ** 17
    assert -(-_chunks(vs.A4_SHAPE, k) // k['CC_TABLE_GRID']) == 256
    # the copies tile the shapes exactly and sit differently in the tiles
    for shape, bz in ((vs.A2_THIN, vs.A2_THIN_BZ), (vs.A3_SHAPE, vs.A3_BZ), (vs.A4_SHAPE, vs.A4_BZ)):
        assert vs.copies(shape, bz) * (bz + 1) == shape[0] and (bz + 1) % k['CC_TZ'] != 0


def test_part_b_arrays_pass_2_31_elements_and_2_32_bytes_inside_the_limits():
    v8 = int(np.prod(vs.V8_SHAPE, dtype=np.int64))
    assert v8 > 2 ** 32 and all(n % 16 for n in vs.V8_SHAPE)
    v8c = int(np.prod(vs.V8C_SHAPE, dtype=np.int64))
    assert v8c > 2 ** 32 and v8c // vs.V8C_SHAPE[3] < 2 ** 31
    vf = int(np.prod(vs.VF_SHAPE, dtype=np.int64))
    assert vf > 2 ** 31 and 4 * vf > 2 ** 33 and vs.VF_SHAPE[:3] == vs.V8C_SHAPE[:3]
    # the limits the entry points state (include/iunet.h): volumes below 2^42 voxels, every extent an int, 2 .. 16 classes, zoom
    # destinations of at most 65535 samples on the two outer axes
    for shape in (vs.V8_SHAPE, vs.V8C_SHAPE, vs.VF_SHAPE):
        assert int(np.prod(shape[:3], dtype=np.int64)) < 2 ** 42 and max(shape) < 2 ** 31
    assert 2 <= vs.V8C_SHAPE[3] <= 16 and vs.V8C_SHAPE[0] // 2 <= 65535 and vs.V8C_SHAPE[1] // 2 <= 65535
    # the far-corner crop: every byte offset in it is past 2^31, and byte 2^32 lies between its first and its last plane
    for shape, C in ((vs.V8_SHAPE, 1), (vs.V8C_SHAPE, vs.V8C_SHAPE[3])):
        off = vs.far_offset(shape)
        first = ((int(off[0]) * shape[1] + int(off[1])) * shape[2] + int(off[2])) * C
        plane = shape[1] * shape[2] * C
        assert 2 ** 31 < first < 2 ** 32 and int(off[0]) < 2 ** 32 // plane < shape[0] - 8 and all(o > 0 and o % 2 == 0 for o in off)


def _blocks():
    rng = np.random.default_rng(5)
    shape = (5, 19, 70)
    return {'binary': ((rng.random(shape) < 0.5).astype(np.uint8), 2),
            'three classes': (rng.integers(0, 3, shape).astype(np.uint8), 3),
            'pred': (random_pred(shape, 3, 6), 0)}


@pytest.mark.parametrize('conn', (6, 18, 26))
@pytest.mark.parametrize('bg', (0, None))
@pytest.mark.parametrize('kind', ('binary', 'three classes', 'pred'))
def test_the_tiled_closed_form_is_the_definition_on_the_concatenated_volume(kind, bg, conn):
    block, free = _blocks()[kind]
    n = 7
    sep = 0 if block.ndim == 4 else (bg if bg is not None else free)
    t = vs.Tiled(block, conn, bg, sep)
    big = t.volume(n).numpy()
    assert big.shape[0] == n * 6 and np.array_equal(big[6:11], block) and (big[5] == sep).all()
    labels, K, cls = cr.label(big, conn, bg)
    assert K == t.count(n) and K >= n
    assert np.array_equal(t.labels(0, n).numpy(), labels) and np.array_equal(t.cls(0, n).numpy(), cls)
    assert np.array_equal(torch.cat([t.labels(0, 3), t.labels(3, n)]).numpy(), labels)        # built in chunks
    want = cr.table(labels, cls, K)
    for got, w in zip(t.table(n), want):
        assert got.dtype == torch.from_numpy(w).dtype and np.array_equal(got.numpy(), w)
    for got, w in zip(vs.table_fast(labels, cls, K), want):
        assert got.dtype == w.dtype and np.array_equal(got, w)


def test_the_geometries_are_dyadic():
    for shape in (vs.V8_SHAPE, vs.V8C_SHAPE):
        for geoms in (vs.slab_geometries(shape), vs.origin_geometries()):
            for a, b, n, o in geoms.values():
                assert vs.is_dyadic([a, b, n], vs.D8, 2.0) and vs.is_dyadic(o, vs.D8, 4096.0)
                assert abs(np.dot(np.cross(a, b), n)) > 0.1                               # three independent directions
    a, b, n = vs.SLAB_VECTORS
    assert all(np.count_nonzero(v) == 3 for v in (a, b, n))                               # oblique
    for m in vs.PATCH_POSES.values():
        assert vs.is_dyadic(m, vs.D4, 2.0) and abs(np.linalg.det(m)) > 0.1
    assert vs.is_dyadic(vs.patch_centre(vs.V8_SHAPE), vs.D4, 4096.0)


# a small whole volume and its far-corner crop: the same relation as the large arrays have to their crops
SMALL, SMALL_CROP = (72, 80, 90), 68


def _small_offset():
    return np.array([n - SMALL_CROP for n in SMALL], dtype=np.int64)


def _rescaled(geoms, shape):
    """The geometries of `shape`, moved to the far corner of SMALL by an integer shift."""
    shift = np.array(shape[:3]) - np.array(SMALL)
    return {name: vs.shifted(g, shift) for name, g in geoms.items()}


@pytest.mark.parametrize('order', (0, 1))
def test_slab_gather_on_a_crop_is_slab_gather_on_the_volume(order):
    vol = np.random.default_rng(1).integers(0, 256, SMALL, dtype=np.uint8)
    off = _small_offset()
    crop = vol[off[0]:, off[1]:, off[2]:]
    for name, geom in _rescaled(vs.slab_geometries(vs.V8_SHAPE), vs.V8_SHAPE).items():
        T, sw = vs.SLAB
        c = sr.coords(geom, T, sw)
        assert all(c[x].min() >= off[x] + 1 for x in range(3)) and any(c[x].max() > SMALL[x] for x in range(3)), name
        want = sr.gather(vol, geom, T, sw, order)
        assert np.array_equal(sr.coords(vs.shifted(geom, off), T, sw), c - off[:, None, None, None])      # exact, not close
        assert np.array_equal(sr.gather(crop, vs.shifted(geom, off), T, sw, order), want), name
        assert want.any() and (want == 0).any()


def test_slab_paste_on_a_crop_is_slab_paste_on_the_volume():
    C, (T, sw) = 3, vs.SLAB
    rng = np.random.default_rng(2)
    dest = rng.integers(0, 256, SMALL + (C,), dtype=np.uint8)
    probs = rng.random((T, sw, sw, C), dtype=np.float32)
    off = _small_offset()
    lo, length = off + 6, np.array([SMALL_CROP - 6] * 3)
    for name, geom in _rescaled(vs.slab_geometries(vs.V8C_SHAPE), vs.V8C_SHAPE).items():
        want = sr.paste(dest, probs, geom, 1, T, 1, lo=lo, length=length)
        got = sr.paste(dest[off[0]:, off[1]:, off[2]:], probs, vs.shifted(geom, off), 1, T, 1, lo=lo - off, length=length)
        assert np.array_equal(got, want[off[0]:, off[1]:, off[2]:]), name
        assert (want != dest).any()


def test_plane_scores_on_a_crop_are_plane_scores_on_the_volume():
    u = np.random.default_rng(3).integers(0, 256, SMALL, dtype=np.uint8)
    off = _small_offset()
    sw = vs.SLAB[1]
    for name, (a, b, _, o) in _rescaled(vs.slab_geometries(vs.V8_SHAPE), vs.V8_SHAPE).items():
        c = pr.plane_coords((a, b, o), sw)
        assert all(c[x].min() >= off[x] for x in range(3)), name
        want = pr.plane_score(u, (a, b, o), sw)
        assert pr.plane_score(u[off[0]:, off[1]:, off[2]:], (a, b, o - off), sw) == want and 0 < want[1] < sw * sw, name
    for name, (a, b, _, o) in vs.origin_geometries().items():                              # the first corner: the crop ends inside the volume
        c = pr.plane_coords((a, b, o), sw)
        assert all(c[x].max() <= SMALL_CROP - 1 for x in range(3)), name
        want = pr.plane_score(u, (a, b, o), sw)
        assert pr.plane_score(u[:SMALL_CROP, :SMALL_CROP, :SMALL_CROP], (a, b, o), sw) == want and 0 < want[1] < sw * sw, name


@pytest.mark.parametrize('order', (0, 1))
def test_patches_on_a_crop_are_patches_on_the_volume(order):
    image, mask, weight = patch_ref.make_volume(np.random.default_rng(4), SMALL, dark=True)
    weight = weight[..., 0]
    off = _small_offset()
    assert (off % 2 == 0).all()
    box = (slice(off[0], None), slice(off[1], None), slice(off[2], None))
    centre = vs.patch_centre(vs.V8_SHAPE) - (np.array(vs.V8_SHAPE) - np.array(SMALL))
    patch = vs.PATCH
    for name, m in vs.PATCH_POSES.items():
        p = patch_ref.coordinates(m.reshape(-1), centre, patch)
        assert all(p[x].min() >= off[x] + 1 for x in range(3)) and any(p[x].max() > SMALL[x] for x in range(3)), name
        assert np.array_equal(patch_ref.coordinates(m.reshape(-1), centre - off, patch), p - off[:, None, None, None].astype(np.float32))
        want = patch_ref.patch(image, mask, weight, m.reshape(-1), centre, patch, 2, order)
        got = patch_ref.patch(image[box], mask[box], weight[box], m.reshape(-1), centre - off, patch, 2, order)
        for g, w in zip(got, want):
            assert g.dtype == np.float16 and np.array_equal(g.view(np.uint16), w.view(np.uint16)), name
    # the offset has to be even: the nearest voxel is rint's, ties to even, and the scaled pose has samples at half-integers
    odd = off + 1
    box = (slice(odd[0], None), slice(odd[1], None), slice(odd[2], None))
    m = vs.PATCH_POSES['dyadic, scaled'].reshape(-1)
    shifted = patch_ref.patch(image[box], mask[box], weight[box], m, centre - odd, patch, 2, order)
    assert not np.array_equal(shifted[2], patch_ref.patch(image, mask, weight, m, centre, patch, 2, order)[2])
