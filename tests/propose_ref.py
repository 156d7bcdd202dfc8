"""The definition of the slice proposal's numbers: what iunet_uncertainty_volume and iunet_plane_scores
compute, and what interactive_unet/propose.py builds on them, restated in plain numpy with loops where that is clearer.  Nothing
here imports the package.

Uncertainty byte of a voxel with predicted bytes q[0 .. C-1], 2 <= C <= 16: b1 the largest byte, b2 the second largest counted with
multiplicity (two channels tied at the top: b2 = b1); u = 255 - (b1 - b2) if b1 > 0 else 0 (an all-zero voxel was never predicted);
u = 0 where any weight byte of the voxel is > 0 (annotated) and where image channel 0 is 0 (the loader's dark rule).
Brick sums at brick size g: bricks[bz, by, bx] = the sum of u over the voxels of the brick that lie inside the volume, uint32,
ceil(dim / g) entries per axis.
Plane score of (a, b, o) at width sw, start = -floor(sw / 2): sample (i, j) at c = (a r_i + b r_j) + o per axis, r_i = start + i,
r_j = start + j, every product and sum rounded on its own (numpy evaluates one ufunc at a time); inside iff 0 <= c <= dim - 1 on all
three axes, then it reads voxel floor(c + 0.5).  score = the sum of u over the inside samples, inside = their count, both int64."""
import numpy as np

BRICKS = (4, 8, 16, 32)


def default_start(sw):
    return int(-np.floor(sw / 2))


def voxel_uncertainty(q, weight=(), dark=False):
    """One voxel: q the predicted bytes, weight its weight bytes (none: not given), dark: image channel 0 is 0."""
    s = sorted(int(t) for t in q)
    b1, b2 = s[-1], s[-2]
    if b1 == 0 or dark or any(int(w) > 0 for w in weight):
        return 0
    return 255 - (b1 - b2)


def uncertainty(pred, weight=None, image=None):
    """uint8 [Z, Y, X] from pred uint8 [Z, Y, X, C], weight None / uint8 [Z, Y, X(, wch)], image None / uint8 [Z, Y, X(, ich)]."""
    pred = np.asarray(pred)
    s = np.sort(pred.astype(np.int64), axis=-1)
    b1, b2 = s[..., -1], s[..., -2]
    u = np.where(b1 > 0, 255 - (b1 - b2), 0)
    if weight is not None:
        w = np.asarray(weight).reshape(pred.shape[:3] + (-1,))
        u[(w > 0).any(axis=-1)] = 0
    if image is not None:
        im = np.asarray(image).reshape(pred.shape[:3] + (-1,))
        u[im[..., 0] == 0] = 0
    return u.astype(np.uint8)


def brick_sums(u, g):
    """uint32 [ceil(Z / g), ceil(Y / g), ceil(X / g)]: brick by brick, edge bricks ragged."""
    u = np.asarray(u)
    nb = [-(-n // g) for n in u.shape]
    out = np.zeros(nb, dtype=np.uint32)
    for bz in range(nb[0]):
        for by in range(nb[1]):
            for bx in range(nb[2]):
                out[bz, by, bx] = u[bz * g:(bz + 1) * g, by * g:(by + 1) * g, bx * g:(bx + 1) * g].sum(dtype=np.uint64)
    return out


def plane_coords(plane, sw, start=None):
    """float64 [3, sw, sw] of the plane (a, b, o)."""
    a, b, o = (np.asarray(t, dtype=np.float64) for t in plane)
    start = default_start(sw) if start is None else start
    ri = (start + np.arange(sw)).astype(np.float64)[None, :, None]
    rj = (start + np.arange(sw)).astype(np.float64)[None, None, :]
    t1 = np.multiply(a[:, None, None], ri)
    t2 = np.multiply(b[:, None, None], rj)
    s = np.add(t1, t2)
    return np.add(s, o[:, None, None])


def plane_score(u, plane, sw, start=None):
    """(score, inside) as Python ints."""
    u = np.asarray(u)
    c = plane_coords(plane, sw, start)
    hi = (np.array(u.shape, dtype=np.float64) - 1.0)[:, None, None]
    inside = np.all((c >= 0.0) & (c <= hi), axis=0)
    idx = np.floor(c + 0.5).astype(np.int64)[:, inside]
    return int(u[idx[0], idx[1], idx[2]].astype(np.int64).sum()), int(inside.sum())


def score_planes(u, planes, sw, start=None):
    """int64 [P, 2]."""
    return np.array([plane_score(u, pl, sw, start) for pl in planes], dtype=np.int64).reshape(-1, 2)


def candidate_origins(bricks, g, shape, count):
    """float64 [n <= count, 3]: the bricks of largest positive sum (sum descending, flat index ascending), each as the centre of its
    in-volume part, b g + (min((b + 1) g, dim) - b g - 1) / 2."""
    bricks = np.asarray(bricks)
    ranked = sorted(range(bricks.size), key=lambda k: (-int(bricks.flat[k]), k))[:count]
    out = []
    for k in ranked:
        if int(bricks.flat[k]) == 0:
            continue
        b = np.unravel_index(k, bricks.shape)
        out.append([b[x] * g + (min((b[x] + 1) * g, int(shape[x])) - b[x] * g - 1) / 2 for x in range(3)])
    return np.array(out, dtype=np.float64).reshape(-1, 3)


def rank(scores):
    """Plane indices by (score descending, index ascending)."""
    return sorted(range(len(scores)), key=lambda p: (-int(scores[p][0]), p))
