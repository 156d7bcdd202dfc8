"""Symmetry ensemble of the 3-D net: mirror / transpose test-time augmentation.

A member of the ensemble is one of the 48 symmetries of the cube, sym = 8 * pi + f: pi indexes the permutations of (0, 1, 2) in
lexicographic order, bit a of f flips output axis a.  The block's bytes are transformed on the device (iunet_sym_block), go through the
engine's ordinary forward, and the probabilities are transformed back into the block's own orientation on their way into the running
sum, minimum and maximum (iunet_sym_accumulate).  The last member writes the mean -- sum * float32(1 / G), one multiply -- and, where
asked for, the spread: per voxel the largest disagreement max_k - min_k over the classes.  Members are taken in list order (fp32 sums
depend on it); the first member of every named set is the identity, so tta=[0] is the plain prediction.

predict.predict_blocks_3d / predict_volume_array / predict_slab take `tta=`: None, a set name, or a sequence of distinct codes."""
import itertools

import numpy as np
import torch

from . import _native as nv

PERMS = tuple(itertools.permutations((0, 1, 2)))
SETS = {'flips': tuple(range(8)),        # the mirrors
        'planar': tuple(range(16)),      # axis 0 stays in place: the slab's natural set (its planes stay planes)
        'full': tuple(range(48))}


def members(spec):
    """None -> None (no ensembling); a set name or a sequence of distinct codes 0 .. 47 -> the tuple of codes, in order."""
    if spec is None:
        return None
    if isinstance(spec, str):
        if spec not in SETS:
            raise ValueError(f'tta={spec!r}: the named sets are {", ".join(map(repr, SETS))}')
        return SETS[spec]
    try:
        raw = list(spec)
    except TypeError:
        raise ValueError(f'tta={spec!r}: None, a set name or a sequence of symmetry codes') from None
    out = []
    for v in raw:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f'tta: {v!r} is not a symmetry code (an int 0 .. 47)')
        if not 0 <= int(v) < 48:
            raise ValueError(f'tta: symmetry code {int(v)} outside 0 .. 47')
        out.append(int(v))
    if not out:
        raise ValueError('tta: an empty member list (None switches the ensemble off)')
    if len(set(out)) != len(out):
        raise ValueError(f'tta: duplicate members in {out}')
    return tuple(out)


def shape(n, sym):
    """The transformed block's shape."""
    perm = PERMS[int(sym) >> 3]
    return tuple(int(n[perm[a]]) for a in range(3))


def transform(block, sym, out):
    """uint8 [D, H, W] on the device -> `out` (uint8, shape(...) elements) in the member's orientation."""
    D, H, W = (int(v) for v in block.shape)
    nv.call('iunet_sym_block', nv.ptr(block), D, H, W, int(sym), nv.ptr(out), nv.stream())
    return out


class Ensemble:
    """The scratch of one block's ensemble, [D, H, W, C] in the block's own orientation: sum (and mn, mx, spread where the spread is
    wanted), owned across the members' calls; `mean` is the caller's."""

    def __init__(self, n, C, device, spread=False):
        self.n, self.C = tuple(int(v) for v in n), int(C)
        self.sum = torch.empty(self.n + (self.C,), dtype=torch.float32, device=device)
        self.mn = torch.empty_like(self.sum) if spread else None
        self.mx = torch.empty_like(self.sum) if spread else None
        self.spread = torch.empty(self.n, dtype=torch.float32, device=device) if spread else None

    def add(self, q, sym, index, count, mean):
        """Member `index` of `count`: q fp32 [m0, m1, m2, C], the forward's probabilities of the transformed block."""
        inv = float(np.float32(1) / np.float32(count))
        nv.call('iunet_sym_accumulate', nv.ptr(q), self.n[0], self.n[1], self.n[2], self.C, int(sym), int(index), int(count), inv,
                nv.ptr(self.sum), nv.ptr(self.mn), nv.ptr(self.mx), nv.ptr(mean), nv.ptr(self.spread), nv.stream())


def run(eng, block, syms, ens, mean, batch=1, blk=None, probs=None):
    """The member loop of one block: transform, forward (`batch` members of equal shape per forward), accumulate in member order.
    block: uint8 [D, H, W]; blk / probs: buffers for `batch` transformed blocks and their probabilities (allocated if None)."""
    n, C, G = tuple(int(v) for v in block.shape), ens.C, len(syms)
    vox = n[0] * n[1] * n[2]
    B = max(1, int(batch))
    if blk is None:
        blk = torch.empty((B, vox), dtype=torch.uint8, device=block.device)
    if probs is None:
        probs = torch.empty((B, vox * C), dtype=torch.float32, device=block.device)
    blk, probs = blk.reshape(blk.shape[0], -1), probs.reshape(probs.shape[0], -1)
    k = 0
    while k < G:
        m = shape(n, syms[k])
        nb = 1
        while nb < B and k + nb < G and shape(n, syms[k + nb]) == m:       # one forward takes members of one shape
            nb += 1
        for j in range(nb):
            transform(block, syms[k + j], blk[j])
        eng.infer(blk, (vox, vox, m[1] * m[2], m[2], 1), nb, m[0], m[1], m[2], probs=probs,
                  out_strides=(vox * C, 1, m[1] * m[2] * C, m[2] * C, C))
        for j in range(nb):
            ens.add(probs[j], syms[k + j], k + j, G, mean)
        k += nb
    return mean
