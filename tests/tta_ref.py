"""The definition of the 3-D net's symmetry ensemble: what iunet_sym_block and iunet_sym_accumulate compute,
restated in plain numpy.  Nothing here imports the package.

A symmetry of the cube is sym = 8 * pi + f, 0 <= sym < 48: pi indexes the permutations of (0, 1, 2) in lexicographic order, bit a of f
flips OUTPUT axis a.  forward: B = np.flip(np.transpose(A, perm), flipped axes), shape m[a] = n[perm[a]]; B[t] = A[s] with s[perm[a]] =
m[a] - 1 - t[a] where bit a is set, t[a] otherwise.  inverse: the same pairing the other way, P[s] = Q[t] -- flip the same axes back,
then transpose by the inverse permutation.  Trailing axes (channels) are never touched.

The ensemble over members g_0 .. g_{G-1} in list order: sum_0 = P_0, sum_k = sum_{k-1} + P_k (each fp32 add rounded on its own),
mean = sum_{G-1} * r with r = float32(1) / float32(G) (one fp32 multiply), spread[s] = max over c of (max_k P_k[s, c] - min_k P_k[s, c])
in fp32."""
import itertools

import numpy as np

PERMS = tuple(itertools.permutations((0, 1, 2)))          # lexicographic: (0,1,2), (0,2,1), (1,0,2), (1,2,0), (2,0,1), (2,1,0)
SETS = {'flips': tuple(range(8)), 'planar': tuple(range(16)), 'full': tuple(range(48))}


def decode(sym):
    """(perm, flipped output axes)."""
    sym = int(sym)
    assert 0 <= sym < 48
    return PERMS[sym >> 3], tuple(a for a in range(3) if (sym & 7) >> a & 1)


def shape(n, sym):
    perm, _ = decode(sym)
    return tuple(int(n[perm[a]]) for a in range(3))


def forward(A, sym):
    A = np.asarray(A)
    perm, flips = decode(sym)
    B = np.transpose(A, perm + tuple(range(3, A.ndim)))
    return np.ascontiguousarray(np.flip(B, flips)) if flips else np.ascontiguousarray(B)


def inverse(Q, sym):
    Q = np.asarray(Q)
    perm, flips = decode(sym)
    P = np.flip(Q, flips) if flips else Q
    inv = tuple(int(i) for i in np.argsort(perm))
    return np.ascontiguousarray(np.transpose(P, inv + tuple(range(3, Q.ndim))))


def ensemble_steps(qs, syms):
    """The running (sum, mn, mx) after every member: qs[k] fp32 [m0, m1, m2, C] is member syms[k]'s output."""
    out, s, lo, hi = [], None, None, None
    for k, (q, sym) in enumerate(zip(qs, syms)):
        P = inverse(np.asarray(q, dtype=np.float32), sym)
        if k == 0:
            s, lo, hi = P.copy(), P.copy(), P.copy()
        else:
            s = (s + P).astype(np.float32)
            lo, hi = np.minimum(lo, P), np.maximum(hi, P)
        out.append((s, lo, hi))
    return out


def ensemble(qs, syms):
    """(mean fp32 [D, H, W, C], spread fp32 [D, H, W])."""
    s, lo, hi = ensemble_steps(qs, syms)[-1]
    r = np.float32(1) / np.float32(len(syms))
    return (s * r).astype(np.float32), (hi - lo).astype(np.float32).max(axis=-1)
