"""Host-side plan of the native UPerNet forward (Xiao et al. 2018: a pyramid-pooling module on the encoder's coarsest output, an FPN
top-down path and a fused multi-level head, on this project's encoder): folded eval-mode BatchNorm, 16-bit (UPerNetEngine, on
engine.EncoderEngine's encoder) and fp32 (UPerNetEngineF32, on engine_f32.EncoderEngineF32's).  Both keep the `load_eval` / `infer(...)`
interface predict.py drives.

Graph (B = L - 1 the bottom level, T = level 2's grid, C = decoder_channels, Cq = ch[B] / 4; R = linear resampling, align_corners=False).
  A_s = adaptive average pool of X^B to s bins per axis, s in (1, 2, 3, 6); Q_1 = relu(conv1x1(A_1) + bias), Q_s = relu(bn(conv1x1(A_s)));
  U = [X^B, R(Q_1), R(Q_2), R(Q_3), R(Q_6)] on G_B (2 ch[B] channels); P^B = relu(bn(conv3^d(U)));
  P^l = R(P^{l+1}) + relu(bn(conv1x1(X^l))) for l = B-1 .. 2;  V = [R(P^B), .., R(P^3), P^2] on T;  F = relu(bn(conv3^d(V)));
  the 1x1 head gives the coarse logits on T, upsampled x4 (align_corners=True) into iunet_head_fwd's output contract.
Every conv is one of deeplab.hip's gathered GEMMs with its BatchNorm folded; csrc/upernet.hip pools X^B (one launch) and resamples into the
channel slots of U and V, adding the lateral in the same pass (the lateral conv writes P^l's buffer, the resize adds R(P^{l+1}) in place;
P^2 lives in V's last slot).  The workspace table is `_UPerNet._bufs`: U on G_B, P^l for l = B .. 3, V and F on T -- no C-channel tensor
finer than T exists.
"""
import torch

from . import _native as nv
from .engine import BN_EPS, CoarseLogits, EncoderEngine, _vox
from .engine_f32 import EncoderEngineF32
from .topology import BN_KEYS

T_LEVEL = 2                  # the target grid T is level 2's grid (stride 4)
POOL_SIZES = (1, 2, 3, 6)    # bins per spatial axis of the pyramid pooling branches


def pool_dims(dim, s):
    """The grid of A_s / Q_s."""
    return (s if dim == 3 else 1, s, s)


def branch(s):
    return f'psp.b{s}'


def laterals(levels):
    """The levels with a lateral conv, in top-down (parameter) order: B-1 .. 2."""
    return list(range(levels - 2, T_LEVEL - 1, -1))


def conv_table(dim, levels, ch, C):
    """(prefix, kernel size, input channels, output channels) of every decoder conv, in parameter order."""
    Cb = ch[-1]
    return [(branch(s), 1, Cb, Cb // 4) for s in POOL_SIZES] + [('psp.out', 3, 2 * Cb, C)] + \
           [(f'lat{l}', 1, ch[l], C) for l in laterals(levels)] + [('fuse', 3, (levels - 2) * C, C)]


def check_setup(name, C, levels):
    if C % 32 or not (32 <= C <= 512) or not (4 <= levels <= 6):
        raise NotImplementedError(f'{name}: decoder_channels {C} (a multiple of 32 in 32 .. 512), {levels} levels (4 .. 6)')


class _UPerNet(CoarseLogits):
    """What the two UPerNet engines share: operator packing, workspace sizes, the decoder's sequence."""
    coarse_level = T_LEVEL

    def _setup(self, decoder_channels):
        self.C = int(decoder_channels)
        check_setup('UPerNet engine', self.C, self.levels)
        self.kvol = 3 ** self.dim

    def _bufs(self, dims, N):
        """(element counts of the activation workspace, of the fp32 workspace): x{l} / a{l} / pin{l} of the encoder; pool{s} (A_s) and
        q{s} (Q_s) on s^d; U on G_B; p{l} (P^l) for l = B .. 3; V (its last slot is P^2) and feat (F) on T; fp32: lc (coarse logits on T)."""
        act, ch, C, L = {}, self.ch, self.C, self.levels
        for l in range(L):
            v = _vox(dims[l])
            act[f'x{l}'] = N * ch[l] * v
            act[f'a{l}'] = N * ch[l] * v
            if l > 0:
                act[f'pin{l}'] = N * ch[l - 1] * v
        for s in POOL_SIZES:
            act[f'pool{s}'] = N * ch[-1] * s ** self.dim
            act[f'q{s}'] = N * (ch[-1] // 4) * s ** self.dim
        act['U'] = N * 2 * ch[-1] * _vox(dims[-1])
        for l in range(L - 1, T_LEVEL, -1):
            act[f'p{l}'] = N * C * _vox(dims[l])
        vt = _vox(dims[T_LEVEL])
        act['V'] = N * (L - 2) * C * vt
        act['feat'] = N * C * vt
        return act, {'lc': N * self.ncls * vt}

    def _pack_decoder(self, src, dtype_code):
        """Fold every decoder BatchNorm into its conv: {prefix: (operator, bias, row length, kept sources)}; psp.b1 has no norm, its bias is
        the conv's own."""
        P = {}
        for prefix, ksz, cin, cout in conv_table(self.dim, self.levels, self.ch, self.C):
            kw = (1 if ksz == 1 else self.kvol) * cin
            w = src(f'{prefix}.conv.weight')
            dst = torch.empty(cout * kw, dtype=self._pack_dtype, device=self.device)
            if prefix == branch(1):
                g, bias = [], src(f'{prefix}.conv.bias')
                fold = (None, None, None, None, 0.0, nv.ptr(dst), None)
            else:
                g, bias = [src(f'{prefix}.bn.{k}') for k in BN_KEYS], torch.empty(cout, dtype=torch.float32, device=self.device)
                fold = (nv.ptr(g[0]), nv.ptr(g[1]), nv.ptr(g[2]), nv.ptr(g[3]), BN_EPS, nv.ptr(dst), nv.ptr(bias))
            nv.call('iunet_dl_pack', dtype_code, self.dim, 0, ksz, nv.ptr(w), *fold, cout, cin, cin, 0, 0, kw, nv.stream())
            P[prefix] = (dst, bias, kw, g + [w])               # (the sources stay alive until the pack has run)
        P['head'] = (src('head.weight').reshape(self.ncls, self.C).contiguous(), src('head.bias'))
        return P

    def _resize(self, src, src_ss, ds, dst, dst_ss, dt, c, N, base=None, base_ss=0):
        nv.call('iunet_pn_resize', self.dt, self.dim, src, src_ss, ds[0], ds[1], ds[2], None, None, base, base_ss, None, None, dst, dst_ss,
                dt[0], dt[1], dt[2], c, N, nv.stream())

    def _decode(self, ws, N):
        """Pyramid pooling on X^B into U, psp.out, the top-down path, the slots of V, fuse into ws['feat']."""
        dims, C, ch, L, P = ws['dims'], self.C, self.ch, self.levels, self._P
        B, Cb, Cq = L - 1, ch[-1], ch[-1] // 4
        db, vb, dt, vt = dims[-1], _vox(dims[-1]), dims[T_LEVEL], _vox(dims[T_LEVEL])
        X, nV = ws[f'x{B}'], (L - 2) * C
        nb = [s ** self.dim for s in POOL_SIZES]
        nv.call('iunet_pn_pool', self.dt, self.dim, P(X), Cb * vb, db[0], db[1], db[2], nv.ptr_array([ws[f'pool{s}'] for s in POOL_SIZES]),
                nv.ll_array([Cb * n for n in nb]), Cb, N, nv.stream())
        self._resize(P(X), Cb * vb, db, P(ws['U']), 2 * Cb * vb, db, Cb, N)
        for k, s in enumerate(POOL_SIZES):
            d = pool_dims(self.dim, s)
            self._conv(branch(s), P(ws[f'pool{s}']), Cb * nb[k], P(ws[f'q{s}']), Cq * nb[k], 0, N, d, Cb, Cq)
            self._resize(P(ws[f'q{s}']), Cq * nb[k], d, P(ws['U'], (Cb + k * Cq) * vb), 2 * Cb * vb, db, Cq, N)
        self._conv('psp.out', P(ws['U']), 2 * Cb * vb, P(ws[f'p{B}']), C * vb, 1, N, db, 2 * Cb, C)
        slot = lambda l: (P(ws['V'], (B - l) * C * vt), nV * vt)          # P^l's slot of V (deepest first)
        pl = lambda l: slot(l) if l == T_LEVEL else (P(ws[f'p{l}']), C * _vox(dims[l]))
        for l in laterals(L):
            (yp, y_ss), (up, u_ss) = pl(l), pl(l + 1)
            self._conv(f'lat{l}', P(ws[f'x{l}']), ch[l] * _vox(dims[l]), yp, y_ss, 0, N, dims[l], ch[l], C)
            self._resize(up, u_ss, dims[l + 1], yp, y_ss, dims[l], C, N, base=yp, base_ss=y_ss)
        for l in range(B, T_LEVEL, -1):
            self._resize(P(ws[f'p{l}']), C * _vox(dims[l]), dims[l], *slot(l), dt, C, N)
        self._conv('fuse', P(ws['V']), nV * vt, P(ws['feat']), C * vt, 1, N, dt, nV, C)


class UPerNetEngine(_UPerNet, EncoderEngine):
    """The 16-bit (fp16 / bf16) UPerNet forward with folded BatchNorm."""

    def __init__(self, dim=2, levels=4, base=32, cin=1, ncls=2, act_dtype=torch.float16, device='cuda', decoder_channels=256):
        EncoderEngine.__init__(self, dim, levels, base, cin, ncls, act_dtype, device)
        self._setup(decoder_channels)

    def _conv(self, prefix, xp, x_ss, yp, y_ss, rate, N, d, ci, co):
        wpk, bias, kw, _ = self.packed[prefix]
        nv.call('iunet_dl_conv_fwd', self.dt, self.dim, xp, x_ss, yp, y_ss, nv.ptr(wpk), kw, 1, nv.int_array([rate]), nv.int_array([0]),
                nv.int_array([0]), None, None, nv.ptr(bias), None, 1.0, None, 1, N, d[0], d[1], d[2], ci, co, nv.stream())


class UPerNetEngineF32(_UPerNet, EncoderEngineF32):
    """The fp32 UPerNet forward (planar fp32 activations, the f32-input matrix instruction): the default prediction form of a UPerNet
    module, within the project's 1e-3 logit promise of the CPU fp32 path."""

    def __init__(self, dim=2, levels=4, base=32, cin=1, ncls=2, device='cuda', decoder_channels=256):
        EncoderEngineF32.__init__(self, dim, levels, base, cin, ncls, device)
        self._setup(decoder_channels)

    def _conv(self, prefix, xp, x_ss, yp, y_ss, rate, N, d, ci, co):
        w, b, kw, _ = self.packed[prefix]
        nv.call('iunet_dl_f32_conv_fwd', self.dim, rate, xp, x_ss, yp, y_ss, nv.ptr(w), kw, nv.ptr(b), None, N, d[0], d[1], d[2], ci, co,
                nv.stream())
