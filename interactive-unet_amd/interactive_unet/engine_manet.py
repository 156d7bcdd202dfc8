"""Host-side plan of the native MA-Net forward (Fan et al. 2020: a position attention block on the encoder's coarsest output and decoder
blocks whose upsampled input is gated by two squeeze-and-excitation branches, on this project's encoder): folded eval-mode BatchNorm,
16-bit (MANetEngine, on engine.EncoderEngine's encoder) and fp32 (MANetEngineF32, on engine_f32.EncoderEngineF32's).  Both keep the
`load_eval` / `infer(...)` interface predict.py drives.

Graph (B = L - 1 the bottom level, Cb = ch[B], T = the voxels of G_B, the tokens).
  Q = conv1x1(X^B) + b (pab.top), Kc = conv1x1(X^B) + b (pab.center), V = conv3^d(X^B) + b (pab.bottom); S[i][j] = sum_k Kc[i][k] Q[j][k];
  A = the row softmax of S; Y = X^B + A V; Z = relu(bn(conv3^d(Y))) (pab.out).
  dec{l}, l = B-1 .. 0, on x = Z or the previous block's output: h = relu(bn(conv1x1(relu(bn(conv3^d(x)))))) (hl3, hl1);
  g = sigmoid(se_hl(mean h)) + sigmoid(se_ll(mean X^l)); u = nearest_up2(h) g; the stage conv{1,2} / bn{1,2} on concat(X^l, u).
  The head reads dec0's output at full resolution.
The convs with a BatchNorm are deeplab.hip's gathered GEMMs with the norm folded; Q, Kc and V are raw convs (their biases are added by the
attention kernel: on load for Q and Kc, once in the residual pass for V, the rows of A summing to 1).  csrc/manet.hip has the attention
(iunet_ma_attn_fwd / iunet_ma_f32_attn_fwd), the gates (iunet_ma_gate on iunet_dl_chansum's means) and the gated upsampling into the
concat buffer's second slot (iunet_ma_up_gate); the skip is copied into the first slot by iunet_pn_resize at equal grids.  The workspace
table is `_MANet._bufs`.
"""
import torch

from . import _native as nv
from .engine import BN_EPS, EncoderEngine, _vox
from .engine_f32 import EncoderEngineF32
from .topology import BN_KEYS

QK = 64                      # width of the queries and keys
MAX_TOKENS = 65536           # the attention kernels' limit on T
SE_KEYS = tuple(f'{se}.{fc}.{k}' for se in ('se_hl', 'se_ll') for fc in ('fc1', 'fc2') for k in ('weight', 'bias'))


def blocks(levels):
    """The levels of the decoder blocks in forward (parameter) order: B-1 .. 0."""
    return list(range(levels - 2, -1, -1))


def gate_width(c):
    return max(c // 16, 1)


def conv_table(levels, ch):
    """(prefix, weight name, BatchNorm prefix or None: a raw conv with a bias, kernel size, input channels, output channels) of every
    decoder conv, in parameter order."""
    Cb = ch[-1]
    t = [('pab.top', 'pab.top.conv', None, 1, Cb, QK), ('pab.center', 'pab.center.conv', None, 1, Cb, QK),
         ('pab.bottom', 'pab.bottom.conv', None, 3, Cb, Cb), ('pab.out', 'pab.out.conv', 'pab.out.bn', 3, Cb, Cb)]
    for l in blocks(levels):
        t += [(f'dec{l}.hl3', f'dec{l}.hl3.conv', f'dec{l}.hl3.bn', 3, ch[l + 1], ch[l + 1]),
              (f'dec{l}.hl1', f'dec{l}.hl1.conv', f'dec{l}.hl1.bn', 1, ch[l + 1], ch[l]),
              (f'dec{l}.conv1', f'dec{l}.conv1', f'dec{l}.bn1', 3, 2 * ch[l], ch[l]),
              (f'dec{l}.conv2', f'dec{l}.conv2', f'dec{l}.bn2', 3, ch[l], ch[l])]
    return t


def check_setup(name, levels, ch):
    if not (3 <= levels <= 5) or ch[-1] % 128 or ch[-1] > 512:
        raise NotImplementedError(f'{name}: MA-Net supports 3 .. 5 levels and at most 512 channels on the coarsest level, got {levels} levels, '
                                  f'{ch[-1]} channels')


def gated_concat(dt, dim, P, ws, l, se, dims, ch, N):
    """The launches between hl1 and the stage of block l, the same in prediction and in training: the means of h and of the skip
    (iunet_dl_chansum), the gates g from the eight tensors `se`, the skip into the concat buffer's first slot (iunet_pn_resize at equal
    grids) and nearest_up2(h) g into its second.  ws holds h{l}, x{l}, cat{l}, mh{l}, ms{l}, g{l}, hid{l}, sig{l}; P: tensor, element
    offset -> pointer."""
    d, di, v, vi, c, s = dims[l], dims[l + 1], _vox(dims[l]), _vox(dims[l + 1]), ch[l], nv.stream()
    nv.call('iunet_dl_chansum', dt, P(ws[f'h{l}']), c * vi, nv.ptr(ws[f'mh{l}']), 1.0 / vi, c, N, vi, s)
    nv.call('iunet_dl_chansum', dt, P(ws[f'x{l}']), c * v, nv.ptr(ws[f'ms{l}']), 1.0 / v, c, N, v, s)
    nv.call('iunet_ma_gate', nv.ptr(ws[f'mh{l}']), nv.ptr(ws[f'ms{l}']), *[nv.ptr(t) for t in se], nv.ptr(ws[f'g{l}']), nv.ptr(ws[f'hid{l}']),
            nv.ptr(ws[f'sig{l}']), c, gate_width(c), N, s)
    nv.call('iunet_pn_resize', dt, dim, P(ws[f'x{l}']), c * v, d[0], d[1], d[2], None, None, None, 0, None, None, P(ws[f'cat{l}']), 2 * c * v,
            d[0], d[1], d[2], c, N, s)
    nv.call('iunet_ma_up_gate', dt, dim, P(ws[f'h{l}']), c * vi, None, None, nv.ptr(ws[f'g{l}']), P(ws[f'cat{l}'], c * v), 2 * c * v,
            di[0], di[1], di[2], c, N, s)


def check_tokens(T):
    if T > MAX_TOKENS:
        raise ValueError(f'MA-Net: the coarsest grid has {T} tokens; the position attention supports at most {MAX_TOKENS} '
                         f'(use a smaller input, or more levels)')


class _MANet:
    """What the two MA-Net engines share: operator packing, workspace sizes, the decoder's sequence."""

    def _setup(self):
        check_setup(type(self).__name__, self.levels, self.ch)
        self.kvol = 3 ** self.dim
        self.zeros = torch.zeros(max(self.ch), dtype=torch.float32, device=self.device)

    def _bufs(self, dims, N):
        """(element counts of the activation workspace, of the fp32 workspace): x{l} / a{l} / pin{l} of the encoder; q, k (64 channels) and
        v, y (Y), z (Z) on G_B; per block t{l} (hl3's output) and h{l} on G_{l+1}, cat{l} (skip, gated upsampling), c1{l} and d{l} (the
        stage) on G_l; fp32: lse (a row's log-sum-exp), mh{l} / ms{l} (the means of h and the skip), g{l}, hid{l}, sig{l} (the gates)."""
        act, f32, ch = {}, {}, self.ch
        for l in range(self.levels):
            v = _vox(dims[l])
            act[f'x{l}'] = N * ch[l] * v
            act[f'a{l}'] = N * ch[l] * v
            if l > 0:
                act[f'pin{l}'] = N * ch[l - 1] * v
        T, Cb = _vox(dims[-1]), ch[-1]
        act.update(q=N * QK * T, k=N * QK * T, v=N * Cb * T, y=N * Cb * T, z=N * Cb * T)
        f32['lse'] = N * T
        for l in blocks(self.levels):
            v, vi, c = _vox(dims[l]), _vox(dims[l + 1]), ch[l]
            act.update({f't{l}': N * ch[l + 1] * vi, f'h{l}': N * c * vi, f'cat{l}': N * 2 * c * v, f'c1{l}': N * c * v, f'd{l}': N * c * v})
            f32.update({f'mh{l}': N * c, f'ms{l}': N * c, f'g{l}': N * c, f'hid{l}': N * 2 * gate_width(c), f'sig{l}': N * 2 * c})
        return act, f32

    def _pack_decoder(self, src, dtype_code):
        """{prefix: (operator, bias, row length, kept sources)}: every BatchNorm folded into its conv, Q / Kc / V raw (`_pack_raw`) with
        their own biases; {dec{l}.se: the eight gate tensors}; the head."""
        P = {}
        for prefix, wn, bn, ksz, cin, cout in conv_table(self.levels, self.ch):
            w = src(wn + '.weight')
            if bn is None:
                P[prefix] = self._pack_raw(w, src(wn + '.bias'), ksz, cin, cout)
                continue
            kw = (1 if ksz == 1 else self.kvol) * cin
            dst = torch.empty(cout * kw, dtype=self._pack_dtype, device=self.device)
            g, bias = [src(f'{bn}.{k}') for k in BN_KEYS], torch.empty(cout, dtype=torch.float32, device=self.device)
            nv.call('iunet_dl_pack', dtype_code, self.dim, 0, ksz, nv.ptr(w), nv.ptr(g[0]), nv.ptr(g[1]), nv.ptr(g[2]), nv.ptr(g[3]), BN_EPS,
                    nv.ptr(dst), nv.ptr(bias), cout, cin, cin, 0, 0, kw, nv.stream())
            P[prefix] = (dst, bias, kw, g + [w])               # (the sources stay alive until the pack has run)
        for l in blocks(self.levels):
            P[f'dec{l}.se'] = [src(f'dec{l}.{k}') for k in SE_KEYS]
        P['head'] = (src('head.weight').reshape(self.ncls, self.ch[0]).contiguous(), src('head.bias'))
        return P

    def _decode(self, ws, N):
        """The position attention block on X^B, then the decoder blocks: dec0's output in ws['d0']."""
        dims, ch, L, P = ws['dims'], self.ch, self.levels, self._P
        B, Cb, db = L - 1, ch[-1], dims[-1]
        T = _vox(db)
        check_tokens(T)
        X = P(ws[f'x{B}'])
        self._raw('pab.top', X, Cb * T, P(ws['q']), QK * T, 0, N, db, Cb, QK)
        self._raw('pab.center', X, Cb * T, P(ws['k']), QK * T, 0, N, db, Cb, QK)
        self._raw('pab.bottom', X, Cb * T, P(ws['v']), Cb * T, 1, N, db, Cb, Cb)
        self._attn(ws, X, N, Cb, T)
        self._conv('pab.out', P(ws['y']), Cb * T, P(ws['z']), Cb * T, 1, N, db, Cb, Cb)
        src = ws['z']
        for l in blocks(L):
            d, di, v, vi, c, ci = dims[l], dims[l + 1], _vox(dims[l]), _vox(dims[l + 1]), ch[l], ch[l + 1]
            self._conv(f'dec{l}.hl3', P(src), ci * vi, P(ws[f't{l}']), ci * vi, 1, N, di, ci, ci)
            self._conv(f'dec{l}.hl1', P(ws[f't{l}']), ci * vi, P(ws[f'h{l}']), c * vi, 0, N, di, ci, c)
            gated_concat(self.dt, self.dim, P, ws, l, self.packed[f'dec{l}.se'], dims, ch, N)
            self._conv(f'dec{l}.conv1', P(ws[f'cat{l}']), 2 * c * v, P(ws[f'c1{l}']), c * v, 1, N, d, 2 * c, c)
            self._conv(f'dec{l}.conv2', P(ws[f'c1{l}']), c * v, P(ws[f'd{l}']), c * v, 1, N, d, c, c)
            src = ws[f'd{l}']

    def infer(self, x, x_strides, N, D, H, W, logits=None, probs=None, cls=None, out_strides=None,
              divisor=1.0, accumulate=False, features_only=False):
        """engine.Engine.infer's contract on the MA-Net graph (features_only: the head's input, dec0's output, contiguous)."""
        ws = self._encoder(x, x_strides, N, D, H, W)
        self._decode(ws, N)
        if features_only:
            return ws['d0']
        hw, hb = self.packed['head']
        args = (self._P(ws['d0']), self.ch[0] * D * H * W, self.ch[0], nv.ptr(hw), nv.ptr(hb), self.ncls, nv.ptr(logits), nv.ptr(probs),
                nv.ptr(cls), nv.ll_array(self._out_strides(out_strides, D, H, W)), float(divisor), int(bool(accumulate)), N, D, H, W, nv.stream())
        if self.act_dtype == torch.float32:
            nv.call('iunet_f32_head_fwd', *args)
        else:
            nv.call('iunet_head_fwd', self.dt, *args)


class MANetEngine(_MANet, EncoderEngine):
    """The 16-bit (fp16 / bf16) MA-Net forward with folded BatchNorm."""

    def __init__(self, dim=2, levels=4, base=32, cin=1, ncls=2, act_dtype=torch.float16, device='cuda'):
        EncoderEngine.__init__(self, dim, levels, base, cin, ncls, act_dtype, device)
        self._setup()

    def _pack_raw(self, w, bias, ksz, cin, cout):
        kw = (1 if ksz == 1 else self.kvol) * cin
        dst = torch.empty(cout * kw, dtype=self._pack_dtype, device=self.device)
        nv.call('iunet_dl_pack', self.dt, self.dim, 0, ksz, nv.ptr(w), None, None, None, None, 0.0, nv.ptr(dst), None, cout, cin, cin, 0, 0, kw,
                nv.stream())
        return (dst, bias, kw, [w])

    def _gemm(self, prefix, xp, x_ss, yp, y_ss, rate, N, d, ci, co, epi):
        wpk, bias, kw, _ = self.packed[prefix]
        nv.call('iunet_dl_conv_fwd', self.dt, self.dim, xp, x_ss, yp, y_ss, nv.ptr(wpk), kw, 1, nv.int_array([rate]), nv.int_array([0]),
                nv.int_array([0]), None, None, nv.ptr(bias) if epi else None, None, 1.0, None, epi, N, d[0], d[1], d[2], ci, co, nv.stream())

    def _conv(self, prefix, xp, x_ss, yp, y_ss, rate, N, d, ci, co):
        self._gemm(prefix, xp, x_ss, yp, y_ss, rate, N, d, ci, co, 1)

    def _raw(self, prefix, xp, x_ss, yp, y_ss, rate, N, d, ci, co):
        self._gemm(prefix, xp, x_ss, yp, y_ss, rate, N, d, ci, co, 0)

    def _attn(self, ws, X, N, Cb, T):
        P, bias = self._P, lambda prefix: nv.ptr(self.packed[prefix][1])
        nv.call('iunet_ma_attn_fwd', self.dt, P(ws['q']), QK * T, bias('pab.top'), P(ws['k']), QK * T, bias('pab.center'), P(ws['v']), Cb * T,
                X, Cb * T, bias('pab.bottom'), P(ws['y']), Cb * T, nv.ptr(ws['lse']), Cb, T, N, nv.stream())


class MANetEngineF32(_MANet, EncoderEngineF32):
    """The fp32 MA-Net forward (planar fp32 activations, the f32-input matrix instruction): the default prediction form of an MA-Net
    module, within the project's 1e-3 logit promise of the CPU fp32 path."""

    def __init__(self, dim=2, levels=4, base=32, cin=1, ncls=2, device='cuda'):
        EncoderEngineF32.__init__(self, dim, levels, base, cin, ncls, device)
        self._setup()

    def _pack_raw(self, w, bias, ksz, cin, cout):
        taps = 1 if ksz == 1 else self.kvol
        dst = torch.empty(nv.lib().iunet_f32_pack_conv_elems(cout, cin, taps), dtype=torch.float32, device=self.device)
        nv.call('iunet_f32_pack_conv', nv.ptr(w), nv.ptr(dst), None, None, None, None, None, BN_EPS, cout, cin, taps, 0, nv.stream())
        return (dst, bias, taps, [w])

    def _conv(self, prefix, xp, x_ss, yp, y_ss, rate, N, d, ci, co):
        w, b, kw, _ = self.packed[prefix]
        nv.call('iunet_dl_f32_conv_fwd', self.dim, rate, xp, x_ss, yp, y_ss, nv.ptr(w), kw, nv.ptr(b), None, N, d[0], d[1], d[2], ci, co,
                nv.stream())

    def _raw(self, prefix, xp, x_ss, yp, y_ss, rate, N, d, ci, co):
        """conv + bias without an activation (the attention kernel is then given zero biases)."""
        w, b, _, _ = self.packed[prefix]
        nv.call('iunet_f32_conv_fwd', self.dim, xp, 0, nv.ll_array((x_ss, _vox(d), d[1] * d[2], d[2], 1)), yp, y_ss, nv.ptr(w), nv.ptr(b),
                N, d[0], d[1], d[2], ci, co, 0, 0 if rate else 2, nv.stream())

    def _attn(self, ws, X, N, Cb, T):
        P, z = self._P, nv.ptr(self.zeros)
        nv.call('iunet_ma_f32_attn_fwd', P(ws['q']), QK * T, z, P(ws['k']), QK * T, z, P(ws['v']), Cb * T, X, Cb * T, z, P(ws['y']), Cb * T,
                nv.ptr(ws['lse']), Cb, T, N, nv.stream())
