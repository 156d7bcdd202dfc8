"""Host-side plan of the native DeepLabV3 forward (Chen et al. 2017, smp's DeepLabV3 decoder on this project's encoder): folded eval-mode
BatchNorm, 16-bit (DeepLabV3Engine, on engine.EncoderEngine's encoder) and fp32 (DeepLabV3EngineF32, on engine_f32.EncoderEngineF32's).  Both keep
the `load_eval` / `infer(...)` interface predict.py drives.

Graph.  X = X^{L-1}, the encoder's coarsest output (enc{L-1}; the U-Net's encoder reaches output stride s = 2^(L-1) there, so smp's
dilated encoder stages have no counterpart).  On that grid: the four spatial ASPP branches (b0 1x1, b1..b3 3^d with the atrous rates) write
the four C-channel slots of one buffer, the pooling branch becomes a per-sample bias of the projection (its W_proj[:, 4C:5C] bp[n]), the
projection reads the four slots as one 4C-channel input, then dec.conv and the 1x1 head give the coarse logits; csrc/deeplab.hip upsamples
them x s (align_corners=True) into iunet_head_fwd's output contract (logits / probs / class map, strides, divisor, accumulate).  Eval-mode
dropout is the identity.
"""
import torch

from . import _native as nv
from .engine import BN_EPS, CoarseLogits, EncoderEngine, _vox
from .engine_f32 import EncoderEngineF32
from .topology import BN_KEYS

BRANCHES = ('aspp.b0', 'aspp.b1', 'aspp.b2', 'aspp.b3')


class _DeepLab(CoarseLogits):
    """What the two DeepLabV3 engines share: rates, operator packing, workspace sizes, the decoder's sequence."""

    def _setup(self, decoder_channels, rates):
        self.C = int(decoder_channels)
        self.rates = (0,) + tuple(int(r) for r in rates)         # b0 is the 1x1 branch
        if self.C % 32 or not (32 <= self.C <= 512) or len(self.rates) != 4 or min(self.rates[1:]) <= 0:
            raise NotImplementedError(f'DeepLabV3 engine: decoder_channels {self.C} (a multiple of 32 in 32 .. 512), rates {rates}')
        self.kvol = 3 ** self.dim
        self.coarse_level = self.levels - 1

    def _bufs(self, dims, N):
        """(element counts of the activation workspace, of the fp32 workspace): x{l} / a{l} / pin{l} of the encoder, cat (the 4 branch
        slots), proj (P), feat (F); fp32: lc (coarse logits), xmean, ypool, bp, psb."""
        act, ch, C = {}, self.ch, self.C
        for l in range(self.levels):
            v = _vox(dims[l])
            act[f'x{l}'] = N * ch[l] * v
            act[f'a{l}'] = N * ch[l] * v
            if l > 0:
                act[f'pin{l}'] = N * ch[l - 1] * v
        vc = _vox(dims[-1])
        act['cat'] = N * 4 * C * vc
        act['proj'] = N * C * vc
        act['feat'] = N * C * vc
        f32 = {'lc': N * self.ncls * vc, 'xmean': N * ch[-1], 'ypool': N * C, 'bp': N * C, 'psb': N * C}
        return act, f32

    def _pack_decoder(self, src, dtype_code):
        """Fold every decoder BatchNorm into its conv: {prefix: (operator, bias, row length)}; the projection's operator covers the four
        spatial slots (K = 4C), its pooling columns stay fp32 in the master weight (iunet_dl_pool_psb reads them)."""
        P, C, Cb = {}, self.C, self.ch[-1]
        convs = [(b, 1 if r == 0 else 3, Cb) for b, r in zip(BRANCHES, self.rates)] + [('aspp.project', 1, 5 * C), ('dec', 3, C)]
        for prefix, ksz, cin_tot in convs:
            cin = 4 * C if prefix == 'aspp.project' else cin_tot
            kw = (1 if ksz == 1 else self.kvol) * cin
            w = src(f'{prefix}.conv.weight')
            g = [src(f'{prefix}.bn.{k}') for k in BN_KEYS]
            dst = torch.empty(C * kw, dtype=self._pack_dtype, device=self.device)
            bias = torch.empty(C, dtype=torch.float32, device=self.device)
            nv.call('iunet_dl_pack', dtype_code, self.dim, 0, ksz, nv.ptr(w), nv.ptr(g[0]), nv.ptr(g[1]), nv.ptr(g[2]), nv.ptr(g[3]), BN_EPS,
                    nv.ptr(dst), nv.ptr(bias), C, cin, cin_tot, 0, 0, kw, nv.stream())
            P[prefix] = (dst, bias, kw, g + [w])               # (the sources stay alive until the pack has run)
        P['pool'] = [src('aspp.pool.conv.weight')] + [src(f'aspp.pool.bn.{k}') for k in BN_KEYS]
        P['proj_src'] = [src('aspp.project.conv.weight'), src('aspp.project.bn.weight'), src('aspp.project.bn.running_var')]
        P['head'] = (src('head.weight').reshape(self.ncls, C).contiguous(), src('head.bias'))
        return P

    def _decode(self, ws, N):
        """The ASPP and dec.conv on the coarse grid into ws['feat']: the pooling branch into ws['psb'] (already x the projection's folded
        scale), the four spatial branches into their slots of ws['cat'], the projection, dec.conv."""
        dims, C, Cb, P, s = ws['dims'], self.C, self.ch[-1], self._P, nv.stream()
        dc, vc, X = dims[-1], _vox(dims[-1]), ws[f'x{self.levels - 1}']
        nv.call('iunet_dl_chansum', self.dt, nv.ptr(X), Cb * vc, nv.ptr(ws['xmean']), 1.0 / vc, Cb, N, vc, s)
        wp, g, b, rm, rv = self.packed['pool']
        nv.call('iunet_dl_pool_gemv', nv.ptr(ws['xmean']), nv.ptr(wp), nv.ptr(ws['ypool']), None, N, Cb, C, s)
        wj, pg, pv = self.packed['proj_src']
        nv.call('iunet_dl_pool_psb', nv.ptr(ws['ypool']), None, None, nv.ptr(g), nv.ptr(b), nv.ptr(rm), nv.ptr(rv), BN_EPS, nv.ptr(ws['bp']),
                nv.ptr(wj), nv.ptr(pg), nv.ptr(pv), nv.ptr(ws['psb']), N, C, s)
        for k, (prefix, rate) in enumerate(zip(BRANCHES, self.rates)):
            self._conv(prefix, P(X), Cb * vc, P(ws['cat'], k * C * vc), 4 * C * vc, rate, N, dc, Cb)
        self._conv('aspp.project', P(ws['cat']), 4 * C * vc, P(ws['proj']), C * vc, 0, N, dc, 4 * C, psb=ws['psb'])
        self._conv('dec', P(ws['proj']), C * vc, P(ws['feat']), C * vc, 1, N, dc, C)


class DeepLabV3Engine(_DeepLab, EncoderEngine):
    """The 16-bit (fp16 / bf16) DeepLabV3 forward with folded BatchNorm."""

    def __init__(self, dim=2, levels=4, base=32, cin=1, ncls=2, act_dtype=torch.float16, device='cuda', decoder_channels=256,
                 rates=(12, 24, 36)):
        EncoderEngine.__init__(self, dim, levels, base, cin, ncls, act_dtype, device)
        self._setup(decoder_channels, rates)

    def _conv(self, prefix, xp, x_ss, yp, y_ss, rate, N, d, ci, psb=None):
        wpk, bias, kw, _ = self.packed[prefix]
        nv.call('iunet_dl_conv_fwd', self.dt, self.dim, xp, x_ss, yp, y_ss, nv.ptr(wpk), kw, 1, nv.int_array([rate]), nv.int_array([0]),
                nv.int_array([0]), None, None, nv.ptr(bias), nv.ptr(psb), 1.0, None, 1, N, d[0], d[1], d[2], ci, self.C, nv.stream())


class DeepLabV3EngineF32(_DeepLab, EncoderEngineF32):
    """The fp32 DeepLabV3 forward (planar fp32 activations, the f32-input matrix instruction): the default prediction form of a DeepLabV3
    module, within the project's 1e-3 logit promise of the CPU fp32 path."""

    def __init__(self, dim=2, levels=4, base=32, cin=1, ncls=2, device='cuda', decoder_channels=256, rates=(12, 24, 36)):
        EncoderEngineF32.__init__(self, dim, levels, base, cin, ncls, device)
        self._setup(decoder_channels, rates)

    def _conv(self, prefix, xp, x_ss, yp, y_ss, rate, N, d, ci, psb=None):
        w, b, kw, _ = self.packed[prefix]
        nv.call('iunet_dl_f32_conv_fwd', self.dim, rate, xp, x_ss, yp, y_ss, nv.ptr(w), kw, nv.ptr(b), nv.ptr(psb), N, d[0], d[1], d[2],
                ci, self.C, nv.stream())
