"""Host-side plan of the native LinkNet forward (Chaurasia & Culurciello 2017, smp's Linknet decoder on this project's encoder): folded
eval-mode BatchNorm, 16-bit (LinkNetEngine, on engine.EncoderEngine's encoder) and fp32 (LinkNetEngineF32, on engine_f32.EncoderEngineF32's).
Both keep the `load_eval` / `infer(...)` interface predict.py drives.

Graph.  X^l is the encoder's level-l output (enc{l}, the U-Net's encoder); D^{L-1} = X^{L-1}; for l = L-2 .. 0 the block dec{l} reads
D^{l+1}: a1 = relu(bn1(conv1x1(D^{l+1}))) (ch[l+1] -> m, m = ch[l+1] / 4), a2 = relu(bn2(convT k4 s2 p1(a1))) (m -> m, 2x grid),
D^l = relu(bn3(conv1x1(a2))) + X^l (m -> ch[l]); the head reads D^0.  There is no "prefinal" block: smp's encoders start at stride 2
and need one, this encoder's enc0 runs at full resolution.  Each block is three csrc/linknet.hip launches with the BatchNorm folded into
the operators (bias + ReLU epilogues, the skip added in fp32 by the last one).
"""
import torch

from . import _native as nv
from .engine import BN_EPS, EncoderEngine, _vox
from .engine_f32 import EncoderEngineF32
from .topology import BN_KEYS


class _Link:
    """What the two LinkNet engines share: workspace sizes, the decoder's operator packing."""

    def _bufs(self, dims, N):
        """(element counts of the workspace: x{l} (encoder outputs), a{l} (conv1 of a stage), pin{l} (pooled input), t1{l} / t2{l}
        (a1 / a2 of block l), d{l} (D^l, l < L-1); no fp32 buffers)."""
        out, ch = {}, self.ch
        for l in range(self.levels):
            v = _vox(dims[l])
            out[f'x{l}'] = N * ch[l] * v
            out[f'a{l}'] = N * ch[l] * v
            if l > 0:
                out[f'pin{l}'] = N * ch[l - 1] * v
            if l < self.levels - 1:
                m = ch[l + 1] // 4
                out[f't1{l}'] = N * m * _vox(dims[l + 1])
                out[f't2{l}'] = N * m * v
                out[f'd{l}'] = N * ch[l] * v
        return out, {}

    def _pack_decoder(self, src, dtype_code):
        """Fold bn1 / bn2 / bn3 into conv1 / up / conv2 of every block: {dec{l}.conv1|up|conv2: (operator, bias), head}."""
        P = {}
        for l in range(self.levels - 2, -1, -1):
            m = self.ch[l + 1] // 4
            for key, bn, kind, co, ci in (('conv1', 'bn1', 0, m, self.ch[l + 1]), ('up', 'bn2', 2, m, m), ('conv2', 'bn3', 0, self.ch[l], m)):
                w = src(f'dec{l}.{key}.weight')
                g = [src(f'dec{l}.{bn}.{k}') for k in BN_KEYS]
                dst = torch.empty(nv.lib().iunet_lk_pack_elems(self.dim, kind, co, ci), dtype=self._pack_dtype, device=self.device)
                bias = torch.empty(co, dtype=torch.float32, device=self.device)
                nv.call('iunet_lk_pack', dtype_code, self.dim, kind, nv.ptr(w), nv.ptr(g[0]), nv.ptr(g[1]), nv.ptr(g[2]), nv.ptr(g[3]),
                        BN_EPS, nv.ptr(dst), nv.ptr(bias), co, ci, nv.stream())
                P[f'dec{l}.{key}'] = (dst, bias, g + [w])          # (the sources stay alive until the pack has run)
        P['head'] = (src('head.weight').reshape(self.ncls, self.ch[0]).contiguous(), src('head.bias'))
        return P


class LinkNetEngine(_Link, EncoderEngine):
    """The 16-bit (fp16 / bf16) LinkNet forward with folded BatchNorm."""

    def infer(self, x, x_strides, N, D, H, W, logits=None, probs=None, cls=None, out_strides=None,
              divisor=1.0, accumulate=False, features_only=False):
        """engine.Engine.infer's contract on the LinkNet graph (features_only: the head's input D^0, NHWC8c, contiguous)."""
        ws = self._encoder(x, x_strides, N, D, H, W)
        dims, L, ch, s, P = ws['dims'], self.levels, self.ch, nv.stream(), self._P
        for l in range(L - 2, -1, -1):
            d, di, v, vi, m = dims[l], dims[l + 1], _vox(dims[l]), _vox(dims[l + 1]), ch[l + 1] // 4
            src = ws[f'x{l + 1}'] if l == L - 2 else ws[f'd{l + 1}']
            self._lk(0, 'conv1', l, P(src), ch[l + 1] * vi, P(ws[f't1{l}']), m * vi, N, di, ch[l + 1], m, s)
            self._lk(1, 'up', l, P(ws[f't1{l}']), m * vi, P(ws[f't2{l}']), m * v, N, di, m, m, s)
            self._lk(0, 'conv2', l, P(ws[f't2{l}']), m * v, P(ws[f'd{l}']), ch[l] * v, N, d, m, ch[l], s, skip=(P(ws[f'x{l}']), ch[l] * v))
        if features_only:
            return ws['d0']
        hw, hb = self.packed['head']
        nv.call('iunet_head_fwd', self.dt, P(ws['d0']), ch[0] * _vox(dims[0]), ch[0], nv.ptr(hw), nv.ptr(hb),
                self.ncls, nv.ptr(logits), nv.ptr(probs), nv.ptr(cls), nv.ll_array(self._out_strides(out_strides, D, H, W)),
                float(divisor), int(bool(accumulate)), N, D, H, W, s)

    def _lk(self, kind, key, l, xp, x_ss, yp, y_ss, N, d, ci, co, s, skip=(None, 0)):
        wpk, bias, _ = self.packed[f'dec{l}.{key}']
        nv.call('iunet_lk_conv_fwd', self.dt, self.dim, kind, xp, x_ss, yp, y_ss, nv.ptr(wpk), None, None, nv.ptr(bias), skip[0], skip[1],
                None, 1, N, d[0], d[1], d[2], ci, co, s)


class LinkNetEngineF32(_Link, EncoderEngineF32):
    """The fp32 LinkNet forward (planar fp32 activations, the f32-input matrix instruction): the default prediction form of a LinkNet
    module, within the project's 1e-3 logit promise of the CPU fp32 path."""

    def infer(self, x, x_strides, N, D, H, W, logits=None, probs=None, cls=None, out_strides=None,
              divisor=1.0, accumulate=False, features_only=False):
        """engine_f32.EngineF32.infer's contract on the LinkNet graph (features_only: D^0, planar fp32)."""
        ws = self._encoder(x, x_strides, N, D, H, W)
        dims, L, ch, s, P = ws['dims'], self.levels, self.ch, nv.stream(), self._P

        def lk(kind, name, xp, x_ss, yp, y_ss, d, ci, co, skip=(None, 0)):
            w, b, _ = self.packed[name]
            nv.call('iunet_lk_f32_conv_fwd', self.dim, kind, xp, x_ss, yp, y_ss, nv.ptr(w), nv.ptr(b), skip[0], skip[1],
                    N, d[0], d[1], d[2], ci, co, s)

        for l in range(L - 2, -1, -1):
            d, di, v, vi, m = dims[l], dims[l + 1], _vox(dims[l]), _vox(dims[l + 1]), ch[l + 1] // 4
            src = ws[f'x{l + 1}'] if l == L - 2 else ws[f'd{l + 1}']
            lk(0, f'dec{l}.conv1', P(src), ch[l + 1] * vi, P(ws[f't1{l}']), m * vi, di, ch[l + 1], m)
            lk(1, f'dec{l}.up', P(ws[f't1{l}']), m * vi, P(ws[f't2{l}']), m * v, di, m, m)
            lk(0, f'dec{l}.conv2', P(ws[f't2{l}']), m * v, P(ws[f'd{l}']), ch[l] * v, d, m, ch[l], skip=(P(ws[f'x{l}']), ch[l] * v))
        if features_only:
            return ws['d0']
        hw, hb = self.packed['head']
        nv.call('iunet_f32_head_fwd', P(ws['d0']), ch[0] * _vox(dims[0]), ch[0], nv.ptr(hw), nv.ptr(hb), self.ncls,
                nv.ptr(logits), nv.ptr(probs), nv.ptr(cls), nv.ll_array(self._out_strides(out_strides, D, H, W)), float(divisor),
                int(bool(accumulate)), N, D, H, W, s)
