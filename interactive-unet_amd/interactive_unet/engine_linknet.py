"""Host-side plan of the native LinkNet forward (Chaurasia & Culurciello 2017, smp's Linknet decoder on this project's encoder): folded
eval-mode BatchNorm, 16-bit (LinkNetEngine, on engine.Engine's encoder launches) and fp32 (LinkNetEngineF32, on engine_f32.EngineF32's).
Both keep the `load_eval` / `infer(...)` interface predict.py drives.

Graph.  X^l is the encoder's level-l output (enc{l}, the U-Net's encoder); D^{L-1} = X^{L-1}; for l = L-2 .. 0 the block dec{l} reads
D^{l+1}: a1 = relu(bn1(conv1x1(D^{l+1}))) (ch[l+1] -> m, m = ch[l+1] / 4), a2 = relu(bn2(convT k4 s2 p1(a1))) (m -> m, 2x grid),
D^l = relu(bn3(conv1x1(a2))) + X^l (m -> ch[l]); the head reads D^0.  There is no "prefinal" block: smp's encoders start at stride 2
and need one, this encoder's enc0 runs at full resolution.  Each block is three csrc/linknet.hip launches with the BatchNorm folded into
the operators (bias + ReLU epilogues, the skip added in fp32 by the last one).
"""
import ctypes

import torch

from . import _native as nv
from .engine import BN_EPS, Engine, _vox
from .engine_f32 import EngineF32


def _bufs(levels, ch, dims, N):
    """Element counts of the forward workspace: x{l} (encoder outputs), a{l} (conv1 of a stage), pin{l} (pooled input), t1{l} / t2{l}
    (a1 / a2 of block l), d{l} (D^l, l < L-1)."""
    out = {}
    for l in range(levels):
        v = _vox(dims[l])
        out[f'x{l}'] = N * ch[l] * v
        out[f'a{l}'] = N * ch[l] * v
        if l > 0:
            out[f'pin{l}'] = N * ch[l - 1] * v
        if l < levels - 1:
            m = ch[l + 1] // 4
            out[f't1{l}'] = N * m * _vox(dims[l + 1])
            out[f't2{l}'] = N * m * v
            out[f'd{l}'] = N * ch[l] * v
    return out


class _Link:
    """What the two LinkNet engines share: names, workspace sizes."""

    def enc_names(self):
        return [f'enc{l}' for l in range(self.levels)]

    def enc_io(self, prefix):
        l = int(prefix[3:])
        return (self.cin if l == 0 else self.ch[l - 1]), self.ch[l]

    def _graph(self):
        return None          # (no C-sequenced handle for LinkNet: every forward is sequenced from Python)

    def bytes_per_slice(self, input_size):
        """Workspace bytes of one 2-D slice of input_size^2 (predict.find_max_batch_size)."""
        S = input_size
        dims = [(1, S >> l, S >> l) for l in range(self.levels)]
        return sum(_bufs(self.levels, self.ch, dims, 1).values()) * self._es

    def _pack_decoder(self, src, dtype_code):
        """Fold bn1 / bn2 / bn3 into conv1 / up / conv2 of every block: {dec{l}.conv1|up|conv2: (operator, bias)}."""
        P = {}
        for l in range(self.levels - 2, -1, -1):
            m = self.ch[l + 1] // 4
            for key, bn, kind, co, ci in (('conv1', 'bn1', 0, m, self.ch[l + 1]), ('up', 'bn2', 2, m, m), ('conv2', 'bn3', 0, self.ch[l], m)):
                w = src(f'dec{l}.{key}.weight')
                g = [src(f'dec{l}.{bn}.{k}') for k in ('weight', 'bias', 'running_mean', 'running_var')]
                dst = torch.empty(nv.lib().iunet_lk_pack_elems(self.dim, kind, co, ci), dtype=self._pack_dtype, device=self.device)
                bias = torch.empty(co, dtype=torch.float32, device=self.device)
                nv.call('iunet_lk_pack', dtype_code, self.dim, kind, nv.ptr(w), nv.ptr(g[0]), nv.ptr(g[1]), nv.ptr(g[2]), nv.ptr(g[3]),
                        BN_EPS, nv.ptr(dst), nv.ptr(bias), co, ci, nv.stream())
                P[f'dec{l}.{key}'] = (dst, bias, g + [w])          # (the sources stay alive until the pack has run)
        return P


class LinkNetEngine(_Link, Engine):
    """The 16-bit (fp16 / bf16) LinkNet forward with folded BatchNorm."""

    def __init__(self, dim=2, levels=4, base=32, cin=1, ncls=2, act_dtype=torch.float16, device='cuda'):
        if act_dtype not in (torch.float16, torch.bfloat16):
            raise NotImplementedError("LinkNetEngine runs fp16 / bf16 activations (LinkNetEngineF32: the fp32 form)")
        Engine.__init__(self, dim, levels, base, cin, ncls, act_dtype, device)
        self.use_graph = False
        self._es, self._pack_dtype = 2, act_dtype

    def load_eval(self, params):
        """Fold eval-mode BatchNorm into every conv and pack all operators."""
        if not hasattr(self, '_stage'):
            self._stage = {}
        src = lambda n: self._source(params, n)
        P, descs, keep = {}, [], []
        for prefix in self.enc_names():
            ci, co = self.enc_io(prefix)
            for j, (a, b) in enumerate(((ci, co), (co, co)), 1):
                w = src(f'{prefix}.conv{j}.weight')
                bn = [src(f'{prefix}.bn{j}.{k}') for k in ('weight', 'bias', 'running_mean', 'running_var')]
                keep += [w] + bn
                bias = torch.empty(b, dtype=torch.float32, device=self.device)
                if prefix == 'enc0' and j == 1:
                    dst = torch.empty(nv.lib().iunet_pack_first_conv_elems(b, a, self.taps), dtype=self.act_dtype, device=self.device)
                    descs.append(nv.make_desc(w, dst, b, a, self.taps, 2, self.act_dtype, bn=bn, bias_out=bias, eps=BN_EPS))
                else:
                    dst = nv.PackedConv(b, a, self.taps, self.act_dtype, self.device)
                    descs += dst.descs(w, bn, bias, BN_EPS, None)
                P[f'{prefix}.conv{j}'] = (dst, bias)
        nv.PackTable(descs, self.device, sources=keep).run()
        P.update(self._pack_decoder(src, self.dt))
        P['head'] = (src('head.weight').reshape(self.ncls, self.ch[0]), src('head.bias'))
        self.packed = P

    def workspace(self, N, D, H, W):
        key = (N, D, H, W)
        ws = self._ws_cache.get(key)
        if ws is None:
            self.check_shape(D, H, W)
            dims = self.level_dims(D, H, W)
            ws = {k: torch.empty(n, dtype=self.act_dtype, device=self.device) for k, n in _bufs(self.levels, self.ch, dims, N).items()}
            ws['dims'] = dims
            self._ws_cache = {key: ws}
        return ws

    def infer(self, x, x_strides, N, D, H, W, logits=None, probs=None, cls=None, out_strides=None,
              divisor=1.0, accumulate=False, features_only=False):
        """engine.Engine.infer's contract on the LinkNet graph (features_only: the head's input D^0, NHWC8c, contiguous)."""
        if self.packed is None:
            raise RuntimeError('LinkNetEngine.load_eval() has not been called')
        ws = self.workspace(N, D, H, W)
        dims, L, ch, s = ws['dims'], self.levels, self.ch, nv.stream()
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        for l in range(L):
            v = _vox(dims[l])
            if l == 0:
                w, b = self.packed['enc0.conv1']
                nv.call('iunet_first_conv_fwd', self.dt, self.dim, nv.ptr(x), nv.IN_DTYPE_CODE[x.dtype], nv.ll_array(x_strides),
                        P(ws['a0']), ch[0] * v, nv.ptr(w), nv.ptr(b), None, N, dims[0][0], dims[0][1], dims[0][2], self.cin, ch[0], 1, s)
            else:
                self._conv3(P(ws[f'pin{l}']), ch[l - 1] * v, P(ws[f'a{l}']), ch[l] * v, f'enc{l}.conv1', N, dims[l], ch[l - 1], ch[l], s)
            self._conv3(P(ws[f'a{l}']), ch[l] * v, P(ws[f'x{l}']), ch[l] * v, f'enc{l}.conv2', N, dims[l], ch[l], ch[l], s)
            if l < L - 1:
                do = dims[l + 1]
                nv.call('iunet_maxpool_fwd', self.dt, self.dim, P(ws[f'x{l}']), ch[l] * v, P(ws[f'pin{l + 1}']), ch[l] * _vox(do), ch[l], N,
                        do[0], do[1], do[2], s)
        for l in range(L - 2, -1, -1):
            d, di, v, vi, m = dims[l], dims[l + 1], _vox(dims[l]), _vox(dims[l + 1]), ch[l + 1] // 4
            src = ws[f'x{l + 1}'] if l == L - 2 else ws[f'd{l + 1}']
            self._lk(0, 'conv1', l, P(src), ch[l + 1] * vi, P(ws[f't1{l}']), m * vi, N, di, ch[l + 1], m, s)
            self._lk(1, 'up', l, P(ws[f't1{l}']), m * vi, P(ws[f't2{l}']), m * v, N, di, m, m, s)
            self._lk(0, 'conv2', l, P(ws[f't2{l}']), m * v, P(ws[f'd{l}']), ch[l] * v, N, d, m, ch[l], s, skip=(P(ws[f'x{l}']), ch[l] * v))
        if features_only:
            return ws['d0']
        hw, hb = self.packed['head']
        if out_strides is None:
            v = _vox(dims[0])
            out_strides = (self.ncls * v, v, H * W, W, 1)
        nv.call('iunet_head_fwd', self.dt, P(ws['d0']), ch[0] * _vox(dims[0]), ch[0], nv.ptr(hw), nv.ptr(hb),
                self.ncls, nv.ptr(logits), nv.ptr(probs), nv.ptr(cls), nv.ll_array(out_strides),
                float(divisor), int(bool(accumulate)), N, D, H, W, s)

    def _lk(self, kind, key, l, xp, x_ss, yp, y_ss, N, d, ci, co, s, skip=(None, 0)):
        wpk, bias, _ = self.packed[f'dec{l}.{key}']
        nv.call('iunet_lk_conv_fwd', self.dt, self.dim, kind, xp, x_ss, yp, y_ss, nv.ptr(wpk), None, None, nv.ptr(bias), skip[0], skip[1],
                None, 1, N, d[0], d[1], d[2], ci, co, s)


class LinkNetEngineF32(_Link, EngineF32):
    """The fp32 LinkNet forward (planar fp32 activations, the f32-input matrix instruction): the default prediction form of a LinkNet
    module, within the project's 1e-3 logit promise of the CPU fp32 path."""

    def __init__(self, dim=2, levels=4, base=32, cin=1, ncls=2, device='cuda'):
        EngineF32.__init__(self, dim, levels, base, cin, ncls, device)
        self._es, self._pack_dtype = 4, torch.float32
        self.use_graph = False

    def load_eval(self, params):
        f32 = lambda n: torch.empty(n, dtype=torch.float32, device=self.device)
        src = lambda name: params[name].detach().to(self.device, torch.float32).contiguous()
        lib, s, P = nv.lib(), nv.stream(), {}
        for prefix in self.enc_names():
            ci, co = self.enc_io(prefix)
            for j, (a, b) in enumerate(((ci, co), (co, co)), 1):
                w = src(f'{prefix}.conv{j}.weight')
                bn = [src(f'{prefix}.bn{j}.{k}') for k in ('weight', 'bias', 'running_mean', 'running_var')]
                dst, bias = f32(lib.iunet_f32_pack_conv_elems(b, a, self.taps)), f32(b)
                nv.call('iunet_f32_pack_conv', nv.ptr(w), nv.ptr(dst), nv.ptr(bias), nv.ptr(bn[0]), nv.ptr(bn[1]),
                        nv.ptr(bn[2]), nv.ptr(bn[3]), BN_EPS, b, a, self.taps, 0, s)
                P[f'{prefix}.conv{j}'] = (dst, bias)
        P.update(self._pack_decoder(src, 2))
        P['head'] = (src('head.weight').reshape(self.ncls, self.ch[0]).contiguous(), src('head.bias'))
        torch.cuda.current_stream().synchronize()          # the staging copies above may be freed by the caller
        self.packed = P

    def workspace(self, N, D, H, W):
        key = (N, D, H, W)
        ws = self._ws_cache.get(key)
        if ws is None:
            f = 2 ** (self.levels - 1)
            if H % f or W % f or (self.dim == 3 and D % f) or (self.dim == 2 and D != 1):
                raise ValueError(f'spatial size {(D, H, W)} must be divisible by {f} (and D == 1 in 2-D)')
            dims = self.level_dims(D, H, W)
            ws = {k: torch.empty(n, dtype=torch.float32, device=self.device) for k, n in _bufs(self.levels, self.ch, dims, N).items()}
            ws['dims'] = dims
            self._ws_cache = {key: ws}
        return ws

    def infer(self, x, x_strides, N, D, H, W, logits=None, probs=None, cls=None, out_strides=None,
              divisor=1.0, accumulate=False, features_only=False):
        """engine_f32.EngineF32.infer's contract on the LinkNet graph (features_only: D^0, planar fp32)."""
        if self.packed is None:
            raise RuntimeError('LinkNetEngineF32.load_eval() has not been called')
        ws = self.workspace(N, D, H, W)
        dims, L, ch, s = ws['dims'], self.levels, self.ch, nv.stream()
        P = lambda t: ctypes.c_void_p(t.data_ptr())

        def conv(name, xp, in_dt, strides, yp, y_ss, d, ci, co):
            w, b = self.packed[name]
            nv.call('iunet_f32_conv_fwd', self.dim, xp, in_dt, nv.ll_array(strides), yp, y_ss, nv.ptr(w), nv.ptr(b),
                    N, d[0], d[1], d[2], ci, co, 1, 0, s)

        def lk(kind, name, xp, x_ss, yp, y_ss, d, ci, co, skip=(None, 0)):
            w, b, _ = self.packed[name]
            nv.call('iunet_lk_f32_conv_fwd', self.dim, kind, xp, x_ss, yp, y_ss, nv.ptr(w), nv.ptr(b), skip[0], skip[1],
                    N, d[0], d[1], d[2], ci, co, s)

        planar = lambda ss, d: (ss, _vox(d), d[1] * d[2], d[2], 1)
        for l in range(L):
            d, v = dims[l], _vox(dims[l])
            if l == 0:
                conv('enc0.conv1', nv.ptr(x), nv.IN_DTYPE_CODE[x.dtype], x_strides, P(ws['a0']), ch[0] * v, d, self.cin, ch[0])
            else:
                conv(f'enc{l}.conv1', P(ws[f'pin{l}']), 0, planar(ch[l - 1] * v, d), P(ws[f'a{l}']), ch[l] * v, d, ch[l - 1], ch[l])
            conv(f'enc{l}.conv2', P(ws[f'a{l}']), 0, planar(ch[l] * v, d), P(ws[f'x{l}']), ch[l] * v, d, ch[l], ch[l])
            if l < L - 1:
                do = dims[l + 1]
                nv.call('iunet_f32_maxpool_fwd', self.dim, P(ws[f'x{l}']), ch[l] * v, P(ws[f'pin{l + 1}']), ch[l] * _vox(do), ch[l], N,
                        do[0], do[1], do[2], s)
        for l in range(L - 2, -1, -1):
            d, di, v, vi, m = dims[l], dims[l + 1], _vox(dims[l]), _vox(dims[l + 1]), ch[l + 1] // 4
            src = ws[f'x{l + 1}'] if l == L - 2 else ws[f'd{l + 1}']
            lk(0, f'dec{l}.conv1', P(src), ch[l + 1] * vi, P(ws[f't1{l}']), m * vi, di, ch[l + 1], m)
            lk(1, f'dec{l}.up', P(ws[f't1{l}']), m * vi, P(ws[f't2{l}']), m * v, di, m, m)
            lk(0, f'dec{l}.conv2', P(ws[f't2{l}']), m * v, P(ws[f'd{l}']), ch[l] * v, d, m, ch[l], skip=(P(ws[f'x{l}']), ch[l] * v))
        if features_only:
            return ws['d0']
        hw, hb = self.packed['head']
        if out_strides is None:
            v = _vox(dims[0])
            out_strides = (self.ncls * v, v, H * W, W, 1)
        nv.call('iunet_f32_head_fwd', P(ws['d0']), ch[0] * _vox(dims[0]), ch[0], nv.ptr(hw), nv.ptr(hb), self.ncls,
                nv.ptr(logits), nv.ptr(probs), nv.ptr(cls), nv.ll_array(out_strides), float(divisor),
                int(bool(accumulate)), N, D, H, W, s)
