"""Host-side plan of the native DeepLabV3 forward (Chen et al. 2017, smp's DeepLabV3 decoder on this project's encoder): folded eval-mode
BatchNorm, 16-bit (DeepLabV3Engine, on engine.Engine's encoder launches) and fp32 (DeepLabV3EngineF32, on engine_f32.EngineF32's).  Both keep
the `load_eval` / `infer(...)` interface predict.py drives.

Graph.  X = X^{L-1}, the encoder's coarsest output (enc{L-1}; the U-Net's encoder reaches output stride s = 2^(L-1) there, so smp's
dilated encoder stages have no counterpart).  On that grid: the four spatial ASPP branches (b0 1x1, b1..b3 3^d with the atrous rates) write
the four C-channel slots of one buffer, the pooling branch becomes a per-sample bias of the projection (its W_proj[:, 4C:5C] bp[n]), the
projection reads the four slots as one 4C-channel input, then dec.conv and the 1x1 head give the coarse logits; csrc/deeplab.hip upsamples
them x s (align_corners=True) into iunet_head_fwd's output contract (logits / probs / class map, strides, divisor, accumulate).  Eval-mode
dropout is the identity.
"""
import ctypes

import torch

from . import _native as nv
from .engine import BN_EPS, Engine, _vox
from .engine_f32 import EngineF32

BRANCHES = ('aspp.b0', 'aspp.b1', 'aspp.b2', 'aspp.b3')


def _bufs(levels, ch, dims, N, C, ncls):
    """(element counts of the activation workspace, of the fp32 workspace): x{l} / a{l} / pin{l} of the encoder, cat (the 4 branch slots),
    proj (P), feat (F); fp32: lc (coarse logits), xmean, ypool, bp, psb."""
    act = {}
    for l in range(levels):
        v = _vox(dims[l])
        act[f'x{l}'] = N * ch[l] * v
        act[f'a{l}'] = N * ch[l] * v
        if l > 0:
            act[f'pin{l}'] = N * ch[l - 1] * v
    vc = _vox(dims[-1])
    act['cat'] = N * 4 * C * vc
    act['proj'] = N * C * vc
    act['feat'] = N * C * vc
    f32 = {'lc': N * ncls * vc, 'xmean': N * ch[-1], 'ypool': N * C, 'bp': N * C, 'psb': N * C}
    return act, f32


class _DeepLab:
    """What the two DeepLabV3 engines share: names, rates, operator packing, workspace sizes."""

    def _setup(self, decoder_channels, rates):
        self.C = int(decoder_channels)
        self.rates = (0,) + tuple(int(r) for r in rates)         # b0 is the 1x1 branch
        if self.C % 32 or not (32 <= self.C <= 512) or len(self.rates) != 4 or min(self.rates[1:]) <= 0:
            raise NotImplementedError(f'DeepLabV3 engine: decoder_channels {self.C} (a multiple of 32 in 32 .. 512), rates {rates}')
        self.kvol = 3 ** self.dim

    def enc_names(self):
        return [f'enc{l}' for l in range(self.levels)]

    def enc_io(self, prefix):
        l = int(prefix[3:])
        return (self.cin if l == 0 else self.ch[l - 1]), self.ch[l]

    def _graph(self):
        return None          # (no C-sequenced handle for DeepLabV3: every forward is sequenced from Python)

    def bytes_per_slice(self, input_size):
        """Workspace bytes of one 2-D slice of input_size^2 (predict.find_max_batch_size)."""
        S = input_size
        dims = [(1, S >> l, S >> l) for l in range(self.levels)]
        act, f32 = _bufs(self.levels, self.ch, dims, 1, self.C, self.ncls)
        return sum(act.values()) * self._es + sum(f32.values()) * 4

    def _pack_decoder(self, src, dtype_code):
        """Fold every decoder BatchNorm into its conv: {prefix: (operator, bias, row length)}; the projection's operator covers the four
        spatial slots (K = 4C), its pooling columns stay fp32 in the master weight (iunet_dl_pool_psb reads them)."""
        P, C, Cb = {}, self.C, self.ch[-1]
        convs = [(b, 1 if r == 0 else 3, Cb) for b, r in zip(BRANCHES, self.rates)] + [('aspp.project', 1, 5 * C), ('dec', 3, C)]
        for prefix, ksz, cin_tot in convs:
            cin = 4 * C if prefix == 'aspp.project' else cin_tot
            kw = (1 if ksz == 1 else self.kvol) * cin
            w = src(f'{prefix}.conv.weight')
            g = [src(f'{prefix}.bn.{k}') for k in ('weight', 'bias', 'running_mean', 'running_var')]
            dst = torch.empty(C * kw, dtype=self._pack_dtype, device=self.device)
            bias = torch.empty(C, dtype=torch.float32, device=self.device)
            nv.call('iunet_dl_pack', dtype_code, self.dim, 0, ksz, nv.ptr(w), nv.ptr(g[0]), nv.ptr(g[1]), nv.ptr(g[2]), nv.ptr(g[3]), BN_EPS,
                    nv.ptr(dst), nv.ptr(bias), C, cin, cin_tot, 0, 0, kw, nv.stream())
            P[prefix] = (dst, bias, kw, g + [w])               # (the sources stay alive until the pack has run)
        P['pool'] = [src('aspp.pool.conv.weight')] + [src(f'aspp.pool.bn.{k}') for k in ('weight', 'bias', 'running_mean', 'running_var')]
        P['proj_src'] = [src('aspp.project.conv.weight'), src('aspp.project.bn.weight'), src('aspp.project.bn.running_var')]
        P['head'] = (src('head.weight').reshape(self.ncls, C).contiguous(), src('head.bias'))
        return P

    def _pool(self, ws, x_dt, X, N, vc):
        """The pooling branch into ws['psb'] (already x the projection's folded scale)."""
        s, P, C, Cb = nv.stream(), self.packed, self.C, self.ch[-1]
        nv.call('iunet_dl_chansum', x_dt, nv.ptr(X), Cb * vc, nv.ptr(ws['xmean']), 1.0 / vc, Cb, N, vc, s)
        wp, g, b, rm, rv = P['pool']
        nv.call('iunet_dl_pool_gemv', nv.ptr(ws['xmean']), nv.ptr(wp), nv.ptr(ws['ypool']), None, N, Cb, C, s)
        wj, pg, pv = P['proj_src']
        nv.call('iunet_dl_pool_psb', nv.ptr(ws['ypool']), None, None, nv.ptr(g), nv.ptr(b), nv.ptr(rm), nv.ptr(rv), BN_EPS, nv.ptr(ws['bp']),
                nv.ptr(wj), nv.ptr(pg), nv.ptr(pv), nv.ptr(ws['psb']), N, C, s)

    def _upsample(self, ws, N, D, H, W, logits, probs, cls, out_strides, divisor, accumulate):
        dc = ws['dims'][-1]
        s = 2 ** (self.levels - 1)
        if out_strides is None:
            v = D * H * W
            out_strides = (self.ncls * v, v, H * W, W, 1)
        nv.call('iunet_dl_up_head', self.dim, nv.ptr(ws['lc']), self.ncls, dc[0], dc[1], dc[2], s, nv.ptr(logits), nv.ptr(probs), nv.ptr(cls),
                nv.ll_array(out_strides), float(divisor), int(bool(accumulate)), N, nv.stream())


class DeepLabV3Engine(_DeepLab, Engine):
    """The 16-bit (fp16 / bf16) DeepLabV3 forward with folded BatchNorm."""

    def __init__(self, dim=2, levels=4, base=32, cin=1, ncls=2, act_dtype=torch.float16, device='cuda', decoder_channels=256,
                 rates=(12, 24, 36)):
        if act_dtype not in (torch.float16, torch.bfloat16):
            raise NotImplementedError("DeepLabV3Engine runs fp16 / bf16 activations (DeepLabV3EngineF32: the fp32 form)")
        Engine.__init__(self, dim, levels, base, cin, ncls, act_dtype, device)
        self._setup(decoder_channels, rates)
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
        self.packed = P

    def workspace(self, N, D, H, W):
        key = (N, D, H, W)
        ws = self._ws_cache.get(key)
        if ws is None:
            self.check_shape(D, H, W)
            dims = self.level_dims(D, H, W)
            act, f32 = _bufs(self.levels, self.ch, dims, N, self.C, self.ncls)
            ws = {k: torch.empty(n, dtype=self.act_dtype, device=self.device) for k, n in act.items()}
            ws.update({k: torch.empty(n, dtype=torch.float32, device=self.device) for k, n in f32.items()})
            ws['dims'] = dims
            self._ws_cache = {key: ws}
        return ws

    def coarse_logits(self, x, x_strides, N, D, H, W):
        """The forward up to the head: fp32 coarse logits [N][ncls][coarse grid] (the workspace's, overwritten by the next call)."""
        if self.packed is None:
            raise RuntimeError('DeepLabV3Engine.load_eval() has not been called')
        ws = self.workspace(N, D, H, W)
        dims, L, ch, s, C = ws['dims'], self.levels, self.ch, nv.stream(), self.C
        P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off * 2)
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
        dc, vc, Cb, X = dims[-1], _vox(dims[-1]), ch[-1], ws[f'x{L - 1}']
        self._pool(ws, self.dt, X, N, vc)
        for k, (prefix, rate) in enumerate(zip(BRANCHES, self.rates)):
            self._conv(prefix, P(X), Cb * vc, P(ws['cat'], k * C * vc), 4 * C * vc, rate, N, dc, Cb)
        self._conv('aspp.project', P(ws['cat']), 4 * C * vc, P(ws['proj']), C * vc, 0, N, dc, 4 * C, psb=ws['psb'])
        self._conv('dec', P(ws['proj']), C * vc, P(ws['feat']), C * vc, 1, N, dc, C)
        hw, hb = self.packed['head']
        nv.call('iunet_head_fwd', self.dt, P(ws['feat']), C * vc, C, nv.ptr(hw), nv.ptr(hb), self.ncls, nv.ptr(ws['lc']), None, None,
                nv.ll_array((self.ncls * vc, vc, dc[1] * dc[2], dc[2], 1)), 1.0, 0, N, dc[0], dc[1], dc[2], s)
        return ws['lc']

    def infer(self, x, x_strides, N, D, H, W, logits=None, probs=None, cls=None, out_strides=None,
              divisor=1.0, accumulate=False, features_only=False):
        """engine.Engine.infer's contract on the DeepLabV3 graph (features_only: the coarse fp32 logits)."""
        lc = self.coarse_logits(x, x_strides, N, D, H, W)
        if features_only:
            return lc
        self._upsample(self.workspace(N, D, H, W), N, D, H, W, logits, probs, cls, out_strides, divisor, accumulate)

    def _conv(self, prefix, xp, x_ss, yp, y_ss, rate, N, d, ci, psb=None):
        wpk, bias, kw, _ = self.packed[prefix]
        nv.call('iunet_dl_conv_fwd', self.dt, self.dim, xp, x_ss, yp, y_ss, nv.ptr(wpk), kw, 1, nv.int_array([rate]), nv.int_array([0]),
                nv.int_array([0]), None, None, nv.ptr(bias), nv.ptr(psb), 1.0, None, 1, N, d[0], d[1], d[2], ci, self.C, nv.stream())


class DeepLabV3EngineF32(_DeepLab, EngineF32):
    """The fp32 DeepLabV3 forward (planar fp32 activations, the f32-input matrix instruction): the default prediction form of a DeepLabV3
    module, within the project's 1e-3 logit promise of the CPU fp32 path."""

    def __init__(self, dim=2, levels=4, base=32, cin=1, ncls=2, device='cuda', decoder_channels=256, rates=(12, 24, 36)):
        EngineF32.__init__(self, dim, levels, base, cin, ncls, device)
        self._setup(decoder_channels, rates)
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
        self.packed = P
        P.update(self._pack_decoder(src, 2))
        torch.cuda.current_stream().synchronize()          # the staging copies above may be freed by the caller

    def workspace(self, N, D, H, W):
        key = (N, D, H, W)
        ws = self._ws_cache.get(key)
        if ws is None:
            f = 2 ** (self.levels - 1)
            if H % f or W % f or (self.dim == 3 and D % f) or (self.dim == 2 and D != 1):
                raise ValueError(f'spatial size {(D, H, W)} must be divisible by {f} (and D == 1 in 2-D)')
            dims = self.level_dims(D, H, W)
            act, f32 = _bufs(self.levels, self.ch, dims, N, self.C, self.ncls)
            ws = {k: torch.empty(n, dtype=torch.float32, device=self.device) for k, n in {**act, **f32}.items()}
            ws['dims'] = dims
            self._ws_cache = {key: ws}
        return ws

    def coarse_logits(self, x, x_strides, N, D, H, W):
        if self.packed is None:
            raise RuntimeError('DeepLabV3EngineF32.load_eval() has not been called')
        ws = self.workspace(N, D, H, W)
        dims, L, ch, s, C = ws['dims'], self.levels, self.ch, nv.stream(), self.C
        P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off * 4)

        def conv(name, xp, in_dt, strides, yp, y_ss, d, ci, co):
            w, b = self.packed[name]
            nv.call('iunet_f32_conv_fwd', self.dim, xp, in_dt, nv.ll_array(strides), yp, y_ss, nv.ptr(w), nv.ptr(b),
                    N, d[0], d[1], d[2], ci, co, 1, 0, s)

        def dl(prefix, xp, x_ss, yp, y_ss, rate, d, ci, psb=None):
            w, b, kw, _ = self.packed[prefix]
            nv.call('iunet_dl_f32_conv_fwd', self.dim, rate, xp, x_ss, yp, y_ss, nv.ptr(w), kw, nv.ptr(b), nv.ptr(psb), N, d[0], d[1], d[2],
                    ci, C, s)

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
        dc, vc, Cb, X = dims[-1], _vox(dims[-1]), ch[-1], ws[f'x{L - 1}']
        self._pool(ws, 2, X, N, vc)
        for k, (prefix, rate) in enumerate(zip(BRANCHES, self.rates)):
            dl(prefix, P(X), Cb * vc, P(ws['cat'], k * C * vc), 4 * C * vc, rate, dc, Cb)
        dl('aspp.project', P(ws['cat']), 4 * C * vc, P(ws['proj']), C * vc, 0, dc, 4 * C, psb=ws['psb'])
        dl('dec', P(ws['proj']), C * vc, P(ws['feat']), C * vc, 1, dc, C)
        hw, hb = self.packed['head']
        nv.call('iunet_f32_head_fwd', P(ws['feat']), C * vc, C, nv.ptr(hw), nv.ptr(hb), self.ncls, nv.ptr(ws['lc']), None, None,
                nv.ll_array((self.ncls * vc, vc, dc[1] * dc[2], dc[2], 1)), 1.0, 0, N, dc[0], dc[1], dc[2], s)
        return ws['lc']

    def infer(self, x, x_strides, N, D, H, W, logits=None, probs=None, cls=None, out_strides=None,
              divisor=1.0, accumulate=False, features_only=False):
        """engine_f32.EngineF32.infer's contract on the DeepLabV3 graph (features_only: the coarse fp32 logits)."""
        lc = self.coarse_logits(x, x_strides, N, D, H, W)
        if features_only:
            return lc
        self._upsample(self.workspace(N, D, H, W), N, D, H, W, logits, probs, cls, out_strides, divisor, accumulate)
