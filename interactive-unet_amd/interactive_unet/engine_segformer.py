"""Host-side plan of the native Segformer forward (Xie et al. 2021, smp's Segformer decoder on this project's encoder): folded eval-mode
BatchNorm, 16-bit (SegformerEngine, on engine.Engine's encoder launches) and fp32 (SegformerEngineF32, on engine_f32.EngineF32's).  Both keep
the `load_eval` / `infer(...)` interface predict.py drives.

Graph.  The decoder projects every encoder output X^l (mlp{l}), resizes it to the target grid T (the input grid / 4, level 2's grid),
concatenates the L maps deepest first and fuses them (1x1 conv, BatchNorm, ReLU).  All of that up to the BatchNorm is linear, so the engine
runs it as ONE gathered GEMM (csrc/segformer.hip): F = relu(s (sum_l M_l R_l(X^l) + beta - mean) + bn.bias) with M_l = W_f,l W_l folded and
packed once per load_eval, the B operand resampled straight out of the encoder tensors.  The 1x1 head gives the coarse logits on T; the
x4 upsampling (align_corners=True) writes iunet_head_fwd's output contract (logits / probs / class map, strides, divisor, accumulate).
No C-channel tensor finer than T and no L C-channel concat exists: the workspace table is `_bufs`.
"""
import ctypes

import torch

from . import _native as nv
from .engine import BN_EPS, Engine, _vox
from .engine_f32 import EngineF32

T_LEVEL = 2          # the target grid T is level 2's grid (stride 4)


def _bufs(levels, ch, dims, N, C, ncls):
    """(element counts of the activation workspace, of the fp32 workspace): x{l} / a{l} / pin{l} of the encoder, feat (F on T);
    fp32: lc (coarse logits on T)."""
    act = {}
    for l in range(levels):
        v = _vox(dims[l])
        act[f'x{l}'] = N * ch[l] * v
        act[f'a{l}'] = N * ch[l] * v
        if l > 0:
            act[f'pin{l}'] = N * ch[l - 1] * v
    vt = _vox(dims[T_LEVEL])
    act['feat'] = N * C * vt
    f32 = {'lc': N * ncls * vt}
    return act, f32


def sources(ws, ch, dims, levels, P):
    """The gather GEMM's source table over the encoder outputs x{l}: (pointers, sample strides, channels, grids)."""
    xs = nv.ptr_array([P(ws[f'x{l}']).value for l in range(levels)])
    ss = nv.ll_array([ch[l] * _vox(dims[l]) for l in range(levels)])
    cin = nv.int_array(ch[:levels])
    grid = nv.int_array([e for l in range(levels) for e in dims[l]])
    return xs, ss, cin, grid


def pack_args(src, levels):
    """(ch array, fuse weight, mlp weight array, mlp bias array, kept sources) of iunet_sf_pack / iunet_sf_param_grads."""
    wf = src('fuse.conv.weight')
    w = [src(f'mlp{l}.weight') for l in range(levels)]
    b = [src(f'mlp{l}.bias') for l in range(levels)]
    return nv.ptr(wf), nv.ptr_array(w), nv.ptr_array(b), [wf] + w + b


class _Segformer:
    """What the two Segformer engines share: names, operator packing, workspace sizes."""

    def _setup(self, decoder_channels):
        self.C = int(decoder_channels)
        if self.C % 32 or not (32 <= self.C <= 512) or not (3 <= self.levels <= 6):
            raise NotImplementedError(f'Segformer engine: decoder_channels {self.C} (a multiple of 32 in 32 .. 512), {self.levels} levels '
                                      f'(3 .. 6)')
        self.K = sum(self.ch)

    def enc_names(self):
        return [f'enc{l}' for l in range(self.levels)]

    def enc_io(self, prefix):
        l = int(prefix[3:])
        return (self.cin if l == 0 else self.ch[l - 1]), self.ch[l]

    def _graph(self):
        return None          # (no C-sequenced handle for Segformer: every forward is sequenced from Python)

    def bytes_per_slice(self, input_size):
        """Workspace bytes of one 2-D slice of input_size^2 (predict.find_max_batch_size)."""
        S = input_size
        dims = [(1, S >> l, S >> l) for l in range(self.levels)]
        act, f32 = _bufs(self.levels, self.ch, dims, 1, self.C, self.ncls)
        return sum(act.values()) * self._es + sum(f32.values()) * 4

    def _pack_decoder(self, src, dtype_code):
        """The collapsed decoder operator with fuse.bn folded: (operator [C][K], bias [C], kept sources)."""
        wf, w, b, keep = pack_args(src, self.levels)
        g = [src(f'fuse.bn.{k}') for k in ('weight', 'bias', 'running_mean', 'running_var')]
        dst = torch.empty(self.C * self.K, dtype=self._pack_dtype, device=self.device)
        bias = torch.empty(self.C, dtype=torch.float32, device=self.device)
        nv.call('iunet_sf_pack', dtype_code, self.levels, self.C, nv.int_array(self.ch), wf, w, b, nv.ptr(g[0]), nv.ptr(g[1]), nv.ptr(g[2]),
                nv.ptr(g[3]), BN_EPS, nv.ptr(dst), None, nv.ptr(bias), nv.stream())
        head = (src('head.weight').reshape(self.ncls, self.C).contiguous(), src('head.bias'))
        return {'sf': (dst, bias, keep + g), 'head': head}

    def _decode(self, ws, dtype_code, N, P):
        dims, C = ws['dims'], self.C
        dt = dims[T_LEVEL]
        xs, ss, cin, grid = sources(ws, self.ch, dims, self.levels, P)
        w, bias, _ = self.packed['sf']
        nv.call('iunet_sf_gemm', dtype_code, self.dim, self.levels, xs, ss, cin, grid, None, None, nv.ptr(w), nv.ptr(bias), P(ws['feat']),
                C * _vox(dt), None, 1, N, dt[0], dt[1], dt[2], C, nv.stream())

    def _upsample(self, ws, N, D, H, W, logits, probs, cls, out_strides, divisor, accumulate):
        dc = ws['dims'][T_LEVEL]
        if out_strides is None:
            v = D * H * W
            out_strides = (self.ncls * v, v, H * W, W, 1)
        nv.call('iunet_dl_up_head', self.dim, nv.ptr(ws['lc']), self.ncls, dc[0], dc[1], dc[2], 4, nv.ptr(logits), nv.ptr(probs), nv.ptr(cls),
                nv.ll_array(out_strides), float(divisor), int(bool(accumulate)), N, nv.stream())

    def infer(self, x, x_strides, N, D, H, W, logits=None, probs=None, cls=None, out_strides=None,
              divisor=1.0, accumulate=False, features_only=False):
        """engine.Engine.infer's contract on the Segformer graph (features_only: the coarse fp32 logits on T)."""
        lc = self.coarse_logits(x, x_strides, N, D, H, W)
        if features_only:
            return lc
        self._upsample(self.workspace(N, D, H, W), N, D, H, W, logits, probs, cls, out_strides, divisor, accumulate)


class SegformerEngine(_Segformer, Engine):
    """The 16-bit (fp16 / bf16) Segformer forward with folded BatchNorm."""

    def __init__(self, dim=2, levels=4, base=32, cin=1, ncls=2, act_dtype=torch.float16, device='cuda', decoder_channels=256):
        if act_dtype not in (torch.float16, torch.bfloat16):
            raise NotImplementedError("SegformerEngine runs fp16 / bf16 activations (SegformerEngineF32: the fp32 form)")
        Engine.__init__(self, dim, levels, base, cin, ncls, act_dtype, device)
        self._setup(decoder_channels)
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
        """The forward up to the head: fp32 coarse logits [N][ncls][T] (the workspace's, overwritten by the next call)."""
        if self.packed is None:
            raise RuntimeError('SegformerEngine.load_eval() has not been called')
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
        self._decode(ws, self.dt, N, P)
        dc, vc = dims[T_LEVEL], _vox(dims[T_LEVEL])
        hw, hb = self.packed['head']
        nv.call('iunet_head_fwd', self.dt, P(ws['feat']), C * vc, C, nv.ptr(hw), nv.ptr(hb), self.ncls, nv.ptr(ws['lc']), None, None,
                nv.ll_array((self.ncls * vc, vc, dc[1] * dc[2], dc[2], 1)), 1.0, 0, N, dc[0], dc[1], dc[2], s)
        return ws['lc']


class SegformerEngineF32(_Segformer, EngineF32):
    """The fp32 Segformer forward (planar fp32 activations, the f32-input matrix instruction): the default prediction form of a Segformer
    module, within the project's 1e-3 logit promise of the CPU fp32 path."""

    def __init__(self, dim=2, levels=4, base=32, cin=1, ncls=2, device='cuda', decoder_channels=256):
        EngineF32.__init__(self, dim, levels, base, cin, ncls, device)
        self._setup(decoder_channels)
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
            raise RuntimeError('SegformerEngineF32.load_eval() has not been called')
        ws = self.workspace(N, D, H, W)
        dims, L, ch, s, C = ws['dims'], self.levels, self.ch, nv.stream(), self.C
        P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off * 4)

        def conv(name, xp, in_dt, strides, yp, y_ss, d, ci, co):
            w, b = self.packed[name]
            nv.call('iunet_f32_conv_fwd', self.dim, xp, in_dt, nv.ll_array(strides), yp, y_ss, nv.ptr(w), nv.ptr(b),
                    N, d[0], d[1], d[2], ci, co, 1, 0, s)

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
        self._decode(ws, 2, N, P)
        dc, vc = dims[T_LEVEL], _vox(dims[T_LEVEL])
        hw, hb = self.packed['head']
        nv.call('iunet_f32_head_fwd', P(ws['feat']), C * vc, C, nv.ptr(hw), nv.ptr(hb), self.ncls, nv.ptr(ws['lc']), None, None,
                nv.ll_array((self.ncls * vc, vc, dc[1] * dc[2], dc[2], 1)), 1.0, 0, N, dc[0], dc[1], dc[2], s)
        return ws['lc']
