"""Host-side plan of the native U-Net++ forward (Zhou et al. 2018, the canonical nested form on this project's stage):
folded eval-mode BatchNorm, 16-bit (NestedEngine, on engine.Engine's conv / convT / pool / head launches) and fp32 (NestedEngineF32,
on engine_f32.EngineF32's).  Both keep the `load_eval` / `infer(...)` interface predict.py drives.

Graph.  X^{i,0} is the encoder (enc{i}); for j >= 1 and i + j <= L - 1, X^{i,j} = stage(concat[X^{i,0}, .., X^{i,j-1}, up(X^{i+1,j-1})])
(dec{i}_{j}); the head reads X^{0,L-1}.  Nodes run column by column (unet.nested_nodes).

Layout.  One buffer per level i with L - i channel-blocked slots of ch[i] channels, [X^{i,0} | X^{i,1} | ..] per sample: the
transposed conv of node (i, j) writes up(X^{i+1,j-1}) into slot j, conv1 reads slots 0..j as one (j + 1) ch[i]-channel input (the
concat is free: consecutive channel planes), and conv2's output overwrites slot j -- up(.) has no reader after conv1.  X^{0,L-1}
goes to a buffer of its own, the head's input.  The 16-bit forward runs as one C call from its second forward on the same weights
(net_graph.NetGraph over iunet_net_create_nested: the same launches sequenced in C++, bit-identical); the fp32 form is sequenced from
Python.
"""
import ctypes

import torch

from . import _native as nv
from . import topology
from .engine import BN_EPS, Engine, _vox
from .engine_f32 import EngineF32
from .unet import nested_nodes


def _level_bufs(levels, ch, dims, N, es):
    """Element counts of the forward workspace: lv{i} (L - i slots), a{i} (conv1 output), pin{i} (pooled input), b0 (head input)."""
    out = {}
    for i in range(levels):
        v = _vox(dims[i])
        out[f'lv{i}'] = N * (levels - i) * ch[i] * v
        out[f'a{i}'] = N * ch[i] * v
        if i > 0:
            out[f'pin{i}'] = N * ch[i - 1] * v
    out['b0'] = N * ch[0] * _vox(dims[0])
    return out


class _Nested:
    """What the two nested engines share: names, shapes, workspace sizes."""
    workspaces_kept = 1

    def stage_names(self):
        return topology.nested_stage_names(self.levels)

    def _build_workspace(self, N, dims):
        ws = {k: torch.empty(n, dtype=self.act_dtype, device=self.device) for k, n in _level_bufs(self.levels, self.ch, dims, N, 0).items()}
        ws['dims'] = dims
        return ws

    def bytes_per_slice(self, input_size):
        """Workspace bytes of one 2-D slice of input_size^2 (predict.find_max_batch_size)."""
        S = input_size
        dims = [(1, S >> l, S >> l) for l in range(self.levels)]
        return sum(_level_bufs(self.levels, self.ch, dims, 1, 0).values()) * self._es

    def _slot(self, ws, i, j, dims):
        """(pointer, sample stride) of slot j of level i."""
        v = _vox(dims[i])
        t = ws[f'lv{i}']
        return ctypes.c_void_p(t.data_ptr() + j * self.ch[i] * v * t.element_size()), (self.levels - i) * self.ch[i] * v


class NestedEngine(_Nested, Engine):
    """The 16-bit (fp16 / bf16) U-Net++ forward with folded BatchNorm."""

    def __init__(self, dim=2, levels=4, base=32, cin=1, ncls=2, act_dtype=torch.float16, device='cuda'):
        if act_dtype not in (torch.float16, torch.bfloat16):
            raise NotImplementedError("NestedEngine runs fp16 / bf16 activations (NestedEngineF32: the fp32 form)")
        Engine.__init__(self, dim, levels, base, cin, ncls, act_dtype, device)
        self.nodes = nested_nodes(self.levels)
        self._es = 2

    def _graph_spec(self):
        """The nested handle (iunet_net_create_nested), at every level count the module allows."""
        return dict(mode=self.dt, nested=True)

    def load_eval(self, params):
        """Fold eval-mode BatchNorm into every stage conv and pack all operators (one launch over a descriptor table, rebuilt when a
        source tensor moves), as Engine.load_eval does for the U-Net."""
        self._new_params(params)
        src, sig = self._sources(params, topology.param_names(self.stage_names(), topology.nested_up_convs(self.levels)))
        if sig != self._eval_sig:
            P, descs = {}, []
            for prefix in self.stage_names():
                ci, co = self.stage_io(prefix)
                for j, (a, b) in enumerate(((ci, co), (co, co)), 1):
                    w = src[f'{prefix}.conv{j}.weight']
                    bn = [src[f'{prefix}.bn{j}.{k}'] for k in topology.BN_KEYS]
                    bias = torch.empty(b, dtype=torch.float32, device=self.device)
                    if prefix == 'enc0' and j == 1:
                        dst = torch.empty(nv.lib().iunet_pack_first_conv_elems(b, a, self.taps), dtype=self.act_dtype, device=self.device)
                        descs.append(nv.make_desc(w, dst, b, a, self.taps, 2, self.act_dtype, bn=bn, bias_out=bias, eps=BN_EPS))
                    else:
                        dst = nv.PackedConv(b, a, self.taps, self.act_dtype, self.device)
                        descs += dst.descs(w, bn, bias, BN_EPS, None)
                    P[f'{prefix}.conv{j}'] = (dst, bias)
            for i, j in self.nodes:
                w = src[f'dec{i}_{j}.up.weight']
                dst = torch.empty(w.numel(), dtype=self.act_dtype, device=self.device)
                descs.append(nv.make_desc(w, dst, self.ch[i], self.ch[i + 1], self.npos, 3, self.act_dtype))
                P[f'dec{i}_{j}.up'] = (dst, src[f'dec{i}_{j}.up.bias'])
            P['head'] = (src['head.weight'].reshape(self.ncls, self.ch[0]), src['head.bias'])
            self._eval_table = nv.PackTable(descs, self.device, sources=list(src.values()))
            self._eval_sig = sig
            self.packed = P
        self._eval_table.run()

    def infer(self, x, x_strides, N, D, H, W, logits=None, probs=None, cls=None, out_strides=None,
              divisor=1.0, accumulate=False, features_only=False):
        """engine.Engine.infer's contract on the nested graph (features_only: the head's input X^{0,L-1}, NHWC8c, contiguous)."""
        self._require_loaded()
        g = self._graph()
        if g is not None and not features_only and self.probe is None:
            self.check_shape(D, H, W)
            return g.infer(x, x_strides, N, D, H, W, logits, probs, cls, out_strides, divisor, accumulate)
        ws = self.workspace(N, D, H, W)
        dims, L, ch, s = ws['dims'], self.levels, self.ch, nv.stream()
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        for l in range(L):
            v = _vox(dims[l])
            x0, x0_ss = self._slot(ws, l, 0, dims)
            if l == 0:
                w, b = self.packed['enc0.conv1']
                nv.call('iunet_first_conv_fwd', self.dt, self.dim, nv.ptr(x), nv.IN_DTYPE_CODE[x.dtype], nv.ll_array(x_strides),
                        P(ws['a0']), ch[0] * v, nv.ptr(w), nv.ptr(b), None, N, dims[0][0], dims[0][1], dims[0][2], self.cin, ch[0], 1, s)
            else:
                self._conv3(P(ws[f'pin{l}']), ch[l - 1] * v, P(ws[f'a{l}']), ch[l] * v, f'enc{l}.conv1', N, dims[l], ch[l - 1], ch[l], s)
            self._conv3(P(ws[f'a{l}']), ch[l] * v, x0, x0_ss, f'enc{l}.conv2', N, dims[l], ch[l], ch[l], s)
            if l < L - 1:
                do = dims[l + 1]
                nv.call('iunet_maxpool_fwd', self.dt, self.dim, x0, x0_ss, P(ws[f'pin{l + 1}']), ch[l] * _vox(do), ch[l], N,
                        do[0], do[1], do[2], s)
        for i, j in self.nodes:
            v, di = _vox(dims[i]), dims[i + 1]
            node = f'dec{i}_{j}'
            src, src_ss = self._slot(ws, i + 1, j - 1, dims)
            cat, cat_ss = self._slot(ws, i, 0, dims)
            up, _ = self._slot(ws, i, j, dims)
            wpk, bias = self.packed[node + '.up']
            nv.call('iunet_convT_fwd', self.dt, self.dim, src, src_ss, up, cat_ss, nv.ptr(wpk), nv.ptr(bias),
                    N, di[0], di[1], di[2], ch[i + 1], ch[i], s)
            self._conv3(cat, cat_ss, P(ws[f'a{i}']), ch[i] * v, node + '.conv1', N, dims[i], (j + 1) * ch[i], ch[i], s)
            out, out_ss = (P(ws['b0']), ch[0] * v) if (i, j) == (0, L - 1) else (up, cat_ss)
            self._conv3(P(ws[f'a{i}']), ch[i] * v, out, out_ss, node + '.conv2', N, dims[i], ch[i], ch[i], s)
        if features_only:
            return ws['b0']
        hw, hb = self.packed['head']
        nv.call('iunet_head_fwd', self.dt, P(ws['b0']), ch[0] * _vox(dims[0]), ch[0], nv.ptr(hw), nv.ptr(hb),
                self.ncls, nv.ptr(logits), nv.ptr(probs), nv.ptr(cls), nv.ll_array(self._out_strides(out_strides, D, H, W)),
                float(divisor), int(bool(accumulate)), N, D, H, W, s)


class NestedEngineF32(_Nested, EngineF32):
    """The fp32 U-Net++ forward (planar fp32 activations, the f32-input matrix instruction): the default prediction form of a
    U-Net++ module, within the project's 1e-3 logit promise of the CPU fp32 path."""

    def __init__(self, dim=2, levels=4, base=32, cin=1, ncls=2, device='cuda'):
        EngineF32.__init__(self, dim, levels, base, cin, ncls, device)
        self.nodes = nested_nodes(self.levels)
        self._es = 4

    def load_eval(self, params):
        f32 = lambda n: torch.empty(n, dtype=torch.float32, device=self.device)
        src = lambda name: params[name].detach().to(self.device, torch.float32).contiguous()
        lib, s, P = nv.lib(), nv.stream(), {}
        for prefix in self.stage_names():
            ci, co = self.stage_io(prefix)
            for j, (a, b) in enumerate(((ci, co), (co, co)), 1):
                w = src(f'{prefix}.conv{j}.weight')
                bn = [src(f'{prefix}.bn{j}.{k}') for k in topology.BN_KEYS]
                dst, bias = f32(lib.iunet_f32_pack_conv_elems(b, a, self.taps)), f32(b)
                nv.call('iunet_f32_pack_conv', nv.ptr(w), nv.ptr(dst), nv.ptr(bias), nv.ptr(bn[0]), nv.ptr(bn[1]),
                        nv.ptr(bn[2]), nv.ptr(bn[3]), BN_EPS, b, a, self.taps, 0, s)
                P[f'{prefix}.conv{j}'] = (dst, bias)
        for i, j in self.nodes:
            w = src(f'dec{i}_{j}.up.weight')
            dst = f32(lib.iunet_f32_pack_conv_elems(self.ch[i], self.ch[i + 1], self.npos))
            nv.call('iunet_f32_pack_conv', nv.ptr(w), nv.ptr(dst), None, None, None, None, None, BN_EPS,
                    self.ch[i], self.ch[i + 1], self.npos, 1, s)
            P[f'dec{i}_{j}.up'] = (dst, src(f'dec{i}_{j}.up.bias'))
        P['head'] = (src('head.weight').reshape(self.ncls, self.ch[0]).contiguous(), src('head.bias'))
        torch.cuda.current_stream().synchronize()          # the staging copies above may be freed by the caller
        self.packed = P

    def infer(self, x, x_strides, N, D, H, W, logits=None, probs=None, cls=None, out_strides=None,
              divisor=1.0, accumulate=False, features_only=False):
        """engine_f32.EngineF32.infer's contract on the nested graph (features_only: X^{0,L-1}, planar fp32)."""
        self._require_loaded()
        ws = self.workspace(N, D, H, W)
        dims, L, ch, s = ws['dims'], self.levels, self.ch, nv.stream()
        P = lambda t: ctypes.c_void_p(t.data_ptr())

        def conv(name, xp, in_dt, strides, yp, y_ss, d, ci, co, transposed=0, relu=1):
            w, b = self.packed[name]
            nv.call('iunet_f32_conv_fwd', self.dim, xp, in_dt, nv.ll_array(strides), yp, y_ss, nv.ptr(w), nv.ptr(b),
                    N, d[0], d[1], d[2], ci, co, relu, transposed, s)

        planar = lambda ss, d: (ss, _vox(d), d[1] * d[2], d[2], 1)
        for l in range(L):
            d, v = dims[l], _vox(dims[l])
            x0, x0_ss = self._slot(ws, l, 0, dims)
            if l == 0:
                conv('enc0.conv1', nv.ptr(x), nv.IN_DTYPE_CODE[x.dtype], x_strides, P(ws['a0']), ch[0] * v, d, self.cin, ch[0])
            else:
                conv(f'enc{l}.conv1', P(ws[f'pin{l}']), 0, planar(ch[l - 1] * v, d), P(ws[f'a{l}']), ch[l] * v, d, ch[l - 1], ch[l])
            conv(f'enc{l}.conv2', P(ws[f'a{l}']), 0, planar(ch[l] * v, d), x0, x0_ss, d, ch[l], ch[l])
            if l < L - 1:
                do = dims[l + 1]
                nv.call('iunet_f32_maxpool_fwd', self.dim, x0, x0_ss, P(ws[f'pin{l + 1}']), ch[l] * _vox(do), ch[l], N,
                        do[0], do[1], do[2], s)
        for i, j in self.nodes:
            d, v, di = dims[i], _vox(dims[i]), dims[i + 1]
            node = f'dec{i}_{j}'
            src, src_ss = self._slot(ws, i + 1, j - 1, dims)
            cat, cat_ss = self._slot(ws, i, 0, dims)
            up, _ = self._slot(ws, i, j, dims)
            conv(node + '.up', src, 0, planar(src_ss, di), up, cat_ss, di, ch[i + 1], ch[i], transposed=1, relu=0)
            conv(node + '.conv1', cat, 0, planar(cat_ss, d), P(ws[f'a{i}']), ch[i] * v, d, (j + 1) * ch[i], ch[i])
            out, out_ss = (P(ws['b0']), ch[0] * v) if (i, j) == (0, L - 1) else (up, cat_ss)
            conv(node + '.conv2', P(ws[f'a{i}']), 0, planar(ch[i] * v, d), out, out_ss, d, ch[i], ch[i])
        if features_only:
            return ws['b0']
        hw, hb = self.packed['head']
        nv.call('iunet_f32_head_fwd', P(ws['b0']), ch[0] * _vox(dims[0]), ch[0], nv.ptr(hw), nv.ptr(hb), self.ncls,
                nv.ptr(logits), nv.ptr(probs), nv.ptr(cls), nv.ll_array(self._out_strides(out_strides, D, H, W)), float(divisor),
                int(bool(accumulate)), N, D, H, W, s)
