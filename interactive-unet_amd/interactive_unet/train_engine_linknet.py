"""Native 16-bit training step of the LinkNet (engine_linknet.py has the graph), sequenced from Python on train_engine.EncoderTrainEngine's
encoder and train_engine.TrainEngine's head / loss kernels, flat AdamW, loss scaling and eval_step.

Forward of block l (csrc/linknet.hip): conv1 writes its raw output y1 and BatchNorm partial sums, iunet_bn_finalize turns them into
scale / shift; the transposed conv reads y1 through relu(scale * y1 + shift) in its loads (a1 is never stored), and so does conv2 with
y2 (a2 is never stored); D^l = relu(bn3(y3)) + X^l is one pass (iunet_lk_bn_relu_add).  The head reads D^0.

Backward of block l, from dD^l: the BatchNorm + ReLU backward of bn3 (iunet_bn_relu_bwd, the mask recomputed from y3), conv2's weight
gradient (input a2 = its activation of y2 again) and data gradient, the same for the transposed conv and conv1; conv1's data gradient is
dD^{l+1}.  X^l's gradient has two sources: the add (dD^l) and the max-pool route of the next level's input gradient --
iunet_bn_relu_pool_bwd takes dD^l as its skip gradient.  At the bottom, X^{L-1} = D^{L-1} gets conv1's data gradient of block L-2 only.

There is no C-sequenced handle for LinkNet (iunet_train_create_* builds the U-Net and U-Net++ only): every step runs this sequence.
"""
import torch

from . import _native as nv
from .engine import BN_EPS
from .train_engine import BN_MOMENTUM, EncoderTrainEngine, _vox


class LinkNetTrainEngine(EncoderTrainEngine):
    architecture = 'LinkNet'
    skip_grad = 'dd'              # dd{l}: the gradient of D^l (l = L-1: of X^{L-1})

    # ------------------------------------------------------------------ graph
    def blocks(self):
        """(l, m) of every decoder block in forward order."""
        return [(l, self.ch[l + 1] // 4) for l in range(self.levels - 2, -1, -1)]

    def _ops(self, l, m):
        """(key, forward pack kind, data-gradient pack kind, Cout, Cin) of the three convs of block l."""
        return (('conv1', 0, 1, m, self.ch[l + 1]), ('up', 2, 3, m, m), ('conv2', 0, 1, self.ch[l], m))

    def _alloc_decoder(self):
        lib = nv.lib()
        for l, m in self.blocks():
            for key, kf, kd, co, ci in self._ops(l, m):
                self.pk[f'dec{l}.{key}'] = tuple(torch.empty(lib.iunet_lk_pack_elems(self.dim, k, co, ci), dtype=self.T, device=self.dev)
                                                 for k in (kf, kd))

    def _pack_decoder(self):
        s = nv.stream()
        for l, m in self.blocks():
            for key, kf, kd, co, ci in self._ops(l, m):
                w = self.p(f'dec{l}.{key}.weight')
                for kind, dst in zip((kf, kd), self.pk[f'dec{l}.{key}']):
                    nv.call('iunet_lk_pack', self.dt, self.dim, kind, nv.ptr(w), None, None, None, None, 0.0, nv.ptr(dst), None, co, ci, s)

    # ------------------------------------------------------------------ workspace
    def _decoder_workspace(self, ws, mx, N, D, H, W):
        dims, ch, lib = ws['dims'], self.ch, nv.lib()
        act = lambda c, v: self._act(N, c, v)
        for l, m in self.blocks():
            d, di, v, vi = dims[l], dims[l + 1], _vox(dims[l]), _vox(dims[l + 1])
            ws[f'y.dec{l}.conv1'] = act(m, vi)
            ws[f'y.dec{l}.up'] = act(m, v)
            ws[f'y.dec{l}.conv2'] = act(ch[l], v)
            ws[f'd{l}'] = act(ch[l], v)
            ws[f'da2.{l}'] = act(m, v)
            ws[f'da1.{l}'] = act(m, vi)
            self._bn_bufs(ws, mx, N, f'dec{l}.conv1', m, vi)
            self._bn_bufs(ws, mx, N, f'dec{l}.up', m, v)
            self._bn_bufs(ws, mx, N, f'dec{l}.conv2', ch[l], v)
            for key, kind, co, ci, g in (('conv1', 0, m, ch[l + 1], di), ('up', 1, m, m, di), ('conv2', 0, ch[l], m, d)):
                mx['stats'] = max(mx['stats'], lib.iunet_lk_stats_parts(self.dim, kind, N, *g, co) * co * 2)
                mx['wslab'] = max(mx['wslab'], lib.iunet_lk_wgrad_slab_floats(self.dim, kind, N, *g, ci, co))

    # ------------------------------------------------------------------ forward
    def _lk_fwd(self, ws, l, key, kind, xp, x_ss, act, N, g, ci, co, count):
        """One decoder conv of block l: raw output y.dec{l}.{key} + BatchNorm statistics -> scale / shift of its BatchNorm.  act: name of the
        layer whose raw output x is, its BatchNorm + ReLU applied in the loads."""
        name, bn = f'dec{l}.{key}', f'dec{l}.' + {'conv1': 'bn1', 'up': 'bn2', 'conv2': 'bn3'}[key]
        wf, _ = self.pk[name]
        s = nv.stream()
        y = ws['y.' + name]
        sc, sh = (None, None) if act is None else (nv.ptr(ws['scale.' + act]), nv.ptr(ws['shift.' + act]))
        nv.call('iunet_lk_conv_fwd', self.dt, self.dim, kind, xp, x_ss, self._P(y), y.numel() // N, nv.ptr(wf), sc, sh, None, None, 0,
                nv.ptr(ws['stats']), 0, N, g[0], g[1], g[2], ci, co, s)
        nparts = nv.lib().iunet_lk_stats_parts(self.dim, kind, N, g[0], g[1], g[2], co)
        nv.call('iunet_bn_finalize', nv.ptr(ws['stats']), nparts, co, float(count),
                nv.ptr(self.p(bn + '.weight')), nv.ptr(self.p(bn + '.bias')),
                nv.ptr(self.p(bn + '.running_mean')), nv.ptr(self.p(bn + '.running_var')), BN_MOMENTUM, BN_EPS,
                nv.ptr(ws['scale.' + name]), nv.ptr(ws['shift.' + name]), nv.ptr(ws['mean.' + name]), nv.ptr(ws['invstd.' + name]), s)

    def _block_input(self, ws, l):
        return ws[f'x{self.levels - 1}'] if l == self.levels - 2 else ws[f'd{l + 1}']

    def forward_train(self, x, x_strides, N, D, H, W):
        ws = self.workspace(N, D, H, W)
        self._encoder_forward(ws, x, x_strides, N)
        ch, dims, s = self.ch, ws['dims'], nv.stream()
        for l, m in self.blocks():
            d, di, v, vi = dims[l], dims[l + 1], _vox(dims[l]), _vox(dims[l + 1])
            src = self._block_input(ws, l)
            self._lk_fwd(ws, l, 'conv1', 0, self._P(src), ch[l + 1] * vi, None, N, di, ch[l + 1], m, N * vi)
            self._lk_fwd(ws, l, 'up', 1, self._P(ws[f'y.dec{l}.conv1']), m * vi, f'dec{l}.conv1', N, di, m, m, N * v)
            self._lk_fwd(ws, l, 'conv2', 0, self._P(ws[f'y.dec{l}.up']), m * v, f'dec{l}.up', N, d, m, ch[l], N * v)
            nv.call('iunet_lk_bn_relu_add', self.dt, self._P(ws[f'y.dec{l}.conv2']), ch[l] * v, self._P(ws[f'x{l}']), ch[l] * v,
                    self._P(ws[f'd{l}']), ch[l] * v, nv.ptr(ws[f'scale.dec{l}.conv2']), nv.ptr(ws[f'shift.dec{l}.conv2']), ch[l], N, v, s)
        return ws

    def train_loss_forward(self, ws, y, w, N, vox):
        return self.loss_forward(ws, ws['d0'], y, w, N, vox)

    # ------------------------------------------------------------------ backward
    def _bn_bwd(self, ws, name, bn, dz, c, v, N):
        """BatchNorm + ReLU backward of a decoder conv (the mask recomputed from its raw output): dz -> ws['dy'], dgamma, dbeta."""
        nv.call('iunet_bn_relu_bwd', self.dt, dz, c * v, None, 0, self._P(ws['y.' + name]), c * v, self._P(ws['dy']), c * v,
                nv.ptr(ws['mean.' + name]), nv.ptr(ws['invstd.' + name]), nv.ptr(self.p(bn + '.weight')), nv.ptr(ws['scale.' + name]),
                nv.ptr(ws['shift.' + name]), nv.ptr(self.g(bn + '.weight')), nv.ptr(self.g(bn + '.bias')), nv.ptr(ws['bnslab']),
                nv.ptr(ws['bncoef']), c, N, v, nv.stream())

    def _lk_bwd(self, ws, l, key, kind, xp, x_ss, act, dxp, N, g, ci, co):
        """Weight gradient (input x, through act's BatchNorm + ReLU where given) and data gradient (into dxp) of one decoder conv whose output
        gradient is ws['dy'].  g: the grid of the call (kind 1: the input grid)."""
        name = f'dec{l}.{key}'
        s = nv.stream()
        sc, sh = (None, None) if act is None else (nv.ptr(ws['scale.' + act]), nv.ptr(ws['shift.' + act]))
        vo = _vox(g) * (2 ** self.dim if kind == 1 else 1)
        nv.call('iunet_lk_wgrad', self.dt, self.dim, kind, xp, x_ss, self._P(ws['dy']), co * vo, sc, sh, nv.ptr(ws['wslab']),
                nv.ptr(self.g(name + '.weight')), 1.0, N, g[0], g[1], g[2], ci, co, s)
        _, wd = self.pk[name]
        # data gradient: kind 0 -> the 1x1 conv with the transposed operator; kind 1 -> kind 2 (the strided conv over dy)
        nv.call('iunet_lk_conv_fwd', self.dt, self.dim, 0 if kind == 0 else 2, self._P(ws['dy']), co * vo, dxp, ci * _vox(g), nv.ptr(wd),
                None, None, None, None, 0, None, 0, N, g[0], g[1], g[2], co, ci, s)

    def backward(self, ws, x, x_strides, y, w, tdt, N):
        ch, dims = self.ch, ws['dims']
        s = nv.stream()
        v0 = _vox(dims[0])
        nparts = nv.lib().iunet_head_loss_bwd_num_parts(N, v0, self.ncls, ch[0])
        nv.call('iunet_head_loss_bwd_dev', self.dt, self._P(ws['d0']), ch[0] * v0, ch[0], nv.ptr(self.p('head.weight')),
                nv.ptr(self.p('head.bias')), self.ncls, nv.ptr(y), nv.ptr(w), tdt, nv.ptr(ws['coef']),
                nv.ptr(self.state), self._P(ws['dd0']), ch[0] * v0, nv.ptr(ws['hslab']), None, None, N, v0, s)
        nv.call('iunet_reduce_slab', nv.ptr(ws['hslab']), nparts, self.ncls * (ch[0] + 1), nv.ptr(ws['htmp']), 1.0, 0, s)
        nv.call('iunet_head_grad_scatter', nv.ptr(ws['htmp']), nv.ptr(self.g('head.weight')), nv.ptr(self.g('head.bias')), self.ncls, ch[0], s)
        for l, m in reversed(self.blocks()):
            d, di, v, vi = dims[l], dims[l + 1], _vox(dims[l]), _vox(dims[l + 1])
            self._bn_bwd(ws, f'dec{l}.conv2', f'dec{l}.bn3', self._P(ws[f'dd{l}']), ch[l], v, N)
            self._lk_bwd(ws, l, 'conv2', 0, self._P(ws[f'y.dec{l}.up']), m * v, f'dec{l}.up', self._P(ws[f'da2.{l}']), N, d, m, ch[l])
            self._bn_bwd(ws, f'dec{l}.up', f'dec{l}.bn2', self._P(ws[f'da2.{l}']), m, v, N)
            self._lk_bwd(ws, l, 'up', 1, self._P(ws[f'y.dec{l}.conv1']), m * vi, f'dec{l}.conv1', self._P(ws[f'da1.{l}']), N, di, m, m)
            self._bn_bwd(ws, f'dec{l}.conv1', f'dec{l}.bn1', self._P(ws[f'da1.{l}']), m, vi, N)
            self._lk_bwd(ws, l, 'conv1', 0, self._P(self._block_input(ws, l)), ch[l + 1] * vi, None, self._P(ws[f'dd{l + 1}']), N, di,
                         ch[l + 1], m)
        self._encoder_backward(ws, x, x_strides, N)
