"""Native 16-bit training step of the LinkNet (engine_linknet.py has the graph), sequenced from Python on train_engine.TrainEngine's
encoder stage helpers, head / loss kernels, flat AdamW, loss scaling and eval_step.

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
from .train_engine import BN_MOMENTUM, TrainEngine, _vox


class LinkNetTrainEngine(TrainEngine):
    def __init__(self, model, lr=None, loss_kind='mcc_ce', betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 loss_scale=None, process_group=None):
        if process_group is not None:
            raise NotImplementedError('LinkNet training runs on one GPU: a process_group (data parallel training) is not supported')
        if getattr(model, 'norm', 'batch') != 'batch':
            raise NotImplementedError('LinkNet training supports BatchNorm only')
        if model.act_dtype not in (torch.float16, torch.bfloat16):
            raise NotImplementedError("LinkNet training runs with 16-bit activations (act_dtype 'fp16' / 'bf16')")
        super().__init__(model, lr=lr, loss_kind=loss_kind, betas=betas, eps=eps, weight_decay=weight_decay, loss_scale=loss_scale)

    # ------------------------------------------------------------------ graph
    def stage_names(self):
        return [f'enc{l}' for l in range(self.levels)]

    def blocks(self):
        """(l, m) of every decoder block in forward order."""
        return [(l, self.ch[l + 1] // 4) for l in range(self.levels - 2, -1, -1)]

    def _ops(self, l, m):
        """(key, forward pack kind, data-gradient pack kind, Cout, Cin) of the three convs of block l."""
        return (('conv1', 0, 1, m, self.ch[l + 1]), ('up', 2, 3, m, m), ('conv2', 0, 1, self.ch[l], m))

    def _alloc_packed(self):
        self.pk = {}
        for prefix in self.stage_names():
            ci, co, _ = self.stage_io(prefix)
            for j, (a, b) in enumerate(((ci, co), (co, co)), 1):
                name = f'{prefix}.conv{j}'
                if name == 'enc0.conv1':
                    self.pk[name] = (torch.empty(nv.lib().iunet_pack_first_conv_elems(b, a, self.taps), dtype=self.T, device=self.dev), None)
                else:
                    self.pk[name] = (nv.PackedConv(b, a, self.taps, self.T, self.dev), nv.PackedConv(b, a, self.taps, self.T, self.dev, dgrad=True))
        lib = nv.lib()
        for l, m in self.blocks():
            for key, kf, kd, co, ci in self._ops(l, m):
                self.pk[f'dec{l}.{key}'] = tuple(torch.empty(lib.iunet_lk_pack_elems(self.dim, k, co, ci), dtype=self.T, device=self.dev)
                                                 for k in (kf, kd))

    def repack(self):
        if getattr(self, '_pack_table', None) is None:
            descs = []
            for prefix in self.stage_names():
                ci, co, _ = self.stage_io(prefix)
                for j, (a, b) in enumerate(((ci, co), (co, co)), 1):
                    name = f'{prefix}.conv{j}'
                    w = self.p(name + '.weight')
                    fwd, dg = self.pk[name]
                    if name == 'enc0.conv1':
                        descs.append(nv.make_desc(w, fwd, b, a, self.taps, 2, self.T))
                    else:
                        descs += fwd.descs(w) + dg.descs(w)
            self._pack_table = nv.PackTable(descs, self.dev, sources=[self.flat])
        self._pack_table.run()
        s = nv.stream()
        for l, m in self.blocks():
            for key, kf, kd, co, ci in self._ops(l, m):
                w = self.p(f'dec{l}.{key}.weight')
                for kind, dst in zip((kf, kd), self.pk[f'dec{l}.{key}']):
                    nv.call('iunet_lk_pack', self.dt, self.dim, kind, nv.ptr(w), None, None, None, None, 0.0, nv.ptr(dst), None, co, ci, s)

    # ------------------------------------------------------------------ workspace
    def workspace(self, N, D, H, W):
        key = (N, D, H, W)
        ws = self._ws.get(key)
        if ws is not None:
            return ws
        f = 2 ** (self.levels - 1)
        if H % f or W % f or (self.dim == 3 and D % f) or (self.dim == 2 and D != 1):
            raise ValueError(f'spatial size {(D, H, W)} must be divisible by {f}')
        L, ch, lib = self.levels, self.ch, nv.lib()
        dims = [((D >> l) if self.dim == 3 else 1, H >> l, W >> l) for l in range(L)]
        act = lambda c, v: torch.empty(N * c * v, dtype=self.T, device=self.dev)
        f32 = lambda n: torch.empty(n, dtype=torch.float32, device=self.dev)
        ws = {'dims': dims}
        max_stats, max_wslab, max_bn, max_dy = 0, 0, 0, 0

        def bn_bufs(name, c, v):
            nonlocal max_bn, max_dy
            for k in ('scale', 'shift', 'mean', 'invstd'):
                ws[f'{k}.{name}'] = f32(c)
            max_bn = max(max_bn, lib.iunet_bn_bwd_num_parts(N, v) * c * 2)
            max_dy = max(max_dy, c * v)
        for l in range(L):
            d, v = dims[l], _vox(dims[l])
            ci = self.cin if l == 0 else ch[l - 1]
            for j, (a, b) in enumerate(((ci, ch[l]), (ch[l], ch[l])), 1):
                name = f'enc{l}.conv{j}'
                ws['y.' + name] = act(b, v)
                if j == 1:
                    ws['z.' + name] = act(b, v)
                    ws['dz.' + name] = act(b, v)
                bn_bufs(name, b, v)
                if name == 'enc0.conv1':
                    max_stats = max(max_stats, lib.iunet_conv3_num_tiles(self.dim, N, *d) * b * 2)
                    max_wslab = max(max_wslab, lib.iunet_first_conv_wgrad_blocks(self.dim, N, *d) * b * 112)
                else:
                    max_stats = max(max_stats, max(lib.iunet_conv3_stats_parts(self.dim, N, *d, b, lay) for lay in (0, 2)) * b * 2)
                    max_wslab = max(max_wslab, lib.iunet_conv3_wgrad_slab_floats(self.dim, N, *d, a, b))
            ws[f'x{l}'] = act(ch[l], v)              # X^l (X^{L-1} = D^{L-1})
            ws[f'dd{l}'] = act(ch[l], v)             # the gradient of D^l (l = L-1: of X^{L-1})
            if l > 0:
                ws[f'pin{l}'] = act(ch[l - 1], v)
                ws[f'dpin{l}'] = act(ch[l - 1], v)
        for l, m in self.blocks():
            d, di, v, vi = dims[l], dims[l + 1], _vox(dims[l]), _vox(dims[l + 1])
            ws[f'y.dec{l}.conv1'] = act(m, vi)
            ws[f'y.dec{l}.up'] = act(m, v)
            ws[f'y.dec{l}.conv2'] = act(ch[l], v)
            ws[f'd{l}'] = act(ch[l], v)
            ws[f'da2.{l}'] = act(m, v)
            ws[f'da1.{l}'] = act(m, vi)
            bn_bufs(f'dec{l}.conv1', m, vi)
            bn_bufs(f'dec{l}.up', m, v)
            bn_bufs(f'dec{l}.conv2', ch[l], v)
            for key, kind, co, ci, g in (('conv1', 0, m, ch[l + 1], di), ('up', 1, m, m, di), ('conv2', 0, ch[l], m, d)):
                max_stats = max(max_stats, lib.iunet_lk_stats_parts(self.dim, kind, N, *g, co) * co * 2)
                max_wslab = max(max_wslab, lib.iunet_lk_wgrad_slab_floats(self.dim, kind, N, *g, ci, co))
        v0 = _vox(dims[0])
        ws['dy'] = act(max_dy, 1)
        ws['stats'] = f32(max_stats)
        ws['wslab'] = f32(max_wslab)
        ws['bnslab'] = f32(max_bn)
        ws['bncoef'] = f32(3 * max(ch))
        ws['lslab'] = f32(lib.iunet_head_loss_num_parts(N, v0) * self.ncls * 8)
        ws['hslab'] = f32(lib.iunet_head_loss_bwd_num_parts(N, v0, self.ncls, ch[0]) * self.ncls * (ch[0] + 1))
        ws['htmp'] = f32(self.ncls * (ch[0] + 1))
        ws['out4'] = f32(4)
        ws['coef'] = f32(self.ncls * 3)
        self._ws = {key: ws}
        return ws

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
        L, ch, dims = self.levels, self.ch, ws['dims']
        s = nv.stream()
        for l in range(L):
            v = _vox(dims[l])
            ci = self.cin if l == 0 else ch[l - 1]
            x2, act, z1p = self._conv2_input(ws, f'enc{l}', l, N)
            if l == 0:
                self._stage_conv_fwd(ws, 'enc0.conv1', None, 0, ci, ch[0], 0, z1p, ch[0] * v, N, x_raw=(x, x_strides))
            else:
                self._stage_conv_fwd(ws, f'enc{l}.conv1', self._P(ws[f'pin{l}']), ci * v, ci, ch[l], l, z1p, ch[l] * v, N)
            pool = None
            if l < L - 1:
                do = dims[l + 1]
                pool = (self._P(ws[f'pin{l + 1}']), ch[l] * _vox(do), do)
            self._stage_conv_fwd(ws, f'enc{l}.conv2', x2, ch[l] * v, ch[l], ch[l], l, self._P(ws[f'x{l}']), ch[l] * v, N, x_act=act, pool=pool)
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
        L, ch, dims = self.levels, self.ch, ws['dims']
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
        for l in range(L - 1, -1, -1):
            v = _vox(dims[l])
            pool_bwd = None
            if l < L - 1:
                do = dims[l + 1]
                pool_bwd = (self._P(ws[f'dpin{l + 1}']), ch[l] * _vox(do), do)      # X^l: the add's gradient dD^l + the max-pool route
            x2, act, _ = self._conv2_input(ws, f'enc{l}', l, N)
            self._stage_conv_bwd(ws, f'enc{l}.conv2', self._P(ws[f'dd{l}']), ch[l] * v, None, ch[l] * v, x2, ch[l] * v, ch[l], ch[l], l,
                                 self._P(ws[f'dz.enc{l}.conv1']), ch[l] * v, N, x_act=act, pool_bwd=pool_bwd, feeds=f'enc{l}.conv1')
            dz1 = self._P(ws[f'dz.enc{l}.conv1'])
            if l == 0:
                self._stage_conv_bwd(ws, 'enc0.conv1', dz1, ch[0] * v, None, ch[0] * v, None, 0, self.cin, ch[0], 0, None, 0, N,
                                     x_raw=(x, x_strides))
            else:
                self._stage_conv_bwd(ws, f'enc{l}.conv1', dz1, ch[l] * v, None, ch[l] * v, self._P(ws[f'pin{l}']), ch[l - 1] * v,
                                     ch[l - 1], ch[l], l, self._P(ws[f'dpin{l}']), ch[l - 1] * v, N)

    # ------------------------------------------------------------------ public steps (TrainEngine.train_step / step_forward / eval_step)
    def _handle(self):
        self._steps_seen = getattr(self, '_steps_seen', 0) + 1
        return None               # (no C-sequenced LinkNet step: TrainHandle would build the U-Net)

    def _eval_engine(self):
        """The folded-BatchNorm LinkNet forward in the training dtype (its features feed the fused head + loss kernel)."""
        m = self.model
        if m.infer_dtype == self.T:
            return m.engine('eval')
        if getattr(self, '_eval_eng', None) is None:
            from .engine_linknet import LinkNetEngine
            self._eval_eng = LinkNetEngine(self.dim, self.levels, m.base, self.cin, self.ncls, self.T, self.dev)
        sig = (m._signature(), getattr(self, '_steps_seen', 0))
        if sig != getattr(self, '_eval_sig', None):
            self._eval_eng.load_eval(m.named_tensors())
            self._eval_sig = sig
        return self._eval_eng
