"""Native 16-bit training step of Segformer (engine_segformer.py has the graph), sequenced from Python on train_engine.TrainEngine's encoder
stage helpers, flat AdamW, loss scaling and device-resident training state.

Forward (csrc/segformer.hip): the collapsed decoder Z = sum_l M_l R_l(X^l) + beta is one gathered GEMM over the encoder outputs with
fuse.bn's statistics rows in its epilogue (the rows include beta: the running mean depends on it); iunet_bn_finalize, iunet_bn_relu_fwd,
the 1x1 head on T and the x4-upsampled loss follow.  The operators M (and M^T for the backward) and beta are re-packed from the fp32
master weights after every update.

Backward: the loss gradient at full resolution and the upsampling's adjoint, the head, fuse.bn's backward giving dZ; then G = dZ R(X)^T
over all levels in one launch, r = the channel sums of dZ, the parameter gradients dW_l = W_f,l^T G_l, dW_f,l = G_l W_l^T + r b_l^T,
db_l = W_f,l^T r in one small launch; U = M^T dZ (iunet_dl_conv_fwd at rate 0 with the transposed operator) and its adjoint resize to every
level's grid, which is the encoder's skip gradient at that level.  The workspace holds no C-channel tensor finer than T and no concat.
"""
import torch

from . import _native as nv
from .engine import BN_EPS
from .engine_segformer import T_LEVEL, sources
from .train_engine import BN_MOMENTUM, TrainEngine, _vox


class SegformerTrainEngine(TrainEngine):
    def __init__(self, model, lr=None, loss_kind='mcc_ce', betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 loss_scale=None, process_group=None):
        if process_group is not None:
            raise NotImplementedError('Segformer training runs on one GPU: a process_group (data parallel training) is not supported')
        if getattr(model, 'norm', 'batch') != 'batch':
            raise NotImplementedError('Segformer training supports BatchNorm only')
        if model.act_dtype not in (torch.float16, torch.bfloat16):
            raise NotImplementedError("Segformer training runs with 16-bit activations (act_dtype 'fp16' / 'bf16')")
        self.C = model.decoder_segmentation_channels
        super().__init__(model, lr=lr, loss_kind=loss_kind, betas=betas, eps=eps, weight_decay=weight_decay, loss_scale=loss_scale)
        self.K = sum(self.ch)
        self.koff = [sum(self.ch[:l]) for l in range(self.levels)]

    # ------------------------------------------------------------------ graph
    def stage_names(self):
        return [f'enc{l}' for l in range(self.levels)]

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
        K = sum(self.ch)
        self.pk['M'] = torch.empty(self.C * K, dtype=self.T, device=self.dev)       # [C][K]
        self.pk['MT'] = torch.empty(K * self.C, dtype=self.T, device=self.dev)      # [K][C]
        self.pk['beta'] = torch.empty(self.C, dtype=torch.float32, device=self.dev)

    def _ops(self, prefix_fn):
        wf = prefix_fn('fuse.conv.weight')
        w = nv.ptr_array([prefix_fn(f'mlp{l}.weight') for l in range(self.levels)])
        b = nv.ptr_array([prefix_fn(f'mlp{l}.bias') for l in range(self.levels)])
        return nv.ptr(wf), w, b

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
        wf, w, b = self._ops(self.p)
        nv.call('iunet_sf_pack', self.dt, self.levels, self.C, nv.int_array(self.ch), wf, w, b, None, None, None, None, 0.0,
                nv.ptr(self.pk['M']), nv.ptr(self.pk['MT']), nv.ptr(self.pk['beta']), nv.stream())

    # ------------------------------------------------------------------ workspace
    def workspace(self, N, D, H, W):
        key = (N, D, H, W)
        ws = self._ws.get(key)
        if ws is not None:
            return ws
        f = 2 ** (self.levels - 1)
        if H % f or W % f or (self.dim == 3 and D % f) or (self.dim == 2 and D != 1):
            raise ValueError(f'spatial size {(D, H, W)} must be divisible by {f}')
        L, ch, lib, C, K = self.levels, self.ch, nv.lib(), self.C, sum(self.ch)
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
            ws[f'x{l}'] = act(ch[l], v)
            ws[f'dskip{l}'] = act(ch[l], v)                  # R_l^T(M_l^T dZ): the skip gradient of level l
            if l > 0:
                ws[f'pin{l}'] = act(ch[l - 1], v)
                ws[f'dpin{l}'] = act(ch[l - 1], v)
        dt, vt = dims[T_LEVEL], _vox(dims[T_LEVEL])
        bn_bufs('fuse', C, vt)
        ws['z'], ws['feat'], ws['dfeat'], ws['dzf'] = act(C, vt), act(C, vt), act(C, vt), act(C, vt)    # Z, F, dF, dZ on T
        ws['u'] = act(K, vt)                                 # M^T dZ on T (K = sum ch channels)
        max_stats = max(max_stats, lib.iunet_sf_stats_parts(N, *dt) * C * 2)
        ws['G'] = f32(C * K)
        ws['gslab'] = f32(lib.iunet_sf_wgrad_slab_floats(N, *dt, K, C))
        ws['rs'] = f32(N * C)
        vf = _vox((D, H, W))
        ws['lc'] = f32(N * self.ncls * vt)
        ws['dlc'] = f32(N * self.ncls * vt)
        ws['dfine'] = f32(N * self.ncls * vf)
        ws['utmp'] = f32(N * self.ncls * D * H * dt[2])
        ws['dy'] = act(max_dy, 1)
        ws['stats'] = f32(max_stats)
        ws['wslab'] = f32(max_wslab)
        ws['bnslab'] = f32(max_bn)
        ws['bncoef'] = f32(3 * max(max(ch), C))
        ws['lslab'] = f32(lib.iunet_dl_up_loss_num_parts(N, vf) * self.ncls * 8)
        ws['hslab'] = f32(lib.iunet_dl_head_bwd_parts(N, vt) * (C // 8 + 1) * 80)
        ws['out4'] = f32(4)
        ws['coef'] = f32(self.ncls * 3)
        self._ws = {key: ws}
        return ws

    # ------------------------------------------------------------------ forward
    def forward_train(self, x, x_strides, N, D, H, W):
        ws = self.workspace(N, D, H, W)
        L, ch, dims, C = self.levels, self.ch, ws['dims'], self.C
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
        dt, vt = dims[T_LEVEL], _vox(dims[T_LEVEL])
        xs, ss, cin, grid = sources(ws, ch, dims, L, self._P)
        nv.call('iunet_sf_gemm', self.dt, self.dim, L, xs, ss, cin, grid, None, None, nv.ptr(self.pk['M']), nv.ptr(self.pk['beta']),
                self._P(ws['z']), C * vt, nv.ptr(ws['stats']), 0, N, dt[0], dt[1], dt[2], C, s)
        nv.call('iunet_bn_finalize', nv.ptr(ws['stats']), nv.lib().iunet_sf_stats_parts(N, *dt), C, float(N * vt),
                nv.ptr(self.p('fuse.bn.weight')), nv.ptr(self.p('fuse.bn.bias')), nv.ptr(self.p('fuse.bn.running_mean')),
                nv.ptr(self.p('fuse.bn.running_var')), BN_MOMENTUM, BN_EPS, nv.ptr(ws['scale.fuse']), nv.ptr(ws['shift.fuse']),
                nv.ptr(ws['mean.fuse']), nv.ptr(ws['invstd.fuse']), s)
        nv.call('iunet_bn_relu_fwd', self.dt, self._P(ws['z']), C * vt, self._P(ws['feat']), C * vt, nv.ptr(ws['scale.fuse']),
                nv.ptr(ws['shift.fuse']), C, N, vt, s)
        nv.call('iunet_head_fwd', self.dt, self._P(ws['feat']), C * vt, C, nv.ptr(self.p('head.weight')), nv.ptr(self.p('head.bias')), self.ncls,
                nv.ptr(ws['lc']), None, None, nv.ll_array((self.ncls * vt, vt, dt[1] * dt[2], dt[2], 1)), 1.0, 0, N, dt[0], dt[1], dt[2], s)
        return ws

    def _up_loss(self, ws, lc, y, w, N):
        tdt = {torch.float32: 0, torch.float16: 1}[y.dtype]
        if w is not None and w.dtype != y.dtype:
            w = w.to(y.dtype)
        dt = ws['dims'][T_LEVEL]
        nv.call('iunet_dl_up_loss_fwd', self.dim, nv.ptr(lc), self.ncls, dt[0], dt[1], dt[2], 4, nv.ptr(y), nv.ptr(w), tdt,
                self.kind, nv.ptr(ws['lslab']), nv.ptr(ws['out4']), nv.ptr(ws['coef']), N, nv.stream())
        return tdt, w

    def train_loss_forward(self, ws, y, w, N, vox):
        return self._up_loss(ws, ws['lc'], y, w, N)

    # ------------------------------------------------------------------ backward
    def backward(self, ws, x, x_strides, y, w, tdt, N):
        L, ch, dims, C, K = self.levels, self.ch, ws['dims'], self.C, self.K
        s = nv.stream()
        dt, vt = dims[T_LEVEL], _vox(dims[T_LEVEL])
        P = self._P
        nv.call('iunet_dl_up_loss_bwd', self.dim, nv.ptr(ws['lc']), self.ncls, dt[0], dt[1], dt[2], 4, nv.ptr(y), nv.ptr(w), tdt,
                nv.ptr(ws['coef']), nv.ptr(self.state), nv.ptr(ws['dfine']), nv.ptr(ws['utmp']), nv.ptr(ws['dlc']), N, s)
        nv.call('iunet_dl_head_bwd', self.dt, P(ws['feat']), C * vt, C, nv.ptr(self.p('head.weight')), nv.ptr(ws['dlc']), self.ncls,
                P(ws['dfeat']), C * vt, nv.ptr(ws['hslab']), nv.ptr(self.g('head.weight')), nv.ptr(self.g('head.bias')), N, vt, s)
        # fuse.bn + ReLU -> dZ
        nv.call('iunet_bn_relu_bwd', self.dt, P(ws['dfeat']), C * vt, None, 0, P(ws['z']), C * vt, P(ws['dzf']), C * vt,
                nv.ptr(ws['mean.fuse']), nv.ptr(ws['invstd.fuse']), nv.ptr(self.p('fuse.bn.weight')), nv.ptr(ws['scale.fuse']),
                nv.ptr(ws['shift.fuse']), nv.ptr(self.g('fuse.bn.weight')), nv.ptr(self.g('fuse.bn.bias')), nv.ptr(ws['bnslab']),
                nv.ptr(ws['bncoef']), C, N, vt, s)
        # G = dZ R(X)^T, r, and the decoder's parameter gradients
        xs, ss, cin, grid = sources(ws, ch, dims, L, P)
        nv.call('iunet_sf_wgrad', self.dt, self.dim, L, xs, ss, cin, grid, None, None, P(ws['dzf']), C * vt, nv.ptr(ws['gslab']),
                nv.ptr(ws['G']), N, dt[0], dt[1], dt[2], C, s)
        nv.call('iunet_dl_chansum', self.dt, P(ws['dzf']), C * vt, nv.ptr(ws['rs']), 1.0, C, N, vt, s)
        wf, w_, b_ = self._ops(self.p)
        nv.call('iunet_sf_param_grads', L, C, nv.int_array(ch), wf, w_, b_, nv.ptr(ws['G']), nv.ptr(ws['rs']), N,
                nv.ptr_array([self.g(f'mlp{l}.weight') for l in range(L)]), nv.ptr_array([self.g(f'mlp{l}.bias') for l in range(L)]),
                nv.ptr(self.g('fuse.conv.weight')), s)
        # U = M^T dZ on T, then its adjoint resize to every level: the encoder's skip gradients
        nv.call('iunet_dl_conv_fwd', self.dt, self.dim, P(ws['dzf']), C * vt, P(ws['u']), K * vt, nv.ptr(self.pk['MT']), C, 1, nv.int_array([0]),
                nv.int_array([0]), nv.int_array([0]), None, None, None, None, 1.0, None, 0, N, dt[0], dt[1], dt[2], C, K, s)
        for l in range(L):
            d = dims[l]
            nv.call('iunet_sf_adjoint', self.dt, self.dim, P(ws['u'], self.koff[l] * vt), K * vt, dt[0], dt[1], dt[2], P(ws[f'dskip{l}']),
                    ch[l] * _vox(d), d[0], d[1], d[2], ch[l], N, s)
        # encoder
        for l in range(L - 1, -1, -1):
            v = _vox(dims[l])
            dz_ptr, dz_ss = P(ws[f'dskip{l}']), ch[l] * v
            pool_bwd = None
            if l < L - 1:
                do = dims[l + 1]
                pool_bwd = (P(ws[f'dpin{l + 1}']), ch[l] * _vox(do), do)
            x2, act, _ = self._conv2_input(ws, f'enc{l}', l, N)
            self._stage_conv_bwd(ws, f'enc{l}.conv2', dz_ptr, dz_ss, None, ch[l] * v, x2, ch[l] * v, ch[l], ch[l], l,
                                 P(ws[f'dz.enc{l}.conv1']), ch[l] * v, N, x_act=act, pool_bwd=pool_bwd, feeds=f'enc{l}.conv1')
            dz1 = P(ws[f'dz.enc{l}.conv1'])
            if l == 0:
                self._stage_conv_bwd(ws, 'enc0.conv1', dz1, ch[0] * v, None, ch[0] * v, None, 0, self.cin, ch[0], 0, None, 0, N,
                                     x_raw=(x, x_strides))
            else:
                self._stage_conv_bwd(ws, f'enc{l}.conv1', dz1, ch[l] * v, None, ch[l] * v, P(ws[f'pin{l}']), ch[l - 1] * v,
                                     ch[l - 1], ch[l], l, P(ws[f'dpin{l}']), ch[l - 1] * v, N)

    # ------------------------------------------------------------------ public steps
    def _handle(self):
        self._steps_seen = getattr(self, '_steps_seen', 0) + 1
        return None               # (no C-sequenced Segformer step: TrainHandle would build the U-Net)

    def _eval_engine(self):
        """The folded-BatchNorm Segformer forward in the training dtype."""
        m = self.model
        if m.infer_dtype == self.T:
            return m.engine('eval')
        if getattr(self, '_eval_eng', None) is None:
            from .engine_segformer import SegformerEngine
            self._eval_eng = SegformerEngine(self.dim, self.levels, m.base, self.cin, self.ncls, self.T, self.dev, decoder_channels=self.C)
        sig = (m._signature(), getattr(self, '_steps_seen', 0))
        if sig != getattr(self, '_eval_sig', None):
            self._eval_eng.load_eval(m.named_tensors())
            self._eval_sig = sig
        return self._eval_eng

    def eval_step(self, X, y, w=None, sync=True):
        """validation_step: eval-mode BatchNorm; the coarse logits of the eval forward, upsampled in the fused loss kernel."""
        self.sync_weights()
        X, y, w, N, D, H, W, vox, xs = self._prep(X, y, w)
        lc = self._eval_engine().coarse_logits(X, xs, N, D, H, W)
        ws = self.workspace(N, D, H, W)
        self._up_loss(ws, lc, y, w, N)
        if not sync:
            return ws['out4']
        o = ws['out4'].tolist()
        return {'Loss': o[0], 'Dice': o[1], 'IoU': o[2], 'MCC': o[3]}
