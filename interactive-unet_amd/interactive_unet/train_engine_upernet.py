"""Native 16-bit training step of UPerNet (engine_upernet.py has the graph), sequenced from Python on train_engine.EncoderTrainEngine's encoder
and train_engine.CoarseTrainEngine's coarse-logit loss (coarse level 2), flat AdamW, loss scaling and device-resident training state.

Forward.  iunet_pn_pool gives A_s (one launch); each branch conv (iunet_dl_conv_fwd at rate 0 on the s^d grid) writes its RAW output and
BatchNorm partial sums, and iunet_pn_resize applies relu(scale y + shift) in its loads while it resamples the branch into its slot of U --
psp.b1 has no norm: its prologue is relu(1 y + bias).  psp.out (3^d over U) and fuse (3^d over V) are followed by iunet_bn_relu_fwd.  A
lateral's raw output is the resize kernel's raw base: P^l = relu(scale y + shift) + R(P^{l+1}) in one pass, so neither the branches' nor
the laterals' activations are stored.  P^2 lives in V's last slot.

Backward.  The loss gradient and the head through CoarseTrainEngine, then fuse; V's gradient slots are dP^l's share from the fuse conv:
top-down from level 2, each lateral (BatchNorm backward, weight gradient, data gradient = X^l's skip gradient), then
dP^{l+1} = R^T(dV slot) + R^T(dP^l) (iunet_pn_resize_adjoint, the second call accumulating).  psp.out gives dU; its branch slots go back
through R^T, the branch BatchNorms (psp.b1: iunet_pn_bias_relu_bwd) and convs to dA_s; iunet_pn_pool_bwd sums the identity slot's gradient
and pool_s^T(dA_s) into X^B's skip gradient.  Levels 0 and 1 receive gradient through the max-pool only (their skip input is a zero plane).
"""
import torch

from . import _native as nv
from .engine import BN_EPS
from .engine_upernet import POOL_SIZES, T_LEVEL, branch, check_setup, conv_table, laterals, pool_dims
from .train_engine import BN_MOMENTUM, CoarseTrainEngine, _vox


class UPerNetTrainEngine(CoarseTrainEngine):
    architecture = 'UPerNet'
    coarse_level = T_LEVEL

    def __init__(self, model, lr=None, loss_kind='mcc_ce', betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 loss_scale=None, process_group=None):
        self.C = model.decoder_channels
        check_setup('UPerNet training', self.C, model.levels)
        super().__init__(model, lr=lr, loss_kind=loss_kind, betas=betas, eps=eps, weight_decay=weight_decay, loss_scale=loss_scale,
                         process_group=process_group)

    # ------------------------------------------------------------------ graph
    def _convs(self):
        return conv_table(self.dim, self.levels, self.ch, self.C)

    def _alloc_decoder(self):
        kv = 3 ** self.dim
        self.kvol = kv
        for prefix, ksz, ci, co in self._convs():
            n = co * ci * (1 if ksz == 1 else kv)
            self.pk[prefix] = torch.empty(n, dtype=self.T, device=self.dev)            # forward [co][k ci]
            self.pk['dg.' + prefix] = torch.empty(n, dtype=self.T, device=self.dev)    # data gradient [ci][k co]
        self.ones = torch.ones(self.ch[-1] // 4, dtype=torch.float32, device=self.dev)  # psp.b1's prologue scale

    def _pack_decoder(self):
        for prefix, ksz, ci, co in self._convs():
            kk = 1 if ksz == 1 else self.kvol
            for mode, dst, ld in ((0, self.pk[prefix], kk * ci), (1, self.pk['dg.' + prefix], kk * co)):
                nv.call('iunet_dl_pack', self.dt, self.dim, mode, ksz, nv.ptr(self.p(prefix + '.conv.weight')), None, None, None, None, 0.0,
                        nv.ptr(dst), None, co, ci, ci, 0, 0, ld, nv.stream())

    # ------------------------------------------------------------------ workspace
    def _grids(self, dims):
        """{prefix: (grid, rate)} of every decoder conv."""
        L = self.levels
        g = {branch(s): (pool_dims(self.dim, s), 0) for s in POOL_SIZES}
        g['psp.out'] = (dims[-1], 1)
        g.update({f'lat{l}': (dims[l], 0) for l in laterals(L)})
        g['fuse'] = (dims[T_LEVEL], 1)
        return g

    def _decoder_workspace(self, ws, mx, N, D, H, W):
        dims, ch, lib, C, L = ws['dims'], self.ch, nv.lib(), self.C, self.levels
        act = lambda c, v: self._act(N, c, v)
        B, Cb, Cq, vb, vt = L - 1, ch[-1], ch[-1] // 4, _vox(dims[-1]), _vox(dims[T_LEVEL])
        grids = self._grids(dims)
        ws['zeros'] = act(max([ch[l] * _vox(dims[l]) for l in range(T_LEVEL)] + [8]), 1).zero_()   # the skip gradient of levels 0 and 1
        for l in range(T_LEVEL, L):
            ws[f'dskip{l}'] = act(ch[l], _vox(dims[l]))
        for s in POOL_SIZES:
            n = s ** self.dim
            ws[f'pool{s}'], ws[f'dpool{s}'] = act(Cb, n), act(Cb, n)                   # A_s and its gradient
            ws[f'y.{branch(s)}'], ws[f'dq{s}'], ws[f'dyq{s}'] = act(Cq, n), act(Cq, n), act(Cq, n)
        ws['U'], ws['dU'] = act(2 * Cb, vb), act(2 * Cb, vb)
        ws['y.psp.out'] = act(C, vb)
        for l in range(B, T_LEVEL, -1):
            ws[f'p{l}'], ws[f'dp{l}'] = act(C, _vox(dims[l])), act(C, _vox(dims[l]))
        for l in laterals(L):
            ws[f'y.lat{l}'] = act(C, _vox(dims[l]))
        ws['V'], ws['dV'] = act((L - 2) * C, vt), act((L - 2) * C, vt)
        ws['y.fuse'], ws['feat'], ws['dfeat'] = act(C, vt), act(C, vt), act(C, vt)
        for prefix, ksz, ci, co in self._convs():
            d, rate = grids[prefix]
            if prefix != branch(1):
                self._bn_bufs(ws, mx, N, prefix, co, _vox(d))
            mx['dy'] = max(mx['dy'], co * _vox(d))
            mx['coef'] = max(mx['coef'], co)
            mx['stats'] = max(mx['stats'], lib.iunet_dl_stats_parts(N, *d, co) * co * 2)
            mx['wslab'] = max(mx['wslab'], lib.iunet_dl_wgrad_slab_floats(self.dim, rate, N, *d, ci, co))
        self._coarse_bufs(ws, N, D, H, W)

    def _skip_grad(self, ws, l):
        if l >= T_LEVEL:
            return self._P(ws[f'dskip{l}']), self.ch[l] * _vox(ws['dims'][l])
        return self._P(ws['zeros']), 0          # levels 0 and 1 receive gradient through the max-pool only

    # ------------------------------------------------------------------ launches
    def _conv(self, ws, op, kw, xp, x_ss, yp, y_ss, rate, N, d, ci, co, stats=False):
        nv.call('iunet_dl_conv_fwd', self.dt, self.dim, xp, x_ss, yp, y_ss, nv.ptr(self.pk[op]), kw, 1, nv.int_array([rate]), nv.int_array([0]),
                nv.int_array([0]), None, None, None, None, 1.0, nv.ptr(ws['stats']) if stats else None, 0, N, d[0], d[1], d[2], ci, co,
                nv.stream())

    def _conv_bn(self, ws, prefix, xp, x_ss, yp, y_ss, rate, N, d, ci, co):
        """The raw conv output with its batch statistics finalized into ws['scale.<prefix>'] ... (running statistics updated)."""
        kw = (self.kvol if rate else 1) * ci
        self._conv(ws, prefix, kw, xp, x_ss, yp, y_ss, rate, N, d, ci, co, stats=True)
        bn = prefix + '.bn'
        nv.call('iunet_bn_finalize', nv.ptr(ws['stats']), nv.lib().iunet_dl_stats_parts(N, *d, co), co, float(N * _vox(d)),
                nv.ptr(self.p(bn + '.weight')), nv.ptr(self.p(bn + '.bias')), nv.ptr(self.p(bn + '.running_mean')),
                nv.ptr(self.p(bn + '.running_var')), BN_MOMENTUM, BN_EPS, nv.ptr(ws[f'scale.{prefix}']), nv.ptr(ws[f'shift.{prefix}']),
                nv.ptr(ws[f'mean.{prefix}']), nv.ptr(ws[f'invstd.{prefix}']), nv.stream())

    def _resize(self, src, src_ss, ds, dst, dst_ss, dt, c, N, act=None, base=None, base_ss=0, base_act=None):
        sc, sh = (None, None) if act is None else act
        bsc, bsh = (None, None) if base_act is None else base_act
        nv.call('iunet_pn_resize', self.dt, self.dim, src, src_ss, ds[0], ds[1], ds[2], sc, sh, base, base_ss, bsc, bsh, dst, dst_ss,
                dt[0], dt[1], dt[2], c, N, nv.stream())

    def _adjoint(self, u, u_ss, dt, dx, dx_ss, ds, c, N, accumulate=False):
        nv.call('iunet_pn_resize_adjoint', self.dt, self.dim, u, u_ss, dt[0], dt[1], dt[2], dx, dx_ss, ds[0], ds[1], ds[2], c, N,
                int(accumulate), nv.stream())

    def _act_of(self, ws, prefix):
        return nv.ptr(ws[f'scale.{prefix}']), nv.ptr(ws[f'shift.{prefix}'])

    def _slots(self, ws, key):
        """l -> (pointer, sample stride) of level l's slot of V / dV (deepest first)."""
        L, C, vt = self.levels, self.C, _vox(ws['dims'][T_LEVEL])
        return lambda l: (self._P(ws[key], (L - 1 - l) * C * vt), (L - 2) * C * vt)

    # ------------------------------------------------------------------ forward
    def forward_train(self, x, x_strides, N, D, H, W):
        ws = self.workspace(N, D, H, W)
        self._encoder_forward(ws, x, x_strides, N)
        L, ch, dims, C, P = self.levels, self.ch, ws['dims'], self.C, self._P
        B, Cb, Cq = L - 1, ch[-1], ch[-1] // 4
        db, vb, dt, vt, nV = dims[-1], _vox(dims[-1]), dims[T_LEVEL], _vox(dims[T_LEVEL]), (L - 2) * C
        X = ws[f'x{B}']
        nb = [s ** self.dim for s in POOL_SIZES]
        nv.call('iunet_pn_pool', self.dt, self.dim, P(X), Cb * vb, db[0], db[1], db[2], nv.ptr_array([ws[f'pool{s}'] for s in POOL_SIZES]),
                nv.ll_array([Cb * n for n in nb]), Cb, N, nv.stream())
        self._resize(P(X), Cb * vb, db, P(ws['U']), 2 * Cb * vb, db, Cb, N)
        for k, s in enumerate(POOL_SIZES):
            d, b = pool_dims(self.dim, s), branch(s)
            if s == 1:
                self._conv(ws, b, Cb, P(ws['pool1']), Cb, P(ws[f'y.{b}']), Cq, 0, N, d, Cb, Cq)
                act = (nv.ptr(self.ones), nv.ptr(self.p(b + '.conv.bias')))
            else:
                self._conv_bn(ws, b, P(ws[f'pool{s}']), Cb * nb[k], P(ws[f'y.{b}']), Cq * nb[k], 0, N, d, Cb, Cq)
                act = self._act_of(ws, b)
            self._resize(P(ws[f'y.{b}']), Cq * nb[k], d, P(ws['U'], (Cb + k * Cq) * vb), 2 * Cb * vb, db, Cq, N, act=act)
        self._conv_bn(ws, 'psp.out', P(ws['U']), 2 * Cb * vb, P(ws['y.psp.out']), C * vb, 1, N, db, 2 * Cb, C)
        nv.call('iunet_bn_relu_fwd', self.dt, P(ws['y.psp.out']), C * vb, P(ws[f'p{B}']), C * vb, *self._act_of(ws, 'psp.out'), C, N, vb,
                nv.stream())
        slot = self._slots(ws, 'V')
        pl = lambda l: slot(l) if l == T_LEVEL else (P(ws[f'p{l}']), C * _vox(dims[l]))
        for l in laterals(L):
            v = _vox(dims[l])
            self._conv_bn(ws, f'lat{l}', P(ws[f'x{l}']), ch[l] * v, P(ws[f'y.lat{l}']), C * v, 0, N, dims[l], ch[l], C)
            (yp, y_ss), (up, u_ss) = pl(l), pl(l + 1)
            self._resize(up, u_ss, dims[l + 1], yp, y_ss, dims[l], C, N, base=P(ws[f'y.lat{l}']), base_ss=C * v,
                         base_act=self._act_of(ws, f'lat{l}'))
        for l in range(B, T_LEVEL, -1):
            self._resize(P(ws[f'p{l}']), C * _vox(dims[l]), dims[l], *slot(l), dt, C, N)
        self._conv_bn(ws, 'fuse', P(ws['V']), nV * vt, P(ws['y.fuse']), C * vt, 1, N, dt, nV, C)
        nv.call('iunet_bn_relu_fwd', self.dt, P(ws['y.fuse']), C * vt, P(ws['feat']), C * vt, *self._act_of(ws, 'fuse'), C, N, vt, nv.stream())
        self._head_fwd(ws, N)
        return ws

    # ------------------------------------------------------------------ backward
    def _bn_bwd(self, ws, prefix, dz, dz_ss, y, y_ss, c, v, N):
        """z = relu(bn(y)) backward into ws['dy'] (sample stride c v), dgamma / dbeta into the flat gradient."""
        bn = prefix + '.bn'
        nv.call('iunet_bn_relu_bwd', self.dt, dz, dz_ss, None, 0, y, y_ss, self._P(ws['dy']), c * v, nv.ptr(ws[f'mean.{prefix}']),
                nv.ptr(ws[f'invstd.{prefix}']), nv.ptr(self.p(bn + '.weight')), nv.ptr(ws[f'scale.{prefix}']), nv.ptr(ws[f'shift.{prefix}']),
                nv.ptr(self.g(bn + '.weight')), nv.ptr(self.g(bn + '.bias')), nv.ptr(ws['bnslab']), nv.ptr(ws['bncoef']), c, N, v, nv.stream())

    def _conv_bwd(self, ws, prefix, rate, xp, x_ss, dxp, dx_ss, N, d, ci, co, dy=None):
        """From the raw-output gradient (ws['dy'] unless given; sample stride co vox): the weight gradient and the data gradient."""
        v = _vox(d)
        dy = self._P(ws['dy']) if dy is None else dy
        nv.call('iunet_dl_wgrad', self.dt, self.dim, rate, xp, x_ss, 0, dy, co * v, None, None, nv.ptr(ws['wslab']),
                nv.ptr(self.g(prefix + '.conv.weight')), ci, 0, 1.0, N, d[0], d[1], d[2], ci, co, nv.stream())
        self._conv(ws, 'dg.' + prefix, (self.kvol if rate else 1) * co, dy, co * v, dxp, dx_ss, rate, N, d, co, ci)

    def backward(self, ws, x, x_strides, y, w, tdt, N):
        L, ch, dims, C, P = self.levels, self.ch, ws['dims'], self.C, self._P
        B, Cb, Cq = L - 1, ch[-1], ch[-1] // 4
        db, vb, dt, vt, nV = dims[-1], _vox(dims[-1]), dims[T_LEVEL], _vox(dims[T_LEVEL]), (L - 2) * C
        self._head_bwd(ws, y, w, tdt, N)
        # fuse -> dV
        self._bn_bwd(ws, 'fuse', P(ws['dfeat']), C * vt, P(ws['y.fuse']), C * vt, C, vt, N)
        self._conv_bwd(ws, 'fuse', 1, P(ws['V']), nV * vt, P(ws['dV']), nV * vt, N, dt, nV, C)
        # top-down path, from level 2 downwards: dP^2 is its slot of dV
        dslot = self._slots(ws, 'dV')
        dpl = lambda l: dslot(l) if l == T_LEVEL else (P(ws[f'dp{l}']), C * _vox(dims[l]))
        for l in reversed(laterals(L)):
            v = _vox(dims[l])
            (gp, g_ss), (np_, n_ss) = dpl(l), dpl(l + 1)
            self._bn_bwd(ws, f'lat{l}', gp, g_ss, P(ws[f'y.lat{l}']), C * v, C, v, N)
            self._conv_bwd(ws, f'lat{l}', 0, P(ws[f'x{l}']), ch[l] * v, P(ws[f'dskip{l}']), ch[l] * v, N, dims[l], ch[l], C)
            self._adjoint(*dslot(l + 1), dt, np_, n_ss, dims[l + 1], C, N)
            self._adjoint(gp, g_ss, dims[l], np_, n_ss, dims[l + 1], C, N, accumulate=True)
        # psp.out -> dU
        self._bn_bwd(ws, 'psp.out', P(ws[f'dp{B}']), C * vb, P(ws['y.psp.out']), C * vb, C, vb, N)
        self._conv_bwd(ws, 'psp.out', 1, P(ws['U']), 2 * Cb * vb, P(ws['dU']), 2 * Cb * vb, N, db, 2 * Cb, C)
        # the branches: R^T of their slots, norm + ReLU, conv -> dA_s
        for k, s in enumerate(POOL_SIZES):
            d, b, n = pool_dims(self.dim, s), branch(s), s ** self.dim
            self._adjoint(P(ws['dU'], (Cb + k * Cq) * vb), 2 * Cb * vb, db, P(ws[f'dq{s}']), Cq * n, d, Cq, N)
            if s == 1:
                nv.call('iunet_pn_bias_relu_bwd', self.dt, P(ws['dq1']), Cq, P(ws[f'y.{b}']), Cq, nv.ptr(self.p(b + '.conv.bias')), P(ws['dyq1']), Cq,
                        nv.ptr(self.g(b + '.conv.bias')), Cq, N, 1, nv.stream())
                dy = P(ws['dyq1'])
            else:
                self._bn_bwd(ws, b, P(ws[f'dq{s}']), Cq * n, P(ws[f'y.{b}']), Cq * n, Cq, n, N)
                dy = None
            self._conv_bwd(ws, b, 0, P(ws[f'pool{s}']), Cb * n, P(ws[f'dpool{s}']), Cb * n, N, d, Cb, Cq, dy=dy)
        nv.call('iunet_pn_pool_bwd', self.dt, self.dim, P(ws['dU']), 2 * Cb * vb, nv.ptr_array([ws[f'dpool{s}'] for s in POOL_SIZES]),
                nv.ll_array([Cb * s ** self.dim for s in POOL_SIZES]), P(ws[f'dskip{B}']), Cb * vb, db[0], db[1], db[2], Cb, N, nv.stream())
        self._encoder_backward(ws, x, x_strides, N)
