"""Native 16-bit training step of DeepLabV3 (engine_deeplab.py has the graph), sequenced from Python on train_engine.EncoderTrainEngine's encoder
and train_engine.CoarseTrainEngine's coarse-logit loss, flat AdamW, loss scaling and device-resident training state.

Forward on the coarse grid (csrc/deeplab.hip): each spatial ASPP branch writes its raw output into its slot of one 4C-channel buffer plus
BatchNorm partial sums; iunet_bn_finalize writes its scale / shift into the matching quarter of one [4C] pair, so the projection reads the
four raw slots through relu(scale * y + shift) in its loads (the branch activations are never stored).  The pooling branch (channel mean,
1x1 GEMV, BatchNorm over the N samples, ReLU) enters the projection as a per-sample bias.  The projection's BatchNorm + ReLU + dropout is one
pass (the mask drawn with the engine's own torch.Generator), dec.conv reads it, its activation F feeds the head, the coarse logits are
upsampled x 2^(L-1) inside the fused softmax + loss kernel.

Backward: the loss gradient at full resolution, the interpolation's adjoint as a gather, the head, dec.conv, the dropout, the projection
(its per-sample-bias gradient is the channel sum of its raw-output gradient), the pooling branch, the four branches' BatchNorm backward into
a 4C-slot gradient buffer and their data gradients in ONE launch with the pooling branch's adjoint added in its epilogue, then the encoder.
The encoder levels above the bottom receive gradient through the max-pool only (their skip input is a zero plane).
"""
import torch

from . import _native as nv
from .engine import BN_EPS
from .engine_deeplab import BRANCHES
from .train_engine import BN_MOMENTUM, CoarseTrainEngine, _vox

N1_MESSAGE = 'Expected more than 1 value per channel when training (the ASPP pooling branch normalises over the batch)'


class DeepLabV3TrainEngine(CoarseTrainEngine):
    architecture = 'DeepLabV3'

    def __init__(self, model, lr=None, loss_kind='mcc_ce', betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 loss_scale=None, process_group=None, seed=None):
        self.C = model.decoder_channels
        self.rates = (0,) + tuple(model.decoder_atrous_rates)
        self.p_drop = float(model.decoder_aspp_dropout)
        super().__init__(model, lr=lr, loss_kind=loss_kind, betas=betas, eps=eps, weight_decay=weight_decay, loss_scale=loss_scale,
                         process_group=process_group)
        self.kvol = 3 ** self.dim
        self.gen = torch.Generator(device=self.dev)
        self.gen.manual_seed(0 if seed is None else int(seed))
        self.last_dropout_mask = None

    @property
    def coarse_level(self):
        return self.levels - 1

    # ------------------------------------------------------------------ graph
    def _alloc_decoder(self):
        C, Cb, kv = self.C, self.ch[-1], 3 ** self.dim
        e = lambda n: torch.empty(n, dtype=self.T, device=self.dev)
        for b, r in zip(BRANCHES, self.rates):
            self.pk[b] = e(C * Cb * (1 if r == 0 else kv))
        self.pk['aspp.project'] = e(C * 4 * C)
        self.pk['dec'] = e(C * C * kv)
        self.pk['dg.project'] = e(4 * C * C)            # [4C][C]
        self.pk['dg.dec'] = e(C * kv * C)               # [C][kv C]
        self.aspp_ld = C * (1 + 3 * kv)                 # the four branches' data-gradient operators side by side: [Cb][C + 3 kv C]
        self.pk['dg.aspp'] = e(Cb * self.aspp_ld)

    def _dl_pack(self, mode, ksz, name, dst, Cout, Cin, Cin_tot, k_off, ld):
        nv.call('iunet_dl_pack', self.dt, self.dim, mode, ksz, nv.ptr(self.p(name)), None, None, None, None, 0.0, nv.ptr(dst), None,
                Cout, Cin, Cin_tot, 0, k_off, ld, nv.stream())

    def _pack_decoder(self):
        C, Cb, kv = self.C, self.ch[-1], 3 ** self.dim
        for k, (b, r) in enumerate(zip(BRANCHES, self.rates)):
            ksz, kk = (1, 1) if r == 0 else (3, kv)
            self._dl_pack(0, ksz, b + '.conv.weight', self.pk[b], C, Cb, Cb, 0, kk * Cb)
            self._dl_pack(1, ksz, b + '.conv.weight', self.pk['dg.aspp'], C, Cb, Cb, 0 if k == 0 else C + (k - 1) * kv * C, self.aspp_ld)
        self._dl_pack(0, 1, 'aspp.project.conv.weight', self.pk['aspp.project'], C, 4 * C, 5 * C, 0, 4 * C)
        self._dl_pack(1, 1, 'aspp.project.conv.weight', self.pk['dg.project'], C, 4 * C, 5 * C, 0, C)
        self._dl_pack(0, 3, 'dec.conv.weight', self.pk['dec'], C, C, C, 0, kv * C)
        self._dl_pack(1, 3, 'dec.conv.weight', self.pk['dg.dec'], C, C, C, 0, kv * C)

    # ------------------------------------------------------------------ workspace
    def _decoder_workspace(self, ws, mx, N, D, H, W):
        dims, ch, lib, C, L = ws['dims'], self.ch, nv.lib(), self.C, self.levels
        act, f32 = (lambda c, v: self._act(N, c, v)), self._f32
        dc, vc, Cb = dims[-1], _vox(dims[-1]), ch[-1]
        ws['dx'] = act(Cb, vc)                               # the gradient of X^{L-1}
        ws['zeros'] = act(max([ch[l] * _vox(dims[l]) for l in range(L - 1)] + [8]), 1).zero_()   # the skip gradient of the upper levels
        ws['ycat'] = act(4 * C, vc)
        ws['dcat'] = act(4 * C, vc)
        ws['dycat'] = act(4 * C, vc)
        for k in ('scale', 'shift', 'mean', 'invstd'):
            ws[f'{k}.cat'] = f32(4 * C)
        for name in ('aspp.project', 'dec', 'aspp.pool'):
            self._bn_bufs(ws, mx, N, name, C, vc)
        mx['coef'] = max(mx['coef'], 4 * C)
        ws['y.aspp.project'], ws['a'], ws['da'] = act(C, vc), act(C, vc), act(C, vc)
        ws['y.dec'], ws['feat'], ws['dfeat'] = act(C, vc), act(C, vc), act(C, vc)
        mx['stats'] = max(mx['stats'], lib.iunet_dl_stats_parts(N, *dc, C) * C * 2, N * C * 2)
        for r, ci, co in [(r, Cb, C) for r in self.rates] + [(0, 4 * C, C), (1, C, C)]:
            mx['wslab'] = max(mx['wslab'], lib.iunet_dl_wgrad_slab_floats(self.dim, r, N, *dc, ci, co))
        for k in ('xmean', 'dxmean'):
            ws[k] = f32(N * Cb)
        for k in ('ypool', 'bp', 'psb', 'dpsb'):
            ws[k] = f32(N * C)
        ws['pscratch'] = f32(2 * N * C)
        self._coarse_bufs(ws, N, D, H, W)

    def _skip_grad(self, ws, l):
        if l == self.levels - 1:
            return self._P(ws['dx']), self.ch[l] * _vox(ws['dims'][l])
        return self._P(ws['zeros']), 0          # the upper levels receive gradient through the max-pool only

    # ------------------------------------------------------------------ forward
    def _finalize(self, ws, bn, stats_parts, c, count, out):
        """iunet_bn_finalize of the BatchNorm `bn` into ws['<k>.<out>'] (out may be a (name, offset) slice of the [4C] branch pair)."""
        name, off = out if isinstance(out, tuple) else (out, 0)
        sl = lambda k: nv.ptr(ws[f'{k}.{name}'][off:off + c])
        nv.call('iunet_bn_finalize', nv.ptr(ws['stats']), stats_parts, c, float(count), nv.ptr(self.p(bn + '.weight')), nv.ptr(self.p(bn + '.bias')),
                nv.ptr(self.p(bn + '.running_mean')), nv.ptr(self.p(bn + '.running_var')), BN_MOMENTUM, BN_EPS,
                sl('scale'), sl('shift'), sl('mean'), sl('invstd'), nv.stream())

    def _dl(self, wpk, kw, xp, x_ss, yp, y_ss, rates, cbase, colbase, N, dc, ci, co, act=None, psb=None, psb_scale=1.0, stats=True):
        sc, sh = (None, None) if act is None else act
        nv.call('iunet_dl_conv_fwd', self.dt, self.dim, xp, x_ss, yp, y_ss, nv.ptr(wpk), kw, len(rates), nv.int_array(rates),
                nv.int_array(cbase), nv.int_array(colbase), sc, sh, None, psb, float(psb_scale),
                nv.ptr(self._ws_cur['stats']) if stats else None, 0, N, dc[0], dc[1], dc[2], ci, co, nv.stream())

    def forward_train(self, x, x_strides, N, D, H, W):
        ws = self.workspace(N, D, H, W)
        self._ws_cur = ws
        self._encoder_forward(ws, x, x_strides, N)
        L, ch, dims, C = self.levels, self.ch, ws['dims'], self.C
        s = nv.stream()
        dc, vc, Cb, X = dims[-1], _vox(dims[-1]), ch[-1], ws[f'x{L - 1}']
        nparts = nv.lib().iunet_dl_stats_parts(N, *dc, C)
        # pooling branch -> per-sample bias of the projection
        nv.call('iunet_dl_chansum', self.dt, self._P(X), Cb * vc, nv.ptr(ws['xmean']), 1.0 / vc, Cb, N, vc, s)
        nv.call('iunet_dl_pool_gemv', nv.ptr(ws['xmean']), nv.ptr(self.p('aspp.pool.conv.weight')), nv.ptr(ws['ypool']), nv.ptr(ws['stats']),
                N, Cb, C, s)
        self._finalize(ws, 'aspp.pool.bn', N, C, N, 'aspp.pool')
        nv.call('iunet_dl_pool_psb', nv.ptr(ws['ypool']), nv.ptr(ws['scale.aspp.pool']), nv.ptr(ws['shift.aspp.pool']), None, None, None, None,
                BN_EPS, nv.ptr(ws['bp']), nv.ptr(self.p('aspp.project.conv.weight')), None, None, nv.ptr(ws['psb']), N, C, s)
        # the four spatial branches: raw outputs into their slots, statistics into their quarter of the [4C] pair
        for k, (b, r) in enumerate(zip(BRANCHES, self.rates)):
            kw = Cb * (1 if r == 0 else self.kvol)
            self._dl(self.pk[b], kw, self._P(X), Cb * vc, self._P(ws['ycat'], k * C * vc), 4 * C * vc, [r], [0], [0], N, dc, Cb, C)
            self._finalize(ws, b + '.bn', nparts, C, N * vc, ('cat', k * C))
        cat_act = (nv.ptr(ws['scale.cat']), nv.ptr(ws['shift.cat']))
        self._dl(self.pk['aspp.project'], 4 * C, self._P(ws['ycat']), 4 * C * vc, self._P(ws['y.aspp.project']), C * vc, [0], [0], [0], N, dc,
                 4 * C, C, act=cat_act, psb=nv.ptr(ws['psb']))
        self._finalize(ws, 'aspp.project.bn', nparts, C, N * vc, 'aspp.project')
        mask = None
        if self.p_drop > 0.0:
            mask = torch.empty((N, C) + tuple(dc[3 - self.dim:]), dtype=torch.uint8, device=self.dev).bernoulli_(1.0 - self.p_drop, generator=self.gen)
        self.last_dropout_mask = mask
        nv.call('iunet_dl_dropout', self.dt, 0, self._P(ws['y.aspp.project']), C * vc, self._P(ws['a']), C * vc, nv.ptr(ws['scale.aspp.project']),
                nv.ptr(ws['shift.aspp.project']), nv.ptr(mask), self.p_drop, C, N, vc, s)
        self._dl(self.pk['dec'], self.kvol * C, self._P(ws['a']), C * vc, self._P(ws['y.dec']), C * vc, [1], [0], [0], N, dc, C, C)
        self._finalize(ws, 'dec.bn', nparts, C, N * vc, 'dec')
        nv.call('iunet_bn_relu_fwd', self.dt, self._P(ws['y.dec']), C * vc, self._P(ws['feat']), C * vc, nv.ptr(ws['scale.dec']),
                nv.ptr(ws['shift.dec']), C, N, vc, s)
        self._head_fwd(ws, N)
        return ws

    # ------------------------------------------------------------------ backward
    def _bn_bwd(self, ws, dz, dz_ss, y, y_ss, dy, dy_ss, bn, name, off, c, v, N):
        sl = lambda k: nv.ptr(ws[f'{k}.{name}'][off:off + c])
        nv.call('iunet_bn_relu_bwd', self.dt, dz, dz_ss, None, 0, y, y_ss, dy, dy_ss, sl('mean'), sl('invstd'), nv.ptr(self.p(bn + '.weight')),
                sl('scale'), sl('shift'), nv.ptr(self.g(bn + '.weight')), nv.ptr(self.g(bn + '.bias')), nv.ptr(ws['bnslab']), nv.ptr(ws['bncoef']),
                c, N, v, nv.stream())

    def _wgrad(self, ws, rate, xp, x_ss, dyp, dy_ss, name, cin_tot, N, dc, ci, co, act=None):
        sc, sh = (None, None) if act is None else act
        nv.call('iunet_dl_wgrad', self.dt, self.dim, rate, xp, x_ss, 0, dyp, dy_ss, sc, sh, nv.ptr(ws['wslab']), nv.ptr(self.g(name)), cin_tot, 0,
                1.0, N, dc[0], dc[1], dc[2], ci, co, nv.stream())

    def backward(self, ws, x, x_strides, y, w, tdt, N):
        L, ch, dims, C = self.levels, self.ch, ws['dims'], self.C
        s = nv.stream()
        dc, vc, Cb, X = dims[-1], _vox(dims[-1]), ch[-1], ws[f'x{L - 1}']
        P = self._P
        self._head_bwd(ws, y, w, tdt, N)
        # dec.conv
        self._bn_bwd(ws, P(ws['dfeat']), C * vc, P(ws['y.dec']), C * vc, P(ws['dy']), C * vc, 'dec.bn', 'dec', 0, C, vc, N)
        self._wgrad(ws, 1, P(ws['a']), C * vc, P(ws['dy']), C * vc, 'dec.conv.weight', C, N, dc, C, C)
        self._dl(self.pk['dg.dec'], self.kvol * C, P(ws['dy']), C * vc, P(ws['da']), C * vc, [1], [0], [0], N, dc, C, C, stats=False)
        # dropout, projection BatchNorm + ReLU
        nv.call('iunet_dl_dropout', self.dt, 1, P(ws['da']), C * vc, P(ws['da']), C * vc, None, None, nv.ptr(self.last_dropout_mask),
                self.p_drop, C, N, vc, s)
        self._bn_bwd(ws, P(ws['da']), C * vc, P(ws['y.aspp.project']), C * vc, P(ws['dy']), C * vc, 'aspp.project.bn', 'aspp.project', 0, C,
                     vc, N)
        # projection: per-sample-bias gradient, weight gradient over the four slots, data gradient into the slots
        nv.call('iunet_dl_chansum', self.dt, P(ws['dy']), C * vc, nv.ptr(ws['dpsb']), 1.0, C, N, vc, s)
        cat_act = (nv.ptr(ws['scale.cat']), nv.ptr(ws['shift.cat']))
        self._wgrad(ws, 0, P(ws['ycat']), 4 * C * vc, P(ws['dy']), C * vc, 'aspp.project.conv.weight', 5 * C, N, dc, 4 * C, C, act=cat_act)
        self._dl(self.pk['dg.project'], C, P(ws['dy']), C * vc, P(ws['dcat']), 4 * C * vc, [0], [0], [0], N, dc, C, 4 * C, stats=False)
        # pooling branch
        nv.call('iunet_dl_pool_bwd', nv.ptr(ws['dpsb']), nv.ptr(ws['bp']), nv.ptr(ws['ypool']), nv.ptr(ws['mean.aspp.pool']),
                nv.ptr(ws['invstd.aspp.pool']), nv.ptr(self.p('aspp.pool.bn.weight')), nv.ptr(self.p('aspp.project.conv.weight')),
                nv.ptr(self.p('aspp.pool.conv.weight')), nv.ptr(ws['xmean']), nv.ptr(self.g('aspp.project.conv.weight')),
                nv.ptr(self.g('aspp.pool.bn.weight')), nv.ptr(self.g('aspp.pool.bn.bias')), nv.ptr(self.g('aspp.pool.conv.weight')),
                nv.ptr(ws['dxmean']), nv.ptr(ws['pscratch']), N, Cb, C, s)
        # the four spatial branches
        for k, (b, r) in enumerate(zip(BRANCHES, self.rates)):
            o = k * C * vc
            self._bn_bwd(ws, P(ws['dcat'], o), 4 * C * vc, P(ws['ycat'], o), 4 * C * vc, P(ws['dycat'], o), 4 * C * vc, b + '.bn', 'cat', k * C,
                         C, vc, N)
            self._wgrad(ws, r, P(X), Cb * vc, P(ws['dycat'], o), 4 * C * vc, b + '.conv.weight', Cb, N, dc, Cb, C)
        kv = self.kvol
        self._dl(self.pk['dg.aspp'], self.aspp_ld, P(ws['dycat']), 4 * C * vc, P(ws['dx']), Cb * vc, list(self.rates), [0, C, 2 * C, 3 * C],
                 [0, C, C + kv * C, C + 2 * kv * C], N, dc, C, Cb, psb=nv.ptr(ws['dxmean']), psb_scale=1.0 / vc, stats=False)
        self._encoder_backward(ws, x, x_strides, N)

    # ------------------------------------------------------------------ public steps
    def _check_batch(self, X):
        if X.shape[0] < 2:
            raise ValueError(N1_MESSAGE)

    def train_step(self, X, y, w=None, sync=True):
        self._check_batch(X)
        return super().train_step(X, y, w, sync)

    def step_forward(self, X, y, w=None):
        self._check_batch(X)
        return super().step_forward(X, y, w)
