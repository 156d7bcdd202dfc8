"""Native 16-bit training step of Segformer (engine_segformer.py has the graph), sequenced from Python on train_engine.EncoderTrainEngine's encoder
and train_engine.CoarseTrainEngine's coarse-logit loss, flat AdamW, loss scaling and device-resident training state.

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
from .engine_segformer import T_LEVEL, pack_args, sources
from .train_engine import BN_MOMENTUM, CoarseTrainEngine, _vox


class SegformerTrainEngine(CoarseTrainEngine):
    architecture = 'Segformer'
    skip_grad = 'dskip'           # dskip{l} = R_l^T(M_l^T dZ): the skip gradient of level l
    coarse_level = T_LEVEL

    def __init__(self, model, lr=None, loss_kind='mcc_ce', betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 loss_scale=None, process_group=None):
        self.C = model.decoder_segmentation_channels
        super().__init__(model, lr=lr, loss_kind=loss_kind, betas=betas, eps=eps, weight_decay=weight_decay, loss_scale=loss_scale,
                         process_group=process_group)
        self.K = sum(self.ch)
        self.koff = [sum(self.ch[:l]) for l in range(self.levels)]

    # ------------------------------------------------------------------ graph
    def _alloc_decoder(self):
        K = sum(self.ch)
        self.pk['M'] = torch.empty(self.C * K, dtype=self.T, device=self.dev)       # [C][K]
        self.pk['MT'] = torch.empty(K * self.C, dtype=self.T, device=self.dev)      # [K][C]
        self.pk['beta'] = torch.empty(self.C, dtype=torch.float32, device=self.dev)

    def _pack_decoder(self):
        wf, w, b, _ = pack_args(self.p, self.levels)
        nv.call('iunet_sf_pack', self.dt, self.levels, self.C, nv.int_array(self.ch), wf, w, b, None, None, None, None, 0.0,
                nv.ptr(self.pk['M']), nv.ptr(self.pk['MT']), nv.ptr(self.pk['beta']), nv.stream())

    # ------------------------------------------------------------------ workspace
    def _decoder_workspace(self, ws, mx, N, D, H, W):
        dims, lib, C, K = ws['dims'], nv.lib(), self.C, sum(self.ch)
        act, f32 = (lambda c, v: self._act(N, c, v)), self._f32
        dt, vt = dims[T_LEVEL], _vox(dims[T_LEVEL])
        self._bn_bufs(ws, mx, N, 'fuse', C, vt)
        mx['coef'] = max(mx['coef'], C)
        ws['z'], ws['feat'], ws['dfeat'], ws['dzf'] = act(C, vt), act(C, vt), act(C, vt), act(C, vt)    # Z, F, dF, dZ on T
        ws['u'] = act(K, vt)                                 # M^T dZ on T (K = sum ch channels)
        mx['stats'] = max(mx['stats'], lib.iunet_sf_stats_parts(N, *dt) * C * 2)
        ws['G'] = f32(C * K)
        ws['gslab'] = f32(lib.iunet_sf_wgrad_slab_floats(N, *dt, K, C))
        ws['rs'] = f32(N * C)
        self._coarse_bufs(ws, N, D, H, W)

    # ------------------------------------------------------------------ forward
    def forward_train(self, x, x_strides, N, D, H, W):
        ws = self.workspace(N, D, H, W)
        self._encoder_forward(ws, x, x_strides, N)
        L, ch, dims, C = self.levels, self.ch, ws['dims'], self.C
        s = nv.stream()
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
        self._head_fwd(ws, N)
        return ws

    # ------------------------------------------------------------------ backward
    def backward(self, ws, x, x_strides, y, w, tdt, N):
        L, ch, dims, C, K = self.levels, self.ch, ws['dims'], self.C, self.K
        s = nv.stream()
        dt, vt = dims[T_LEVEL], _vox(dims[T_LEVEL])
        P = self._P
        self._head_bwd(ws, y, w, tdt, N)
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
        wf, w_, b_, _ = pack_args(self.p, L)
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
        self._encoder_backward(ws, x, x_strides, N)
