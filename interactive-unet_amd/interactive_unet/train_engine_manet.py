"""Native 16-bit training step of MA-Net (engine_manet.py has the graph), sequenced from Python on train_engine.EncoderTrainEngine's encoder
and train_engine.TrainEngine's head / loss kernels, flat AdamW, loss scaling and eval_step.

Forward.  Q, Kc and V are raw gathered GEMMs (iunet_dl_conv_fwd); iunet_ma_attn_fwd adds their biases, writes Y = X^B + A V + b and keeps a
row's log-sum-exp.  Every conv with a BatchNorm writes its RAW output and partial sums, iunet_bn_finalize turns them into scale / shift and
iunet_bn_relu_fwd writes the activation.  A block's gates are iunet_ma_gate on iunet_dl_chansum's means of h and of the skip; the skip is
copied into the concat buffer's first slot (iunet_pn_resize at equal grids) and iunet_ma_up_gate writes nearest_up2(h) g into the second.

Backward.  The head's gradient (iunet_head_loss_bwd_dev), then per block from level 0 upwards: the stage convs (BatchNorm backward, weight
gradient, data gradient) down to the concat buffer's gradient; its second slot gives dg (iunet_ma_up_gate_dg, fixed-order sums), the gates'
parameter gradients and the two mean gradients (iunet_ma_gate_bwd), then dh (iunet_ma_up_gate_bwd); the first slot, with the skip mean's
share added (iunet_ma_add_mean_grad), is X^l's skip gradient; hl1 and hl3 give the gradient of the block's input.  The attention block:
pab.out gives dY; iunet_ma_attn_bwd (two launches, P recomputed from Q, Kc and the log-sum-exp) gives dQ, dKc and dV; the bias gradients
are fixed-order sums of dKc and dY (the queries' bias does not reach the output: its gradient is zero); X^B's skip gradient is dY plus the
three convs' data gradients, added one at a time by iunet_pn_resize at equal grids.
"""
import torch

from . import _native as nv
from .engine import BN_EPS
from .engine_manet import QK, SE_KEYS, blocks, check_setup, check_tokens, conv_table, gate_width, gated_concat
from .train_engine import BN_MOMENTUM, EncoderTrainEngine, _vox


class MANetTrainEngine(EncoderTrainEngine):
    architecture = 'MA-Net'

    def __init__(self, model, lr=None, loss_kind='mcc_ce', betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 loss_scale=None, process_group=None):
        if process_group is not None:
            raise NotImplementedError('MA-Net training runs on one GPU: a process_group (data parallel training) is not supported')
        check_setup('MA-Net training', model.levels, [model.base * 2 ** l for l in range(model.levels)])
        super().__init__(model, lr=lr, loss_kind=loss_kind, betas=betas, eps=eps, weight_decay=weight_decay, loss_scale=loss_scale,
                         process_group=process_group)

    # ------------------------------------------------------------------ graph
    def _first_decoder_param(self):
        return 'pab.top.conv.weight'

    def _convs(self):
        return conv_table(self.levels, self.ch)

    def _alloc_decoder(self):
        self.kvol = 3 ** self.dim
        for prefix, _, _, ksz, ci, co in self._convs():
            n = co * ci * (1 if ksz == 1 else self.kvol)
            self.pk[prefix] = torch.empty(n, dtype=self.T, device=self.dev)            # forward [co][k ci]
            self.pk['dg.' + prefix] = torch.empty(n, dtype=self.T, device=self.dev)    # data gradient [ci][k co]

    def _pack_decoder(self):
        for prefix, wn, _, ksz, ci, co in self._convs():
            kk = 1 if ksz == 1 else self.kvol
            for mode, dst, ld in ((0, self.pk[prefix], kk * ci), (1, self.pk['dg.' + prefix], kk * co)):
                nv.call('iunet_dl_pack', self.dt, self.dim, mode, ksz, nv.ptr(self.p(wn + '.weight')), None, None, None, None, 0.0, nv.ptr(dst),
                        None, co, ci, ci, 0, 0, ld, nv.stream())

    # ------------------------------------------------------------------ workspace
    def _grids(self, dims):
        """{prefix: grid} of every decoder conv."""
        g = {p: dims[-1] for p in ('pab.top', 'pab.center', 'pab.bottom', 'pab.out')}
        for l in blocks(self.levels):
            g.update({f'dec{l}.hl3': dims[l + 1], f'dec{l}.hl1': dims[l + 1], f'dec{l}.conv1': dims[l], f'dec{l}.conv2': dims[l]})
        return g

    def _decoder_workspace(self, ws, mx, N, D, H, W):
        dims, ch, lib, L = ws['dims'], self.ch, nv.lib(), self.levels
        act = lambda c, v: self._act(N, c, v)
        Cb, T = ch[-1], _vox(dims[-1])
        check_tokens(T)
        for k in ('q', 'k', 'dq', 'dk'):
            ws[k] = act(QK, T)
        for k in ('v', 'dv', 'Y', 'dY', 'z', 'dz', 'dxa', f'dskip{L - 1}'):
            ws[k] = act(Cb, T)
        ws['lse'], ws['delta'], ws['bsum'] = self._f32(N * T), self._f32(N * T), self._f32(N * Cb)
        for l in blocks(L):
            v, vi, c, ci = _vox(dims[l]), _vox(dims[l + 1]), ch[l], ch[l + 1]
            m = gate_width(c)
            ws[f't{l}'], ws[f'dt{l}'] = act(ci, vi), act(ci, vi)
            ws[f'h{l}'], ws[f'dh{l}'] = act(c, vi), act(c, vi)
            ws[f'cat{l}'], ws[f'dcat{l}'] = act(2 * c, v), act(2 * c, v)
            ws[f'c1{l}'], ws[f'dc1{l}'] = act(c, v), act(c, v)
            ws[f'd{l}'], ws[f'dd{l}'] = act(c, v), act(c, v)
            for k in ('mh', 'ms', 'g', 'dg', 'dmh', 'dms'):
                ws[f'{k}{l}'] = self._f32(N * c)
            ws[f'hid{l}'], ws[f'dhid{l}'], ws[f'sig{l}'] = self._f32(N * 2 * m), self._f32(N * 2 * m), self._f32(N * 2 * c)
            ws[f'dgpart{l}'] = self._f32(nv.answer(lib.iunet_ma_up_gate_dg_parts(self.dim, N, *dims[l + 1], c)) * N * c)
        grids = self._grids(dims)
        for prefix, _, bn, ksz, ci, co in self._convs():
            d = grids[prefix]
            if bn is not None:
                ws['y.' + prefix] = act(co, _vox(d))
                self._bn_bufs(ws, mx, N, prefix, co, _vox(d))
            mx['dy'] = max(mx['dy'], co * _vox(d))
            mx['coef'] = max(mx['coef'], co)
            mx['stats'] = max(mx['stats'], lib.iunet_dl_stats_parts(N, *d, co) * co * 2)
            mx['wslab'] = max(mx['wslab'], lib.iunet_dl_wgrad_slab_floats(self.dim, int(ksz == 3), N, *d, ci, co))

    def _skip_grad(self, ws, l):
        if l == self.levels - 1:
            return self._P(ws[f'dskip{l}']), self.ch[l] * _vox(ws['dims'][l])
        return self._P(ws[f'dcat{l}']), 2 * self.ch[l] * _vox(ws['dims'][l])      # the concat gradient's first slot

    # ------------------------------------------------------------------ launches
    def _conv(self, ws, op, kw, xp, x_ss, yp, y_ss, rate, N, d, ci, co, stats=False):
        nv.call('iunet_dl_conv_fwd', self.dt, self.dim, xp, x_ss, yp, y_ss, nv.ptr(self.pk[op]), kw, 1, nv.int_array([rate]), nv.int_array([0]),
                nv.int_array([0]), None, None, None, None, 1.0, nv.ptr(ws['stats']) if stats else None, 0, N, d[0], d[1], d[2], ci, co,
                nv.stream())

    def _conv_bn_relu(self, ws, prefix, bn, xp, x_ss, zp, z_ss, rate, N, d, ci, co):
        """z = relu(bn(conv(x))): the raw output in ws['y.<prefix>'], its batch statistics finalized (running statistics updated)."""
        v = _vox(d)
        y = self._P(ws['y.' + prefix])
        self._conv(ws, prefix, (self.kvol if rate else 1) * ci, xp, x_ss, y, co * v, rate, N, d, ci, co, stats=True)
        nv.call('iunet_bn_finalize', nv.ptr(ws['stats']), nv.lib().iunet_dl_stats_parts(N, *d, co), co, float(N * v),
                nv.ptr(self.p(bn + '.weight')), nv.ptr(self.p(bn + '.bias')), nv.ptr(self.p(bn + '.running_mean')),
                nv.ptr(self.p(bn + '.running_var')), BN_MOMENTUM, BN_EPS, nv.ptr(ws[f'scale.{prefix}']), nv.ptr(ws[f'shift.{prefix}']),
                nv.ptr(ws[f'mean.{prefix}']), nv.ptr(ws[f'invstd.{prefix}']), nv.stream())
        nv.call('iunet_bn_relu_fwd', self.dt, y, co * v, zp, z_ss, nv.ptr(ws[f'scale.{prefix}']), nv.ptr(ws[f'shift.{prefix}']), co, N, v,
                nv.stream())

    def _add(self, ws, a, b, dst, c, d, N):
        """dst = a + b on one grid (contiguous tensors of c channels; dst may be a)."""
        ss = c * _vox(d)
        nv.call('iunet_pn_resize', self.dt, self.dim, b, ss, d[0], d[1], d[2], None, None, a, ss, None, None, dst, ss, d[0], d[1], d[2], c, N,
                nv.stream())

    def _block_input(self, ws, l):
        """(activation, its gradient) of block l's input: Z for the first block, else the previous block's output."""
        return (ws['z'], ws['dz']) if l == self.levels - 2 else (ws[f'd{l + 1}'], ws[f'dd{l + 1}'])

    # ------------------------------------------------------------------ forward
    def forward_train(self, x, x_strides, N, D, H, W):
        ws = self.workspace(N, D, H, W)
        self._encoder_forward(ws, x, x_strides, N)
        L, ch, dims, P, s = self.levels, self.ch, ws['dims'], self._P, nv.stream()
        B, Cb, db = L - 1, ch[-1], dims[-1]
        T = _vox(db)
        X = P(ws[f'x{B}'])
        self._conv(ws, 'pab.top', Cb, X, Cb * T, P(ws['q']), QK * T, 0, N, db, Cb, QK)
        self._conv(ws, 'pab.center', Cb, X, Cb * T, P(ws['k']), QK * T, 0, N, db, Cb, QK)
        self._conv(ws, 'pab.bottom', self.kvol * Cb, X, Cb * T, P(ws['v']), Cb * T, 1, N, db, Cb, Cb)
        nv.call('iunet_ma_attn_fwd', self.dt, P(ws['q']), QK * T, nv.ptr(self.p('pab.top.conv.bias')), P(ws['k']), QK * T,
                nv.ptr(self.p('pab.center.conv.bias')), P(ws['v']), Cb * T, X, Cb * T, nv.ptr(self.p('pab.bottom.conv.bias')), P(ws['Y']),
                Cb * T, nv.ptr(ws['lse']), Cb, T, N, s)
        self._conv_bn_relu(ws, 'pab.out', 'pab.out.bn', P(ws['Y']), Cb * T, P(ws['z']), Cb * T, 1, N, db, Cb, Cb)
        for l in blocks(L):
            d, di, v, vi, c, ci = dims[l], dims[l + 1], _vox(dims[l]), _vox(dims[l + 1]), ch[l], ch[l + 1]
            src, _ = self._block_input(ws, l)
            self._conv_bn_relu(ws, f'dec{l}.hl3', f'dec{l}.hl3.bn', P(src), ci * vi, P(ws[f't{l}']), ci * vi, 1, N, di, ci, ci)
            self._conv_bn_relu(ws, f'dec{l}.hl1', f'dec{l}.hl1.bn', P(ws[f't{l}']), ci * vi, P(ws[f'h{l}']), c * vi, 0, N, di, ci, c)
            gated_concat(self.dt, self.dim, P, ws, l, [self.p(f'dec{l}.{k}') for k in SE_KEYS], dims, ch, N)
            self._conv_bn_relu(ws, f'dec{l}.conv1', f'dec{l}.bn1', P(ws[f'cat{l}']), 2 * c * v, P(ws[f'c1{l}']), c * v, 1, N, d, 2 * c, c)
            self._conv_bn_relu(ws, f'dec{l}.conv2', f'dec{l}.bn2', P(ws[f'c1{l}']), c * v, P(ws[f'd{l}']), c * v, 1, N, d, c, c)
        return ws

    def train_loss_forward(self, ws, y, w, N, vox):
        return self.loss_forward(ws, ws['d0'], y, w, N, vox)

    # ------------------------------------------------------------------ backward
    def _bn_bwd(self, ws, prefix, bn, dz, c, v, N):
        """z = relu(bn(y)) backward (the mask recomputed from the raw output) into ws['dy'], dgamma / dbeta into the flat gradient."""
        nv.call('iunet_bn_relu_bwd', self.dt, dz, c * v, None, 0, self._P(ws['y.' + prefix]), c * v, self._P(ws['dy']), c * v,
                nv.ptr(ws[f'mean.{prefix}']), nv.ptr(ws[f'invstd.{prefix}']), nv.ptr(self.p(bn + '.weight')), nv.ptr(ws[f'scale.{prefix}']),
                nv.ptr(ws[f'shift.{prefix}']), nv.ptr(self.g(bn + '.weight')), nv.ptr(self.g(bn + '.bias')), nv.ptr(ws['bnslab']),
                nv.ptr(ws['bncoef']), c, N, v, nv.stream())

    def _conv_bwd(self, ws, prefix, wn, rate, xp, x_ss, dxp, dx_ss, N, d, ci, co, dy=None):
        """From the raw-output gradient (ws['dy'] unless given; sample stride co vox): the weight gradient and the data gradient."""
        v = _vox(d)
        dy = self._P(ws['dy']) if dy is None else dy
        nv.call('iunet_dl_wgrad', self.dt, self.dim, rate, xp, x_ss, 0, dy, co * v, None, None, nv.ptr(ws['wslab']),
                nv.ptr(self.g(wn + '.weight')), ci, 0, 1.0, N, d[0], d[1], d[2], ci, co, nv.stream())
        self._conv(ws, 'dg.' + prefix, (self.kvol if rate else 1) * co, dy, co * v, dxp, dx_ss, rate, N, d, co, ci)

    def _bias_grad(self, ws, t, c, T, N, name):
        """The gradient of a conv bias: the sum of t over the grid (per sample, iunet_dl_chansum), then over the batch in sample order."""
        s = nv.stream()
        nv.call('iunet_dl_chansum', self.dt, self._P(t), c * T, nv.ptr(ws['bsum']), 1.0, c, N, T, s)
        nv.call('iunet_reduce_slab', nv.ptr(ws['bsum']), N, c, nv.ptr(self.g(name)), 1.0, 0, s)

    def backward(self, ws, x, x_strides, y, w, tdt, N):
        L, ch, dims, P, s = self.levels, self.ch, ws['dims'], self._P, nv.stream()
        v0 = _vox(dims[0])
        nparts = nv.lib().iunet_head_loss_bwd_num_parts(N, v0, self.ncls, ch[0])
        nv.call('iunet_head_loss_bwd_dev', self.dt, P(ws['d0']), ch[0] * v0, ch[0], nv.ptr(self.p('head.weight')),
                nv.ptr(self.p('head.bias')), self.ncls, nv.ptr(y), nv.ptr(w), tdt, nv.ptr(ws['coef']),
                nv.ptr(self.state), P(ws['dd0']), ch[0] * v0, nv.ptr(ws['hslab']), None, None, N, v0, s)
        nv.call('iunet_reduce_slab', nv.ptr(ws['hslab']), nparts, self.ncls * (ch[0] + 1), nv.ptr(ws['htmp']), 1.0, 0, s)
        nv.call('iunet_head_grad_scatter', nv.ptr(ws['htmp']), nv.ptr(self.g('head.weight')), nv.ptr(self.g('head.bias')), self.ncls, ch[0], s)
        for l in reversed(blocks(L)):
            d, di, v, vi, c, ci = dims[l], dims[l + 1], _vox(dims[l]), _vox(dims[l + 1]), ch[l], ch[l + 1]
            m = gate_width(c)
            src, dsrc = self._block_input(ws, l)
            # the stage: conv2, conv1 -> the concat buffer's gradient
            self._bn_bwd(ws, f'dec{l}.conv2', f'dec{l}.bn2', P(ws[f'dd{l}']), c, v, N)
            self._conv_bwd(ws, f'dec{l}.conv2', f'dec{l}.conv2', 1, P(ws[f'c1{l}']), c * v, P(ws[f'dc1{l}']), c * v, N, d, c, c)
            self._bn_bwd(ws, f'dec{l}.conv1', f'dec{l}.bn1', P(ws[f'dc1{l}']), c, v, N)
            self._conv_bwd(ws, f'dec{l}.conv1', f'dec{l}.conv1', 1, P(ws[f'cat{l}']), 2 * c * v, P(ws[f'dcat{l}']), 2 * c * v, N, d, 2 * c, c)
            # the gated upsampling: dg, the gates, dh; the skip's share of its gate's gradient
            du = P(ws[f'dcat{l}'], c * v)
            nv.call('iunet_ma_up_gate_dg', self.dt, self.dim, du, 2 * c * v, P(ws[f'h{l}']), c * vi, None, None, nv.ptr(ws[f'dgpart{l}']),
                    nv.ptr(ws[f'dg{l}']), di[0], di[1], di[2], c, N, s)
            se = lambda k: f'dec{l}.{k}'
            nv.call('iunet_ma_gate_bwd', nv.ptr(ws[f'dg{l}']), nv.ptr(ws[f'mh{l}']), nv.ptr(ws[f'ms{l}']),
                    nv.ptr(self.p(se('se_hl.fc1.weight'))), nv.ptr(self.p(se('se_hl.fc2.weight'))), nv.ptr(self.p(se('se_ll.fc1.weight'))),
                    nv.ptr(self.p(se('se_ll.fc2.weight'))), nv.ptr(ws[f'hid{l}']), nv.ptr(ws[f'sig{l}']), nv.ptr(ws[f'dhid{l}']),
                    *[nv.ptr(self.g(se(k))) for k in SE_KEYS], nv.ptr(ws[f'dmh{l}']), nv.ptr(ws[f'dms{l}']), c, m, N, s)
            nv.call('iunet_ma_up_gate_bwd', self.dt, self.dim, du, 2 * c * v, nv.ptr(ws[f'g{l}']), nv.ptr(ws[f'dmh{l}']), P(ws[f'dh{l}']), c * vi,
                    di[0], di[1], di[2], c, N, s)
            nv.call('iunet_ma_add_mean_grad', self.dt, P(ws[f'dcat{l}']), 2 * c * v, nv.ptr(ws[f'dms{l}']), c, N, v, s)
            # hl1, hl3 -> the gradient of the block's input
            self._bn_bwd(ws, f'dec{l}.hl1', f'dec{l}.hl1.bn', P(ws[f'dh{l}']), c, vi, N)
            self._conv_bwd(ws, f'dec{l}.hl1', f'dec{l}.hl1.conv', 0, P(ws[f't{l}']), ci * vi, P(ws[f'dt{l}']), ci * vi, N, di, ci, c)
            self._bn_bwd(ws, f'dec{l}.hl3', f'dec{l}.hl3.bn', P(ws[f'dt{l}']), ci, vi, N)
            self._conv_bwd(ws, f'dec{l}.hl3', f'dec{l}.hl3.conv', 1, P(src), ci * vi, P(dsrc), ci * vi, N, di, ci, ci)
        # the position attention block
        B, Cb, db = L - 1, ch[-1], dims[-1]
        T = _vox(db)
        X, dX = P(ws[f'x{B}']), P(ws[f'dskip{B}'])
        self._bn_bwd(ws, 'pab.out', 'pab.out.bn', P(ws['dz']), Cb, T, N)
        self._conv_bwd(ws, 'pab.out', 'pab.out.conv', 1, P(ws['Y']), Cb * T, P(ws['dY']), Cb * T, N, db, Cb, Cb)
        nv.call('iunet_ma_attn_bwd', self.dt, P(ws['q']), QK * T, nv.ptr(self.p('pab.top.conv.bias')), P(ws['k']), QK * T,
                nv.ptr(self.p('pab.center.conv.bias')), P(ws['v']), Cb * T, P(ws['dY']), Cb * T, nv.ptr(ws['lse']), nv.ptr(ws['delta']),
                P(ws['dq']), QK * T, P(ws['dk']), QK * T, P(ws['dv']), Cb * T, Cb, T, N, s)
        self.g('pab.top.conv.bias').zero_()            # (a row's softmax does not see a term that is constant along it)
        self._bias_grad(ws, ws['dk'], QK, T, N, 'pab.center.conv.bias')
        self._bias_grad(ws, ws['dY'], Cb, T, N, 'pab.bottom.conv.bias')
        self._conv_bwd(ws, 'pab.top', 'pab.top.conv', 0, X, Cb * T, P(ws['dxa']), Cb * T, N, db, Cb, QK, dy=P(ws['dq']))
        self._add(ws, P(ws['dY']), P(ws['dxa']), dX, Cb, db, N)
        self._conv_bwd(ws, 'pab.center', 'pab.center.conv', 0, X, Cb * T, P(ws['dxa']), Cb * T, N, db, Cb, QK, dy=P(ws['dk']))
        self._add(ws, dX, P(ws['dxa']), dX, Cb, db, N)
        self._conv_bwd(ws, 'pab.bottom', 'pab.bottom.conv', 1, X, Cb * T, P(ws['dxa']), Cb * T, N, db, Cb, Cb, dy=P(ws['dv']))
        self._add(ws, dX, P(ws['dxa']), dX, Cb, db, N)
        self._encoder_backward(ws, x, x_strides, N)
