"""Native 16-bit training step of the U-Net++ (engine_nested.py has the graph and the level-buffer layout), sequenced from Python on
train_engine.TrainEngine's stage helpers, head / loss kernels, flat AdamW, loss scaling and eval_step.

Forward.  The level buffers hold [X^{i,0} | X^{i,1} | ..] as in prediction: node (i, j)'s transposed conv writes up(X^{i+1,j-1}) into
slot j, conv1 reads slots 0..j, conv2's activation overwrites slot j.  conv1's weight gradient needs its input again, so up(.) is
stashed (one ch[i]-channel copy) after conv1 and restored before the node's backward.  The alternative, a concat buffer per node,
would copy X^{i,0..j-1} into every node of the level -- j times the tensor traffic of the stash and that much more memory.

Backward, in reverse topological order (columns j = L-1 .. 1, then the encoder bottom-up).  A node's restore may overwrite
X^{i,j} because every reader of X^{i,j} -- the later nodes of level i and node (i-1, j+1)'s transposed conv -- ran its backward
before.  X^{i,j}'s gradient is the sum of slot j of every later node's conv1 data gradient on its level, the data gradient of the
transposed conv above it and, for the encoder, the max-pool route of the next level's input gradient: with more than one such
consumer, iunet_bn_relu_sum_bwd forms that sum inside the BatchNorm + ReLU backward; with one, the U-Net path runs as it is.

From the second step the whole step is one C call (TrainEngine._handle: TrainHandle over iunet_train_create_nested, csrc/train_net.hip
sequences these launches in C++, bit-identical).  Data parallel: the flat vector is the encoder, then every node, then the head, so the
nodes + head are the tail bucket (all-reduced once the node loop of the backward is done) and enc{L-1} the bottom bucket.
"""
import ctypes

import torch

from . import _native as nv
from . import topology
from .engine import check_spatial
from .train_engine import TrainEngine, _vox
from .unet import nested_nodes


class NestedTrainEngine(TrainEngine):
    nested = True           # (TrainHandle: iunet_train_create_nested)

    def __init__(self, model, lr=None, loss_kind='mcc_ce', betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 loss_scale=None, process_group=None):
        if getattr(model, 'norm', 'batch') != 'batch':
            raise NotImplementedError('U-Net++ training supports BatchNorm only')
        if model.act_dtype not in (torch.float16, torch.bfloat16):
            raise NotImplementedError("U-Net++ training runs with 16-bit activations (act_dtype 'fp16' / 'bf16')")
        self.nodes = nested_nodes(model.levels)
        self.last = f'dec0_{model.levels - 1}'          # X^{0,L-1}: the head's input
        super().__init__(model, lr=lr, loss_kind=loss_kind, betas=betas, eps=eps, weight_decay=weight_decay, loss_scale=loss_scale,
                         process_group=process_group)

    def _first_decoder_param(self):
        return 'dec0_1.up.weight'       # the first node: every node + the head are the data-parallel tail bucket, enc{L-1} the bottom one

    # ------------------------------------------------------------------ graph
    def stage_names(self):
        return topology.nested_stage_names(self.levels)

    def up_convs(self):
        return topology.nested_up_convs(self.levels)

    # ------------------------------------------------------------------ workspace
    def workspace(self, N, D, H, W):
        key = (N, D, H, W)
        ws = self._ws.get(key)
        if ws is not None:
            return ws
        check_spatial(self.dim, self.levels, D, H, W)
        L, ch, lib = self.levels, self.ch, nv.lib()
        dims = topology.level_dims(self.dim, L, D, H, W)
        act = lambda c, v: torch.empty(N * c * v, dtype=self.T, device=self.dev)
        f32 = lambda n: torch.empty(n, dtype=torch.float32, device=self.dev)
        ws = {'dims': dims}
        max_stats, max_wslab, max_bn = 0, 0, 0
        for prefix in self.stage_names():
            ci, co, l = self.stage_io(prefix)
            d, v = dims[l], _vox(dims[l])
            for j, (a, b) in enumerate(((ci, co), (co, co)), 1):
                name = f'{prefix}.conv{j}'
                ws['y.' + name] = act(b, v)
                if j == 1 or name == self.last + '.conv2':      # conv1's activation (where it is materialised), the head's input
                    ws['z.' + name] = act(b, v)
                ws['dz.' + name] = act(b, v) if j == 1 else None
                for k in ('scale', 'shift', 'mean', 'invstd'):
                    ws[f'{k}.{name}'] = f32(b)
                if name == 'enc0.conv1':
                    max_stats = max(max_stats, lib.iunet_conv3_num_tiles(self.dim, N, *d) * b * 2)
                    max_wslab = max(max_wslab, lib.iunet_first_conv_wgrad_blocks(self.dim, N, *d) * b * 112)
                else:
                    max_stats = max(max_stats, max(lib.iunet_conv3_num_tiles(self.dim, N, *d), lib.iunet_conv3_stats_parts(self.dim, N, *d, b, 2)) * b * 2)
                    max_wslab = max(max_wslab, lib.iunet_conv3_wgrad_slab_floats(self.dim, N, *d, a, b))
                max_bn = max(max_bn, lib.iunet_bn_bwd_num_parts(N, v) * b * 2)
        for l in range(L):
            v = _vox(dims[l])
            ws[f'lv{l}'] = act((L - l) * ch[l], v)             # [X^{l,0} | X^{l,1} | ..]
            if l > 0:
                ws[f'pin{l}'] = act(ch[l - 1], v)
                ws[f'dpin{l}'] = act(ch[l - 1], v)
        for i, j in self.nodes:
            node, v, vi = f'dec{i}_{j}', _vox(dims[i]), _vox(dims[i + 1])
            ws['up.' + node] = act(ch[i], v)                    # the stash of up(X^{i+1,j-1})
            ws['dcat.' + node] = act((j + 1) * ch[i], v)        # conv1's data gradient, slot by slot
            ws['dT.' + node] = act(ch[i + 1], vi)               # the transposed conv's data gradient: a source of X^{i+1,j-1}
            nb = lib.iunet_convT_wgrad_blocks(self.dim, N, *dims[i + 1], ch[i + 1], ch[i])
            max_wslab = max(max_wslab, nb * ch[i + 1] * ch[i] * self.npos)
            ws['bslab.' + node] = f32(nb * ch[i])
        v0 = _vox(dims[0])
        ws['dz.last'] = act(ch[0], v0)
        ws['dy'] = act(max(ch[l] * _vox(dims[l]) for l in range(L)), 1)
        ws['stats'] = f32(max_stats)
        ws['wslab'] = f32(max_wslab)
        ws['bnslab'] = f32(max_bn)
        ws['bncoef'] = f32(3 * max(ch))
        nparts = lib.iunet_head_loss_num_parts(N, v0)
        ws['lslab'] = f32(nparts * self.ncls * 8)
        ws['hslab'] = f32(lib.iunet_head_loss_bwd_num_parts(N, v0, self.ncls, ch[0]) * self.ncls * (ch[0] + 1))
        ws['htmp'] = f32(self.ncls * (ch[0] + 1))
        ws['out4'] = f32(4)
        ws['coef'] = f32(self.ncls * 3)
        self._ws = {key: ws}
        return ws

    def _slot(self, ws, t, i, j, slots):
        """(pointer, sample stride) of channel slot j (ch[i] channels) of the level-i tensor ws[t] with `slots` slots per sample."""
        v = _vox(ws['dims'][i])
        return self._P(ws[t], j * self.ch[i] * v), slots * self.ch[i] * v

    def _stash(self, ws, i, j, N, restore=False):
        """Copy up(X^{i+1,j-1}) out of slot j of level i (or back into it)."""
        v = _vox(ws['dims'][i])
        c = self.ch[i] * v
        sl = ws[f'lv{i}'].view(N, self.levels - i, c)[:, j]
        st = ws[f'up.dec{i}_{j}'].view(N, c)
        (sl.copy_(st) if restore else st.copy_(sl))

    # ------------------------------------------------------------------ forward
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
            z0, z0_ss = self._slot(ws, f'lv{l}', l, 0, L - l)
            pool = None
            if l < L - 1:
                do = dims[l + 1]
                pool = (self._P(ws[f'pin{l + 1}']), ch[l] * _vox(do), do)
            self._stage_conv_fwd(ws, f'enc{l}.conv2', x2, ch[l] * v, ch[l], ch[l], l, z0, z0_ss, N, x_act=act, pool=pool)
        for i, j in self.nodes:
            node, v, di = f'dec{i}_{j}', _vox(dims[i]), dims[i + 1]
            src, src_ss = self._slot(ws, f'lv{i + 1}', i + 1, j - 1, L - i - 1)
            cat, cat_ss = self._slot(ws, f'lv{i}', i, 0, L - i)
            up, _ = self._slot(ws, f'lv{i}', i, j, L - i)
            wf, _ = self.pk[node + '.up']
            nv.call('iunet_convT_fwd', self.dt, self.dim, src, src_ss, up, cat_ss, nv.ptr(wf), nv.ptr(self.p(node + '.up.bias')),
                    N, di[0], di[1], di[2], ch[i + 1], ch[i], s)
            x2, act, z1p = self._conv2_input(ws, node, i, N)
            self._stage_conv_fwd(ws, node + '.conv1', cat, cat_ss, (j + 1) * ch[i], ch[i], i, z1p, ch[i] * v, N)
            self._stash(ws, i, j, N)
            if node == self.last:
                # the head's input: with head_act the head kernels apply its BatchNorm + ReLU while loading y (never written)
                z2 = None if self.head_act else (self._P(ws[f'z.{node}.conv2']), ch[0] * v)
            else:
                z2 = (up, cat_ss)
            self._stage_conv_fwd(ws, node + '.conv2', x2, ch[i] * v, ch[i], ch[i], i, None if z2 is None else z2[0],
                                 0 if z2 is None else z2[1], N, x_act=act)
        return ws

    def _head_input(self, ws):
        last = self.last + '.conv2'
        return (ws['y.' + last], last) if self.head_act else (ws['z.' + last], None)

    # ------------------------------------------------------------------ backward
    def _sources(self, ws, i, m):
        """(pointer, sample stride) of every gradient source of X^{i,m} except the max-pool route, in a fixed order: slot m of the
        conv1 data gradient of nodes (i, m+1), (i, m+2), .., then the transposed conv of node (i-1, m+1)."""
        L = self.levels
        out = [self._slot(ws, f'dcat.dec{i}_{jj}', i, m, jj + 1) for jj in range(m + 1, L - i)]
        if i >= 1:
            out.append((self._P(ws[f'dT.dec{i - 1}_{m + 1}']), self.ch[i] * _vox(ws['dims'][i])))
        return out

    def _node_conv2_bwd(self, ws, stage, i, m, N, pool_bwd=None, dy_ready=False):
        """conv2 backward of the stage producing X^{i,m}: its BatchNorm + ReLU backward from the summed gradient, then the weight
        and data gradients (the data gradient also takes conv1's BatchNorm-backward sums where that fusion applies)."""
        L, ch = self.levels, self.ch
        d, v = ws['dims'][i], _vox(ws['dims'][i])
        name = stage + '.conv2'
        x2, act, _ = self._conv2_input(ws, stage, i, N)
        dz1 = self._P(ws[f'dz.{stage}.conv1'])
        if dy_ready:
            dz_ptr, dz_ss = None, 0
        else:
            srcs = self._sources(ws, i, m)
            if len(srcs) + (pool_bwd is not None) == 1:          # one consumer: the U-Net path
                dz_ptr, dz_ss = srcs[0]
            else:
                bn = stage + '.bn2'
                dp_ptr, dp_ss = (pool_bwd[0], pool_bwd[1]) if pool_bwd is not None else (None, 0)
                nv.call('iunet_bn_relu_sum_bwd', self.dt, self.dim, len(srcs),
                        (ctypes.c_void_p * len(srcs))(*[p for p, _ in srcs]), nv.ll_array([ss for _, ss in srcs]), dp_ptr, dp_ss,
                        self._P(ws['y.' + name]), ch[i] * v, self._P(ws['dy']), ch[i] * v, nv.ptr(ws['mean.' + name]),
                        nv.ptr(ws['invstd.' + name]), nv.ptr(self.p(bn + '.weight')), nv.ptr(ws['scale.' + name]),
                        nv.ptr(ws['shift.' + name]), nv.ptr(self.g(bn + '.weight')), nv.ptr(self.g(bn + '.bias')),
                        nv.ptr(ws['bnslab']), nv.ptr(ws['bncoef']), ch[i], N, d[0], d[1], d[2], nv.stream())
                dz_ptr, dz_ss, dy_ready = None, 0, True
        self._stage_conv_bwd(ws, name, dz_ptr, dz_ss, None, ch[i] * v, x2, ch[i] * v, ch[i], ch[i], i, dz1, ch[i] * v, N,
                             x_act=act, feeds=stage + '.conv1', dy_ready=dy_ready)

    def backward(self, ws, x, x_strides, y, w, tdt, N):
        L, ch, dims = self.levels, self.ch, ws['dims']
        s = nv.stream()
        v0 = _vox(dims[0])
        last = self.last + '.conv2'
        dfeat = ws['dz.last']
        nparts = nv.lib().iunet_head_loss_bwd_num_parts(N, v0, self.ncls, ch[0])
        head_dy = False
        if self.head_bn and nv.lib().iunet_head_bn_bwd_ok(ch[0], self.ncls):
            # head backward + the last node's conv2 BatchNorm backward in two passes over its raw output
            bn = self.last + '.bn2'
            nv.call('iunet_head_bn_bwd', self.dt, self._P(ws['y.' + last]), ch[0] * v0, ch[0], nv.ptr(self.p('head.weight')),
                    nv.ptr(self.p('head.bias')), self.ncls, nv.ptr(y), nv.ptr(w), tdt, nv.ptr(ws['coef']), 0.0, nv.ptr(self.state),
                    nv.ptr(ws['scale.' + last]), nv.ptr(ws['shift.' + last]), nv.ptr(ws['mean.' + last]), nv.ptr(ws['invstd.' + last]),
                    nv.ptr(self.p(bn + '.weight')), nv.ptr(self.g(bn + '.weight')), nv.ptr(self.g(bn + '.bias')), self._P(ws['dy']), ch[0] * v0,
                    nv.ptr(ws['hslab']), nv.ptr(ws['bnslab']), nv.ptr(ws['bncoef']), self._P(dfeat), N, v0, s)
            head_dy = True
        elif self.head_act:
            nv.call('iunet_head_loss_bwd_dev', self.dt, self._P(ws['y.' + last]), ch[0] * v0, ch[0], nv.ptr(self.p('head.weight')),
                    nv.ptr(self.p('head.bias')), self.ncls, nv.ptr(y), nv.ptr(w), tdt, nv.ptr(ws['coef']),
                    nv.ptr(self.state), self._P(dfeat), ch[0] * v0, nv.ptr(ws['hslab']), nv.ptr(ws['scale.' + last]),
                    nv.ptr(ws['shift.' + last]), N, v0, s)
        else:
            nv.call('iunet_head_loss_bwd_dev', self.dt, self._P(ws['z.' + last]), ch[0] * v0, ch[0], nv.ptr(self.p('head.weight')),
                    nv.ptr(self.p('head.bias')), self.ncls, nv.ptr(y), nv.ptr(w), tdt, nv.ptr(ws['coef']),
                    nv.ptr(self.state), self._P(dfeat), ch[0] * v0, nv.ptr(ws['hslab']), None, None, N, v0, s)
        nv.call('iunet_reduce_slab', nv.ptr(ws['hslab']), nparts, self.ncls * (ch[0] + 1), nv.ptr(ws['htmp']), 1.0, 0, s)
        nv.call('iunet_head_grad_scatter', nv.ptr(ws['htmp']), nv.ptr(self.g('head.weight')), nv.ptr(self.g('head.bias')), self.ncls, ch[0], s)
        for i, j in reversed(self.nodes):
            node, v, di, vi = f'dec{i}_{j}', _vox(dims[i]), dims[i + 1], _vox(dims[i + 1])
            if node == self.last and not head_dy:
                x2, act, _ = self._conv2_input(ws, node, i, N)
                self._stage_conv_bwd(ws, last, self._P(dfeat), ch[0] * v, None, ch[0] * v, x2, ch[0] * v, ch[0], ch[0], 0,
                                     self._P(ws[f'dz.{node}.conv1']), ch[0] * v, N, x_act=act, feeds=node + '.conv1')
            else:
                self._node_conv2_bwd(ws, node, i, j, N, dy_ready=node == self.last)
            self._stash(ws, i, j, N, restore=True)
            cat, cat_ss = self._slot(ws, f'lv{i}', i, 0, L - i)
            dcat, dcat_ss = self._P(ws['dcat.' + node]), (j + 1) * ch[i] * v
            self._stage_conv_bwd(ws, node + '.conv1', self._P(ws[f'dz.{node}.conv1']), ch[i] * v, None, ch[i] * v, cat, cat_ss,
                                 (j + 1) * ch[i], ch[i], i, dcat, dcat_ss, N)
            # transposed conv: weight / bias gradient and the data gradient of X^{i+1,j-1}
            src, src_ss = self._slot(ws, f'lv{i + 1}', i + 1, j - 1, L - i - 1)
            dup, _ = self._slot(ws, 'dcat.' + node, i, j, j + 1)
            nv.call('iunet_convT_wgrad', self.dt, self.dim, src, src_ss, dup, dcat_ss, nv.ptr(ws['wslab']), nv.ptr(ws['bslab.' + node]),
                    nv.ptr(self.g(node + '.up.weight')), nv.ptr(self.g(node + '.up.bias')), N, di[0], di[1], di[2], ch[i + 1], ch[i], s)
            _, wd = self.pk[node + '.up']
            nv.call('iunet_convT_dgrad', self.dt, self.dim, dup, dcat_ss, self._P(ws['dT.' + node]), ch[i + 1] * vi,
                    nv.ptr(wd), N, di[0], di[1], di[2], ch[i + 1], ch[i], s)
        # data parallel: every node's and the head's gradients are final -- their all-reduce runs while the encoder backward computes
        if self.pg is not None:
            self.buckets.start_tail()
        for l in range(L - 1, -1, -1):
            v = _vox(dims[l])
            pool_bwd = None
            if l < L - 1:
                do = dims[l + 1]
                pool_bwd = (self._P(ws[f'dpin{l + 1}']), ch[l] * _vox(do), do)
            srcs = self._sources(ws, l, 0)
            if len(srcs) == 1 and pool_bwd is None:
                self._node_conv2_bwd(ws, f'enc{l}', l, 0, N)
            elif len(srcs) == 0:                     # (only the max-pool: not a node of this graph, L >= 2)
                raise AssertionError('encoder stage without a decoder consumer')
            else:
                self._node_conv2_bwd(ws, f'enc{l}', l, 0, N, pool_bwd=pool_bwd)
            dz1 = self._P(ws[f'dz.enc{l}.conv1'])
            if l == 0:
                self._stage_conv_bwd(ws, 'enc0.conv1', dz1, ch[0] * v, None, ch[0] * v, None, 0, self.cin, ch[0], 0, None, 0, N,
                                     x_raw=(x, x_strides))
            else:
                self._stage_conv_bwd(ws, f'enc{l}.conv1', dz1, ch[l] * v, None, ch[l] * v, self._P(ws[f'pin{l}']), ch[l - 1] * v,
                                     ch[l - 1], ch[l], l, self._P(ws[f'dpin{l}']), ch[l - 1] * v, N)
            if l == L - 1 and self.pg is not None and self._bottom_start is not None:
                self.buckets.start(self._bottom_start, self._dec_start)

    # ------------------------------------------------------------------ public steps (TrainEngine.train_step / step_forward)
    def train_loss_forward(self, ws, y, w, N, vox):
        feat, act = self._head_input(ws)
        return self.loss_forward(ws, feat, y, w, N, vox, act=act)
