"""float64 / fp32 CPU reference of the nested U-Net (U-Net++, Zhou et al. 2018) on the canonical stage of oracle/unet_ref.py:
X^{i,0} = enc{i}; for j >= 1, i + j <= L - 1: X^{i,j} = stage(concat[X^{i,0}, .., X^{i,j-1}, up(X^{i+1,j-1})]) with parameters
`dec{i}_{j}.*`; the head reads X^{0,L-1}.  The rounding points of `act_dtype` and `training=True` are those of unet_ref.forward_logits.
"""
import math

import torch
import torch.nn.functional as F

from oracle.unet_ref import BN_EPS, _conv, _convT, _pool, _rnd, _rnd_ag, fold_bn


def nodes(levels):
    return [(i, j) for j in range(1, levels) for i in range(levels - j)]


def param_shapes(dim=2, levels=4, base=32, cin=1, ncls=2):
    ch = [base * 2 ** l for l in range(levels)]
    k3, k2, k1 = (3,) * dim, (2,) * dim, (1,) * dim
    shapes = {}

    def stage(prefix, ci, co):
        for j, (a, b) in enumerate(((ci, co), (co, co)), 1):
            shapes[f'{prefix}.conv{j}.weight'] = (b, a) + k3
            for k in ('weight', 'bias', 'running_mean', 'running_var'):
                shapes[f'{prefix}.bn{j}.{k}'] = (b,)
    for l in range(levels):
        stage(f'enc{l}', cin if l == 0 else ch[l - 1], ch[l])
    for i, j in nodes(levels):
        shapes[f'dec{i}_{j}.up.weight'] = (ch[i + 1], ch[i]) + k2
        shapes[f'dec{i}_{j}.up.bias'] = (ch[i],)
        stage(f'dec{i}_{j}', (j + 1) * ch[i], ch[i])
    shapes['head.weight'] = (ncls, ch[0]) + k1
    shapes['head.bias'] = (ncls,)
    return shapes


def init_params(dim=2, levels=4, base=32, cin=1, ncls=2, seed=0, randomize_bn=False):
    """unet_ref.init_params' distributions on the nested names."""
    g = torch.Generator().manual_seed(seed)
    p = {}
    for name, shp in param_shapes(dim, levels, base, cin, ncls).items():
        if name.endswith('conv1.weight') or name.endswith('conv2.weight') or name == 'head.weight':
            p[name] = torch.randn(shp, generator=g) * math.sqrt(2.0 / (shp[1] * math.prod(shp[2:])))
        elif name.endswith('up.weight'):
            p[name] = torch.randn(shp, generator=g) * math.sqrt(1.0 / shp[0])
        elif name.endswith('running_var'):
            p[name] = (0.5 + torch.rand(shp, generator=g)) if randomize_bn else torch.ones(shp)
        elif name.endswith('running_mean'):
            p[name] = (0.2 * torch.randn(shp, generator=g)) if randomize_bn else torch.zeros(shp)
        elif name.endswith('bn1.weight') or name.endswith('bn2.weight'):
            p[name] = (0.75 + 0.5 * torch.rand(shp, generator=g)) if randomize_bn else torch.ones(shp)
        else:
            p[name] = (0.1 * torch.randn(shp, generator=g)) if (randomize_bn or name == 'head.bias') else torch.zeros(shp)
    return p


def forward_logits(p, x, dim=2, levels=4, training=False, act_dtype=None, bn_stats_out=None, dtype=torch.float32):
    """x [N, cin, *spatial] in [0, 1] -> logits [N, ncls, *spatial] in `dtype` (float64: the double reference)."""
    conv, convT, pool = _conv(dim), _convT(dim), _pool(dim)
    p = {k: v.to(dtype) for k, v in p.items()}
    x = _rnd(x.to(dtype), act_dtype).to(dtype)
    R = (lambda t: _rnd_ag(t, act_dtype).to(dtype)) if training else (lambda t: _rnd(t, act_dtype).to(dtype))

    def stage(prefix, t):
        for j in (1, 2):
            w = p[f'{prefix}.conv{j}.weight']
            bn = [p[f'{prefix}.bn{j}.{k}'] for k in ('weight', 'bias', 'running_mean', 'running_var')]
            if training:
                y = R(conv(t, R(w), padding=1))
                dims = [0] + list(range(2, y.dim()))
                mean, var = y.mean(dim=dims), y.var(dim=dims, unbiased=False)
                if bn_stats_out is not None:
                    bn_stats_out[f'{prefix}.bn{j}'] = (mean.detach(), var.detach())
                shape = [1, -1] + [1] * dim
                y = (y - mean.view(shape)) / torch.sqrt(var.view(shape) + BN_EPS) * bn[0].view(shape) + bn[1].view(shape)
                t = R(F.relu(y))
            else:
                wf, bf = fold_bn(w, *bn)
                t = R(F.relu(conv(t, R(wf), bias=bf, padding=1)))
        return t

    X = {}
    t = x
    for l in range(levels):
        t = stage(f'enc{l}', t)
        X[l, 0] = t
        if l < levels - 1:
            t = pool(t, 2)
    for i, j in nodes(levels):
        up = R(convT(X[i + 1, j - 1], R(p[f'dec{i}_{j}.up.weight']), bias=p[f'dec{i}_{j}.up.bias'], stride=2))
        X[i, j] = stage(f'dec{i}_{j}', torch.cat([X[i, k] for k in range(j)] + [up], dim=1))
    return conv(X[0, levels - 1], p['head.weight'], bias=p['head.bias'])


def forward(p, x, dim=2, levels=4, training=False, act_dtype=None, dtype=torch.float32):
    return torch.softmax(forward_logits(p, x, dim, levels, training, act_dtype, dtype=dtype), dim=1)


def to_unet_names(p):
    """L = 2: the nested network is the U-Net; dec0_1 is dec0."""
    return {k.replace('dec0_1.', 'dec0.'): v for k, v in p.items()}
