"""float64 / fp32 CPU reference of the LinkNet (Chaurasia & Culurciello 2017, smp's Linknet decoder) on the canonical encoder of
oracle/unet_ref.py: X^l = enc{l}, D^{L-1} = X^{L-1}; for l = L-2 .. 0, with m = ch[l+1] / 4,
  a1 = relu(bn1(conv1x1(D^{l+1}))), a2 = relu(bn2(convT k4 s2 p1(a1))), D^l = relu(bn3(conv1x1(a2))) + X^l;
the head reads D^0.  No conv bias in the decoder, no "prefinal" block (the encoder's enc0 is at full resolution).

16-bit rounding points (act_dtype), where the native kernels store a tensor:
  - eval (folded BatchNorm): the operators (w * gamma / sqrt(var + eps)), every encoder activation, a1, a2 and D^l = round(relu(conv +
    bias) + X^l) -- the skip is added in fp32 before the one rounding;
  - training: the raw conv outputs y1, y2, y3 (statistics of the unrounded values are close to the rounded ones'), a1 and a2 as
    relu(bn(round(y))) rounded (the loaders of the next conv apply them: iunet_bn_relu_fwd's bits) and D^l = round(relu(bn3(y3)) + X^l).
The encoder's rounding points are unet_ref.forward_logits'.
"""
import math

import torch
import torch.nn.functional as F

from oracle.unet_ref import BN_EPS, _conv, _convT, _pool, _rnd, _rnd_ag, fold_bn


def param_shapes(dim=2, levels=4, base=32, cin=1, ncls=2):
    ch = [base * 2 ** l for l in range(levels)]
    k3, k4, k1 = (3,) * dim, (4,) * dim, (1,) * dim
    shapes = {}
    for l in range(levels):
        ci = cin if l == 0 else ch[l - 1]
        for j, (a, b) in enumerate(((ci, ch[l]), (ch[l], ch[l])), 1):
            shapes[f'enc{l}.conv{j}.weight'] = (b, a) + k3
            for k in ('weight', 'bias', 'running_mean', 'running_var'):
                shapes[f'enc{l}.bn{j}.{k}'] = (b,)
    for l in range(levels - 2, -1, -1):
        m = ch[l + 1] // 4
        for key, shp, bn, c in (('conv1', (m, ch[l + 1]) + k1, 'bn1', m), ('up', (m, m) + k4, 'bn2', m), ('conv2', (ch[l], m) + k1, 'bn3', ch[l])):
            shapes[f'dec{l}.{key}.weight'] = shp
            for k in ('weight', 'bias', 'running_mean', 'running_var'):
                shapes[f'dec{l}.{bn}.{k}'] = (c,)
    shapes['head.weight'] = (ncls, ch[0]) + k1
    shapes['head.bias'] = (ncls,)
    return shapes


def init_params(dim=2, levels=4, base=32, cin=1, ncls=2, seed=0, randomize_bn=False):
    """unet_ref.init_params' distributions on the LinkNet names."""
    g = torch.Generator().manual_seed(seed)
    p = {}
    for name, shp in param_shapes(dim, levels, base, cin, ncls).items():
        if name.endswith('conv1.weight') or name.endswith('conv2.weight') or name == 'head.weight':
            p[name] = torch.randn(shp, generator=g) * math.sqrt(2.0 / (shp[1] * math.prod(shp[2:])))
        elif name.endswith('up.weight'):
            p[name] = torch.randn(shp, generator=g) * math.sqrt(2.0 / (shp[0] * 2 ** dim))
        elif name.endswith('running_var'):
            p[name] = (0.5 + torch.rand(shp, generator=g)) if randomize_bn else torch.ones(shp)
        elif name.endswith('running_mean'):
            p[name] = (0.2 * torch.randn(shp, generator=g)) if randomize_bn else torch.zeros(shp)
        elif name.endswith('bn1.weight') or name.endswith('bn2.weight') or name.endswith('bn3.weight'):
            p[name] = (0.75 + 0.5 * torch.rand(shp, generator=g)) if randomize_bn else torch.ones(shp)
        else:
            p[name] = (0.1 * torch.randn(shp, generator=g)) if (randomize_bn or name == 'head.bias') else torch.zeros(shp)
    return p


def fold_bn_T(w, gamma, beta, mean, var):
    """Eval-mode BatchNorm folded into a bias-free ConvTranspose (weights [Cin][Cout][k..]: the scale is per dim 1)."""
    a = gamma / torch.sqrt(var + BN_EPS)
    return w * a.view(1, -1, *([1] * (w.dim() - 2))), beta - mean * a


def forward_logits(p, x, dim=2, levels=4, training=False, act_dtype=None, bn_stats_out=None, dtype=torch.float32):
    """x [N, cin, *spatial] in [0, 1] -> logits [N, ncls, *spatial] in `dtype` (float64: the double reference)."""
    conv, convT, pool = _conv(dim), _convT(dim), _pool(dim)
    p = {k: v.to(dtype) for k, v in p.items()}
    x = _rnd(x.to(dtype), act_dtype).to(dtype)
    R = (lambda t: _rnd_ag(t, act_dtype).to(dtype)) if training else (lambda t: _rnd(t, act_dtype).to(dtype))
    shape = [1, -1] + [1] * dim

    def bn_train(y, name, bn):
        dims = [0] + list(range(2, y.dim()))
        mean, var = y.mean(dim=dims), y.var(dim=dims, unbiased=False)
        if bn_stats_out is not None:
            bn_stats_out[name] = (mean.detach(), var.detach())
        return (y - mean.view(shape)) / torch.sqrt(var.view(shape) + BN_EPS) * bn[0].view(shape) + bn[1].view(shape)

    def bnp(name):
        return [p[f'{name}.{k}'] for k in ('weight', 'bias', 'running_mean', 'running_var')]

    def stage(prefix, t):
        for j in (1, 2):
            w, bn = p[f'{prefix}.conv{j}.weight'], bnp(f'{prefix}.bn{j}')
            if training:
                y = R(conv(t, R(w), padding=1))
                t = R(F.relu(bn_train(y, f'{prefix}.bn{j}', bn)))
            else:
                wf, bf = fold_bn(w, *bn)
                t = R(F.relu(conv(t, R(wf), bias=bf, padding=1)))
        return t

    X = []
    t = x
    for l in range(levels):
        t = stage(f'enc{l}', t)
        X.append(t)
        if l < levels - 1:
            t = pool(t, 2)
    D = X[levels - 1]
    for l in range(levels - 2, -1, -1):
        w1, wu, w2 = p[f'dec{l}.conv1.weight'], p[f'dec{l}.up.weight'], p[f'dec{l}.conv2.weight']
        if training:
            a1 = R(F.relu(bn_train(R(conv(D, R(w1))), f'dec{l}.bn1', bnp(f'dec{l}.bn1'))))
            a2 = R(F.relu(bn_train(R(convT(a1, R(wu), stride=2, padding=1)), f'dec{l}.bn2', bnp(f'dec{l}.bn2'))))
            D = R(F.relu(bn_train(R(conv(a2, R(w2))), f'dec{l}.bn3', bnp(f'dec{l}.bn3'))) + X[l])
        else:
            wf1, bf1 = fold_bn(w1, *bnp(f'dec{l}.bn1'))
            wfu, bfu = fold_bn_T(wu, *bnp(f'dec{l}.bn2'))
            wf2, bf2 = fold_bn(w2, *bnp(f'dec{l}.bn3'))
            a1 = R(F.relu(conv(D, R(wf1), bias=bf1)))
            a2 = R(F.relu(convT(a1, R(wfu), bias=bfu, stride=2, padding=1)))
            D = R(F.relu(conv(a2, R(wf2), bias=bf2)) + X[l])
    return conv(D, p['head.weight'], bias=p['head.bias'])


def forward(p, x, dim=2, levels=4, training=False, act_dtype=None, dtype=torch.float32):
    return torch.softmax(forward_logits(p, x, dim, levels, training, act_dtype, dtype=dtype), dim=1)
