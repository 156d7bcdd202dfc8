"""Functional CPU reference of the native DeepLabV3 (architecture='DeepLabV3'): smp's DeepLabV3 decoder on the project's encoder, in float64
(or any dtype), with the dropout mask an argument.  `act=torch.float16 / torch.bfloat16` rounds where the native 16-bit forward rounds: the
input, the folded operators, every stored activation (the fp32 pooling branch and the fp32 logits are not rounded)."""
import math

import torch
import torch.nn.functional as F

BN_EPS = 1e-5
BRANCHES = ('aspp.b0', 'aspp.b1', 'aspp.b2', 'aspp.b3')


def param_shapes(dim=2, levels=4, base=32, cin=1, ncls=2, C=256):
    ch = [base * 2 ** l for l in range(levels)]
    k3, k1 = (3,) * dim, (1,) * dim
    s = {}

    def bn(prefix, c):
        for k in ('weight', 'bias', 'running_mean', 'running_var'):
            s[f'{prefix}.{k}'] = (c,)
    for l in range(levels):
        for j, (a, b) in enumerate(((cin if l == 0 else ch[l - 1], ch[l]), (ch[l], ch[l])), 1):
            s[f'enc{l}.conv{j}.weight'] = (b, a) + k3
            bn(f'enc{l}.bn{j}', b)
    for prefix, shp in (('aspp.b0', (C, ch[-1]) + k1), ('aspp.b1', (C, ch[-1]) + k3), ('aspp.b2', (C, ch[-1]) + k3),
                        ('aspp.b3', (C, ch[-1]) + k3), ('aspp.pool', (C, ch[-1]) + k1), ('aspp.project', (C, 5 * C) + k1), ('dec', (C, C) + k3)):
        s[f'{prefix}.conv.weight'] = shp
        bn(f'{prefix}.bn', C)
    s['head.weight'] = (ncls, C) + k1
    s['head.bias'] = (ncls,)
    return s


def init_params(dim=2, levels=4, base=32, cin=1, ncls=2, C=256, seed=0, randomize_bn=False):
    g = torch.Generator().manual_seed(seed)
    p = {}
    for k, shp in param_shapes(dim, levels, base, cin, ncls, C).items():
        if k.endswith('.weight') and len(shp) > 1:
            fan = shp[1] * math.prod(shp[2:])
            p[k] = torch.randn(shp, generator=g) * math.sqrt(2.0 / fan)
        elif k.endswith('running_var') or k.endswith('weight'):
            p[k] = (0.5 + torch.rand(shp, generator=g)) if randomize_bn else torch.ones(shp)
        elif randomize_bn or k == 'head.bias':
            p[k] = 0.2 * torch.randn(shp, generator=g)
        else:
            p[k] = torch.zeros(shp)
    return p


def _conv(x, w, dim, dilation=1):
    k = w.shape[-1]
    pad = dilation * (k // 2)
    return (F.conv3d if dim == 3 else F.conv2d)(x, w, padding=pad, dilation=dilation)


def _bn(y, p, prefix, training, stats):
    if training:
        axes = [0] + list(range(2, y.dim()))
        mean = y.mean(axes)
        var = y.var(axes, unbiased=False)
        if stats is not None:
            n = y.numel() // y.shape[1]
            stats[prefix] = (mean, var * n / max(n - 1, 1))
    else:
        mean, var = p[prefix + '.running_mean'].to(y.dtype), p[prefix + '.running_var'].to(y.dtype)
    sh = (1, -1) + (1,) * (y.dim() - 2)
    return (y - mean.view(sh)) / torch.sqrt(var.view(sh) + BN_EPS) * p[prefix + '.weight'].to(y.dtype).view(sh) + p[prefix + '.bias'].to(y.dtype).view(sh)


def forward_logits(p, x, dim=2, levels=4, rates=(12, 24, 36), training=False, mask=None, p_drop=0.5, act=None, dtype=torch.float64,
                   stats=None):
    """Full-resolution logits.  training: batch statistics (running ones are left alone; `stats` receives {bn prefix: (mean, unbiased
    var)} for the running-statistics update), dropout applied with `mask` ([N, C, *coarse grid], 1 = kept); act: 16-bit rounding."""
    p = {k: v.to(dtype) for k, v in p.items()}
    r = (lambda t: t.to(act).to(dtype)) if act is not None else (lambda t: t)
    relu = torch.relu
    h = r(x.to(dtype))
    for l in range(levels):
        if l > 0:
            h = (F.max_pool3d if dim == 3 else F.max_pool2d)(h, 2)
        for j in (1, 2):
            h = r(relu(_bn(_conv(h, p[f'enc{l}.conv{j}.weight'], dim), p, f'enc{l}.bn{j}', training, stats)))
    X = h
    outs = []
    for b, rate in zip(BRANCHES, (0,) + tuple(rates)):
        w = p[b + '.conv.weight']
        outs.append(r(relu(_bn(_conv(X, w, dim, dilation=max(rate, 1)), p, b + '.bn', training, stats))))
    m = X.mean(dim=tuple(range(2, X.dim())), keepdim=True)
    bp = relu(_bn((F.conv3d if dim == 3 else F.conv2d)(m, p['aspp.pool.conv.weight']), p, 'aspp.pool.bn', training, stats))
    bp = bp.expand_as(outs[0])
    P = relu(_bn((F.conv3d if dim == 3 else F.conv2d)(torch.cat(outs + [bp], 1), p['aspp.project.conv.weight']), p, 'aspp.project.bn',
                 training, stats))
    P = r(P)
    if training and p_drop > 0:
        P = r(P * mask.to(dtype) / (1.0 - p_drop))
    Fe = r(relu(_bn(_conv(P, p['dec.conv.weight'], dim), p, 'dec.bn', training, stats)))
    lc = (F.conv3d if dim == 3 else F.conv2d)(Fe, p['head.weight'], p['head.bias'])
    return F.interpolate(lc, scale_factor=2 ** (levels - 1), mode='trilinear' if dim == 3 else 'bilinear', align_corners=True)
