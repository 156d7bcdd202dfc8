"""Functional CPU reference of the native Segformer (architecture='Segformer'): smp's Segformer decoder on the project's encoder, in float64
(or any dtype).  act=None runs smp's literal order (project -> resize -> concat -> fuse -> head -> x4).  `act=torch.float16 / torch.bfloat16`
rounds where the native 16-bit path rounds, which runs the collapsed form Z = sum_l M_l R_l(X^l) + beta: the input, every encoder
activation, the resampled encoder outputs, the operators M_l (with fuse.bn folded in eval), Z (training) and F (the fp32 logits are not
rounded)."""
import math

import torch
import torch.nn.functional as F

BN_EPS = 1e-5


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
    for l in range(levels):
        s[f'mlp{l}.weight'] = (C, ch[l])
        s[f'mlp{l}.bias'] = (C,)
    s['fuse.conv.weight'] = (C, levels * C) + k1
    bn('fuse.bn', C)
    s['head.weight'] = (ncls, C) + k1
    s['head.bias'] = (ncls,)
    return s


def init_params(dim=2, levels=4, base=32, cin=1, ncls=2, C=256, seed=0, randomize_bn=False):
    """He-normal weights; randomize_bn: random BatchNorm affine pairs / running statistics AND non-zero MLP biases (a dropped beta only
    shows then)."""
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


def _conv(x, w, dim):
    k = w.shape[-1]
    return (F.conv3d if dim == 3 else F.conv2d)(x, w, padding=k // 2)


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


def mode(dim):
    return 'trilinear' if dim == 3 else 'bilinear'


def encoder(p, x, dim, levels, training=False, r=lambda t: t, stats=None):
    h, feats = r(x), []
    for l in range(levels):
        if l > 0:
            h = (F.max_pool3d if dim == 3 else F.max_pool2d)(h, 2)
        for j in (1, 2):
            h = r(torch.relu(_bn(_conv(h, p[f'enc{l}.conv{j}.weight'], dim), p, f'enc{l}.bn{j}', training, stats)))
        feats.append(h)
    return feats


def target_size(x):
    return [d // 4 for d in x.shape[2:]]


def resize(t, size, dim):
    return F.interpolate(t, size=size, mode=mode(dim), align_corners=False)


def decoder_literal(p, feats, size, dim):
    """Z in smp's order: project every level, resize to T, concatenate deepest first, fuse (no BatchNorm yet)."""
    L = len(feats)
    outs = []
    for l in range(L - 1, -1, -1):
        P = torch.einsum('kc,nc...->nk...', p[f'mlp{l}.weight'], feats[l]) + p[f'mlp{l}.bias'].view((1, -1) + (1,) * dim)
        outs.append(resize(P, size, dim))
    return (F.conv3d if dim == 3 else F.conv2d)(torch.cat(outs, 1), p['fuse.conv.weight'])


def collapsed_ops(p, L):
    """(M_l for every level, beta) of Z = sum_l M_l R_l(X^l) + beta."""
    C = p['fuse.conv.weight'].shape[0]
    wf = p['fuse.conv.weight'].reshape(C, L * C)
    blk = lambda l: wf[:, (L - 1 - l) * C:(L - l) * C]
    M = [blk(l) @ p[f'mlp{l}.weight'] for l in range(L)]
    beta = sum(blk(l) @ p[f'mlp{l}.bias'] for l in range(L))
    return M, beta


def forward_logits(p, x, dim=2, levels=4, training=False, act=None, dtype=torch.float64, stats=None):
    """Full-resolution logits.  training: batch statistics (running ones are left alone; `stats` receives {bn prefix: (mean, unbiased
    var)} for the running-statistics update); act: 16-bit rounding where the native path rounds (the collapsed form)."""
    p = {k: v.to(dtype) for k, v in p.items()}
    r = (lambda t: t.to(act).to(dtype)) if act is not None else (lambda t: t)
    x = x.to(dtype)
    feats = encoder(p, x, dim, levels, training, r, stats)
    size = target_size(x)
    sh = (1, -1) + (1,) * dim
    if act is None:
        Fe = torch.relu(_bn(decoder_literal(p, feats, size, dim), p, 'fuse.bn', training, stats))
    else:
        M, beta = collapsed_ops(p, levels)
        B = [r(resize(f, size, dim)) for f in feats]
        if training:
            Z = sum(torch.einsum('kc,nc...->nk...', r(M[l]), B[l]) for l in range(levels)) + beta.view(sh)
            Fe = r(torch.relu(_bn(r(Z), p, 'fuse.bn', training, stats)))
        else:
            s = p['fuse.bn.weight'] / torch.sqrt(p['fuse.bn.running_var'] + BN_EPS)
            bias = s * (beta - p['fuse.bn.running_mean']) + p['fuse.bn.bias']
            Z = sum(torch.einsum('kc,nc...->nk...', r(s[:, None] * M[l]), B[l]) for l in range(levels)) + bias.view(sh)
            Fe = r(torch.relu(Z))
    lc = (F.conv3d if dim == 3 else F.conv2d)(Fe, p['head.weight'], p['head.bias'])
    return F.interpolate(lc, scale_factor=4, mode=mode(dim), align_corners=True)
