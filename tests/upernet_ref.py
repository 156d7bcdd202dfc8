"""Functional CPU reference of the native UPerNet (architecture='UPerNet'), in float64 (or any dtype): the canonical definition.

B = L - 1, T = level 2's grid, C = decoder_channels, Cq = ch[B] / 4, R = F.interpolate(size=, bilinear / trilinear, align_corners=False).
  A_s = adaptive_avg_pool(X^B, s), s in (1, 2, 3, 6);  Q_1 = relu(conv1x1(A_1) + bias);  Q_s = relu(bn(conv1x1(A_s))) for s > 1
  U = cat[X^B, R(Q_1), R(Q_2), R(Q_3), R(Q_6)];  P^B = relu(bn(conv3^d(U)))
  P^l = R(P^{l+1}) + relu(bn(conv1x1(X^l))),  l = B-1 .. 2
  V = cat[R(P^B), .., R(P^3), P^2] on T;  F = relu(bn(conv3^d(V)));  logits = x4 upsampling (align_corners=True) of the 1x1 head.

act=None runs that order literally.  `act=torch.float16 / torch.bfloat16` rounds where the native 16-bit path rounds:
  * the input and every encoder activation;
  * A_s (the pooled means are stored in 16 bits);
  * every operator: the weight (training), or the weight times the folded eval-mode BatchNorm scale (eval);
  * training: every raw conv output y (the batch statistics come from the unrounded fp32 sums), then relu(scale y + shift) of the
    ROUNDED y, rounded (the bits of iunet_bn_relu_fwd; the resize kernel's prologue and raw base apply the same); eval: relu(acc + bias);
  * Q_1: relu(y + bias) of the rounded y (training) / relu(acc + bias) (eval), rounded;
  * every resampled tensor (the slots of U and V) and every sum P^l = lateral + R(P^{l+1}) (one rounding of the fp32 sum);
  * P^B and F.  The fp32 coarse logits and everything after them are not rounded."""
import math

import torch
import torch.nn.functional as F

BN_EPS = 1e-5
POOL_SIZES = (1, 2, 3, 6)
T_LEVEL = 2


def _decoder_convs(dim, levels, ch, C):
    k3, k1 = (3,) * dim, (1,) * dim
    Cb = ch[-1]
    return [(f'psp.b{s}', (Cb // 4, Cb) + k1) for s in POOL_SIZES] + [('psp.out', (C, 2 * Cb) + k3)] + \
           [(f'lat{l}', (C, ch[l]) + k1) for l in range(levels - 2, T_LEVEL - 1, -1)] + [('fuse', (C, (levels - 2) * C) + k3)]


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
    for prefix, shp in _decoder_convs(dim, levels, ch, C):
        s[f'{prefix}.conv.weight'] = shp
        if prefix == 'psp.b1':
            s[f'{prefix}.conv.bias'] = (shp[0],)
        else:
            bn(f'{prefix}.bn', shp[0])
    s['head.weight'] = (ncls, C) + k1
    s['head.bias'] = (ncls,)
    return s


def init_params(dim=2, levels=4, base=32, cin=1, ncls=2, C=256, seed=0, randomize_bn=False):
    """He-normal weights; randomize_bn: random BatchNorm affine pairs / running statistics AND a non-zero psp.b1.conv.bias."""
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


def mode(dim):
    return 'trilinear' if dim == 3 else 'bilinear'


def resize(t, size, dim):
    return F.interpolate(t, size=list(size), mode=mode(dim), align_corners=False)


def pool(t, s, dim):
    return (F.adaptive_avg_pool3d if dim == 3 else F.adaptive_avg_pool2d)(t, s)


def _conv(x, w, dim):
    return (F.conv3d if dim == 3 else F.conv2d)(x, w, padding=w.shape[-1] // 2)


def _view(v, t):
    return v.view((1, -1) + (1,) * (t.dim() - 2))


def conv_bn_relu(p, prefix, x, dim, training, r, stats, bn='bn', conv='conv'):
    """r(relu(bn(conv(x)))) with the roundings of the docstring (r the identity: the literal float64 form)."""
    w = p[f'{prefix}.{conv}.weight']
    g, b = p[f'{prefix}.{bn}.weight'], p[f'{prefix}.{bn}.bias']
    if training:
        y = _conv(x, r(w), dim)
        axes = [0] + list(range(2, y.dim()))
        mean, var = y.mean(axes), y.var(axes, unbiased=False)
        if stats is not None:
            n = y.numel() // y.shape[1]
            stats[f'{prefix}.{bn}'] = (mean.detach(), (var * n / max(n - 1, 1)).detach())
        scale = g / torch.sqrt(var + BN_EPS)
        return r(torch.relu(_view(scale, y) * r(y) + _view(b - mean * scale, y)))
    scale = g / torch.sqrt(p[f'{prefix}.{bn}.running_var'] + BN_EPS)
    y = _conv(x, r(w * scale.view((-1,) + (1,) * (w.dim() - 1))), dim)
    return r(torch.relu(y + _view(b - p[f'{prefix}.{bn}.running_mean'] * scale, y)))


def encoder(p, x, dim, levels, training, r, stats):
    h, feats = r(x), []
    for l in range(levels):
        if l > 0:
            h = (F.max_pool3d if dim == 3 else F.max_pool2d)(h, 2)
        for j in (1, 2):
            h = conv_bn_relu(p, f'enc{l}', h, dim, training, r, stats, bn=f'bn{j}', conv=f'conv{j}')
        feats.append(h)
    return feats


def decoder(p, feats, dim, training=False, r=lambda t: t, stats=None):
    """F on T from the encoder outputs."""
    L = len(feats)
    B = L - 1
    X = feats[B]
    gb, gt = X.shape[2:], feats[T_LEVEL].shape[2:]
    parts = [X]
    for s in POOL_SIZES:
        A = r(pool(X, s, dim))
        if s == 1:
            y = _conv(A, r(p['psp.b1.conv.weight']), dim)
            y = r(y) if training else y
            Q = r(torch.relu(y + _view(p['psp.b1.conv.bias'], y)))
        else:
            Q = conv_bn_relu(p, f'psp.b{s}', A, dim, training, r, stats)
        parts.append(r(resize(Q, gb, dim)))
    P = {B: conv_bn_relu(p, 'psp.out', torch.cat(parts, 1), dim, training, r, stats)}
    for l in range(B - 1, T_LEVEL - 1, -1):
        P[l] = r(resize(P[l + 1], feats[l].shape[2:], dim) + conv_bn_relu(p, f'lat{l}', feats[l], dim, training, r, stats))
    V = torch.cat([r(resize(P[l], gt, dim)) for l in range(B, T_LEVEL, -1)] + [P[T_LEVEL]], 1)
    return conv_bn_relu(p, 'fuse', V, dim, training, r, stats)


def forward_logits(p, x, dim=2, levels=4, training=False, act=None, dtype=torch.float64, stats=None):
    """Full-resolution logits.  training: batch statistics (running ones are left alone; `stats` receives {bn prefix: (mean, unbiased
    var)} for the running-statistics update); act: 16-bit rounding where the native path rounds (the list above)."""
    p = {k: v.to(dtype) for k, v in p.items()}
    r = (lambda t: t.to(act).to(dtype)) if act is not None else (lambda t: t)
    x = x.to(dtype)
    feats = encoder(p, x, dim, levels, training, r, stats)
    Fe = decoder(p, feats, dim, training, r, stats)
    lc = (F.conv3d if dim == 3 else F.conv2d)(Fe, p['head.weight'], p['head.bias'])
    return F.interpolate(lc, scale_factor=4, mode=mode(dim), align_corners=True)
