"""Functional CPU reference of the native MA-Net (architecture='MA-Net'), in float64 (or any dtype): the canonical definition.

B = L - 1, Cb = ch[B], T = the voxels of G_B (the tokens), K = 64, up = nearest neighbour x2.
  Q = conv1x1(X^B) + b (pab.top);  Kc = conv1x1(X^B) + b (pab.center);  V = conv3^d(X^B) + b (pab.bottom)
  S[i][j] = sum_k Kc[i][k] Q[j][k] (no 1 / sqrt(K));  A = softmax_j S;  O[i] = sum_j A[i][j] V[j];  Y = X^B + O
  Z = relu(bn(conv3^d(Y))) (pab.out)
  dec{l}, l = B-1 .. 0, on x = Z, then the previous block's output:
    h = relu(bn(conv1x1(relu(bn(conv3^d(x))))))  (hl3: ch[l+1] -> ch[l+1], hl1: ch[l+1] -> ch[l])
    g_s = sigmoid(W2 relu(W1 mean_vox(.) + b1) + b2), s = se_hl on h, se_ll on X^l, m = max(ch[l] / 16, 1)
    u = up(h) (g_hl + g_ll);  the stage conv{1,2} / bn{1,2} on cat[X^l, u]
  logits = the 1x1 head on dec0's output.

act=None runs that order literally.  `act=torch.float16 / torch.bfloat16` rounds where the native 16-bit path rounds:
  * the input and every encoder activation;
  * every operator: the weight (training, and Q / Kc / V always), or the weight times the folded eval-mode BatchNorm scale (eval);
  * the raw outputs of Q, Kc and V (stored without their biases), then Q + b and Kc + b as the attention kernel rounds them on load;
  * P = exp(S - the row's maximum), rounded for the product with V; the row sum is taken of the unrounded P; V's bias enters in
    Y = X + O / sum + b, rounded once (the kernel rounds P against its running maximum: the same rounding up to the block order);
  * training: every raw conv output y (the batch statistics come from the unrounded fp32 sums), then relu(scale y + shift) of the
    ROUNDED y, rounded (the bits of iunet_bn_relu_fwd); eval: relu(acc + bias), rounded;
  * u = up(h) g, rounded once (the gates and the means they read stay in fp32).  The head's logits are not rounded."""
import math

import torch
import torch.nn.functional as F

from tests.upernet_ref import _conv, conv_bn_relu, encoder

BN_EPS = 1e-5
QK = 64


def gate_width(c):
    return max(c // 16, 1)


def param_shapes(dim=2, levels=4, base=32, cin=1, ncls=2):
    ch = [base * 2 ** l for l in range(levels)]
    k3, k1 = (3,) * dim, (1,) * dim
    s = {}

    def bn(prefix, c):
        for k in ('weight', 'bias', 'running_mean', 'running_var'):
            s[f'{prefix}.{k}'] = (c,)

    def conv_bn(prefix, shp):
        s[f'{prefix}.conv.weight'] = shp
        bn(f'{prefix}.bn', shp[0])

    def stage(prefix, a, b):
        for j, (ci, co) in enumerate(((a, b), (b, b)), 1):
            s[f'{prefix}.conv{j}.weight'] = (co, ci) + k3
            bn(f'{prefix}.bn{j}', co)
    for l in range(levels):
        stage(f'enc{l}', cin if l == 0 else ch[l - 1], ch[l])
    Cb = ch[-1]
    for prefix, shp in (('pab.top', (QK, Cb) + k1), ('pab.center', (QK, Cb) + k1), ('pab.bottom', (Cb, Cb) + k3)):
        s[f'{prefix}.conv.weight'] = shp
        s[f'{prefix}.conv.bias'] = (shp[0],)
    conv_bn('pab.out', (Cb, Cb) + k3)
    for l in range(levels - 2, -1, -1):
        m = gate_width(ch[l])
        conv_bn(f'dec{l}.hl3', (ch[l + 1], ch[l + 1]) + k3)
        conv_bn(f'dec{l}.hl1', (ch[l], ch[l + 1]) + k1)
        for se in ('se_hl', 'se_ll'):
            s[f'dec{l}.{se}.fc1.weight'] = (m, ch[l])
            s[f'dec{l}.{se}.fc1.bias'] = (m,)
            s[f'dec{l}.{se}.fc2.weight'] = (ch[l], m)
            s[f'dec{l}.{se}.fc2.bias'] = (ch[l],)
        stage(f'dec{l}', 2 * ch[l], ch[l])
    s['head.weight'] = (ncls, ch[0]) + k1
    s['head.bias'] = (ncls,)
    return s


def init_params(dim=2, levels=4, base=32, cin=1, ncls=2, seed=0, randomize_bn=False, attn_scale=1.0):
    """He-normal conv weights, fan-in scaled gate weights; randomize_bn: random BatchNorm affine pairs / running statistics AND non-zero
    biases everywhere.  attn_scale multiplies the query / key weights (the logits S grow with its square)."""
    g = torch.Generator().manual_seed(seed)
    p = {}
    for k, shp in param_shapes(dim, levels, base, cin, ncls).items():
        if k.endswith('.weight') and len(shp) > 1:
            fan = shp[1] * math.prod(shp[2:])
            p[k] = torch.randn(shp, generator=g) * math.sqrt((1.0 if '.fc' in k else 2.0) / fan)
            if k.startswith(('pab.top.', 'pab.center.')):
                p[k] *= attn_scale
        elif k.endswith('running_var') or k.endswith('weight'):
            p[k] = (0.5 + torch.rand(shp, generator=g)) if randomize_bn else torch.ones(shp)
        elif randomize_bn or k == 'head.bias':
            p[k] = 0.2 * torch.randn(shp, generator=g)
        else:
            p[k] = torch.zeros(shp)
    return p


def attention(Q, Kc, V, r=lambda t: t):
    """(O [N, T, Cb], A [N, T, T]) from Q, Kc [N, T, K] and V [N, T, Cb]; r: P is rounded for the second product, the row sum is taken
    of the unrounded P."""
    S = torch.bmm(Kc, Q.transpose(1, 2))
    P = torch.exp(S - S.max(2, keepdim=True).values)
    l = P.sum(2, keepdim=True)
    return torch.bmm(r(P), V) / l, P / l


def position_attention(p, X, dim, r, rounded):
    """Y = X + A V + b from X^B; rounded: the 16-bit path's stores (the docstring's list)."""
    N, Cb = X.shape[:2]
    tok = lambda t: t.flatten(2).transpose(1, 2)                      # [N, C, *sp] -> [N, T, C]
    raw = lambda prefix: r(_conv(X, r(p[f'{prefix}.conv.weight']), dim)) if rounded else _conv(X, p[f'{prefix}.conv.weight'], dim)
    Q = r(tok(raw('pab.top')) + p['pab.top.conv.bias'])
    Kc = r(tok(raw('pab.center')) + p['pab.center.conv.bias'])
    O, A = attention(Q, Kc, tok(raw('pab.bottom')), r)
    Y = tok(X) + (O + p['pab.bottom.conv.bias'])
    return r(Y.transpose(1, 2).reshape(X.shape)), A.detach()


def gates(p, prefix, h, skip):
    """g[n][c] = sigmoid(se_hl(mean h)) + sigmoid(se_ll(mean skip))."""
    out = 0
    for se, t in (('se_hl', h), ('se_ll', skip)):
        mean = t.flatten(2).mean(2)
        z = torch.relu(F.linear(mean, p[f'{prefix}.{se}.fc1.weight'], p[f'{prefix}.{se}.fc1.bias']))
        out = out + torch.sigmoid(F.linear(z, p[f'{prefix}.{se}.fc2.weight'], p[f'{prefix}.{se}.fc2.bias']))
    return out


def decoder(p, feats, dim, training=False, r=lambda t: t, stats=None, rounded=False, keep=None):
    """dec0's output from the encoder outputs.  keep: a dict that receives the attention weights ('A': [N, T, T])."""
    L = len(feats)
    Y, A = position_attention(p, feats[-1], dim, r, rounded)
    if keep is not None:
        keep['A'] = A
    x = conv_bn_relu(p, 'pab.out', Y, dim, training, r, stats)
    for l in range(L - 2, -1, -1):
        t = conv_bn_relu(p, f'dec{l}.hl3', x, dim, training, r, stats)
        h = conv_bn_relu(p, f'dec{l}.hl1', t, dim, training, r, stats)
        g = gates(p, f'dec{l}', h, feats[l])
        u = r(F.interpolate(h, scale_factor=2, mode='nearest') * g.reshape(g.shape + (1,) * dim))
        x = torch.cat([feats[l], u], 1)
        for j in (1, 2):
            x = conv_bn_relu(p, f'dec{l}', x, dim, training, r, stats, bn=f'bn{j}', conv=f'conv{j}')
    return x


def forward_logits(p, x, dim=2, levels=4, training=False, act=None, dtype=torch.float64, stats=None, keep=None):
    """Full-resolution logits.  training: batch statistics (running ones are left alone; `stats` receives {bn prefix: (mean, unbiased
    var)} for the running-statistics update); act: 16-bit rounding where the native path rounds (the list above)."""
    p = {k: v.to(dtype) for k, v in p.items()}
    r = (lambda t: t.to(act).to(dtype)) if act is not None else (lambda t: t)
    x = x.to(dtype)
    feats = encoder(p, x, dim, levels, training, r, stats)
    d0 = decoder(p, feats, dim, training, r, stats, rounded=act is not None, keep=keep)
    return (F.conv3d if dim == 3 else F.conv2d)(d0, p['head.weight'], p['head.bias'])
