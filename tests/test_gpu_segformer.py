"""Segformer on the MI355X: the kernels of csrc/segformer.hip against float64 torch, the forwards against the CPU reference, one training
step against CPU autograd, and the public interface."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import unet_ref, metrics_ref
from tests import segformer_ref as ref

pytestmark = pytest.mark.gpu

CODE = {torch.float16: 0, torch.bfloat16: 1, torch.float32: 2}


def _blocked(t, T):
    """[N, C, *sp] -> [N, C/8, *sp, 8] contiguous in T (NHWC8c)."""
    N, C = t.shape[:2]
    sp = t.shape[2:]
    t = t.reshape(N, C // 8, 8, *sp)
    return t.permute(0, 1, *range(3, 3 + len(sp)), 2).contiguous().to(T)


def _unblocked(b, C, sp):
    N = b.shape[0]
    b = b.reshape(N, C // 8, *sp, 8)
    return b.permute(0, 1, 2 + len(sp), *range(2, 2 + len(sp))).reshape(N, C, *sp)


def _store(t, T):
    """The kernel layout of a float tensor: NHWC8c for 16-bit, planar for fp32."""
    return (_blocked(t, T) if T != torch.float32 else t.float().contiguous()).cuda()


def _load(b, T, C, sp):
    b = b.cpu().reshape(-1, C * int(np.prod(sp)))
    return (_unblocked(b, C, sp) if T != torch.float32 else b.reshape(-1, C, *sp)).double()


def _model(dim=2, levels=4, base=32, ncls=2, **kw):
    from interactive_unet.unet import UNet
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return UNet(architecture='Segformer', num_classes=ncls, dim=dim, levels=levels, base=base, pretrained=False, **kw)


def _dims(sp):
    return tuple(sp) if len(sp) == 3 else (1,) + tuple(sp)


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _rnd(T):
    return (lambda t: t) if T == torch.float32 else (lambda t: t.to(T).double())


# ---------------------------------------------------------------------------------------------- 1. the kernels
# (nd, T grid, [(source grid, channels)]): every resize ratio -2 .. +3, odd and non-square grids, axes of size 1 and 2
GEMM_CASES = [
    (2, (5, 7), [((20, 28), 32), ((10, 14), 64), ((5, 7), 32), ((3, 4), 32), ((2, 2), 64), ((1, 1), 32)]),
    (2, (6, 3), [((24, 12), 32), ((12, 6), 32), ((6, 3), 64), ((3, 2), 32)]),
    (3, (3, 5, 2), [((12, 20, 8), 32), ((6, 10, 4), 32), ((3, 5, 2), 64), ((2, 3, 1), 32), ((1, 2, 1), 32), ((1, 1, 1), 32)]),
    (3, (4, 2, 6), [((16, 8, 24), 32), ((8, 4, 12), 64), ((4, 2, 6), 32)]),
]


def _sources(nd, srcs, N, T, act, seed):
    g = torch.Generator().manual_seed(seed)
    xs, scs, shs, keep, B = [], [], [], [], []
    for sp, c in srcs:
        sp = sp if nd == 3 else sp
        x = torch.randn((N, c) + tuple(sp), generator=g, dtype=torch.float64)
        xr = _rnd(T)(x)
        keep.append(_store(xr, T))
        if act:
            sc, sh = 0.5 + torch.rand(c, generator=g), 0.3 * torch.randn(c, generator=g)
            scs.append(sc.cuda())
            shs.append(sh.cuda())
            shp = (1, -1) + (1,) * len(sp)
            xr = _rnd(T)(torch.relu(sc.double().view(shp) * xr + sh.double().view(shp)))
        xs.append(xr)
    return xs, keep, scs, shs


def _tables(nd, srcs, keep, N):
    dims = [_dims(sp) for sp, _ in srcs]
    vox = [d[0] * d[1] * d[2] for d in dims]
    from interactive_unet import _native as nv
    return (nv.ptr_array(keep), nv.ll_array([c * v for (_, c), v in zip(srcs, vox)]), nv.int_array([c for _, c in srcs]),
            nv.int_array([e for d in dims for e in d]))


@pytest.mark.parametrize('T', [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize('case', range(len(GEMM_CASES)))
@pytest.mark.parametrize('act', [False, True])
def test_gather_gemm(T, case, act):
    from interactive_unet import _native as nv
    nd, tsp, srcs = GEMM_CASES[case]
    N, Cout = 2, 48
    xs, keep, scs, shs = _sources(nd, srcs, N, T, act, seed=case)
    K = sum(c for _, c in srcs)
    g = torch.Generator().manual_seed(100 + case)
    M = _rnd(T)(torch.randn((Cout, K), generator=g, dtype=torch.float64) / K ** 0.5)
    bias = torch.randn(Cout, generator=g, dtype=torch.float64)
    B = torch.cat([_rnd(T)(F.interpolate(x, size=list(tsp), mode=ref.mode(nd), align_corners=False)) for x in xs], 1)
    want = torch.einsum('ok,nk...->no...', M, B) + bias.view((1, -1) + (1,) * nd)
    D, H, W = _dims(tsp)
    vt = D * H * W
    mk = (M.to(T) if T != torch.float32 else M.float()).contiguous().cuda()
    tabs = _tables(nd, srcs, keep, N)
    sc = nv.ptr_array(scs) if act else None
    sh = nv.ptr_array(shs) if act else None
    parts = nv.lib().iunet_sf_stats_parts(N, D, H, W)
    bk = bias.float().cuda()
    for epi in (0, 1):
        y = torch.zeros(N * Cout * vt, dtype=T, device='cuda')
        stats = torch.zeros(parts * Cout * 2, device='cuda') if epi == 0 else None
        nv.call('iunet_sf_gemm', CODE[T], nd, len(srcs), *tabs, sc, sh, _P(mk), _P(bk), _P(y), Cout * vt,
                _P(stats) if stats is not None else None, epi, N, D, H, W, Cout, nv.stream())
        torch.cuda.synchronize()
        got = _load(y, T, Cout, tsp)
        exp = want if epi == 0 else torch.relu(want)
        tol = (1e-5 if T == torch.float32 else 8e-3 if T == torch.float16 else 6e-2) * max(1.0, exp.abs().max().item())
        err = (got - exp).abs().max().item()
        print(f'{T} nd={nd} case {case} act={act} epi={epi}: max err {err:.2e} (tol {tol:.1e})')
        assert err <= tol
        if epi == 0:
            st = stats.cpu().double().reshape(parts, Cout, 2).sum(0)
            axes = (0,) + tuple(range(2, 2 + nd))
            assert torch.allclose(st[:, 0], want.sum(axes), rtol=1e-3, atol=1e-3 * vt * N)
            assert torch.allclose(st[:, 1], (want * want).sum(axes), rtol=1e-3, atol=1e-3 * vt * N)


@pytest.mark.parametrize('T', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('case', [0, 2, 3])
def test_wgrad(T, case):
    from interactive_unet import _native as nv
    nd, tsp, srcs = GEMM_CASES[case]
    N, Cout = 2, 96
    xs, keep, _, _ = _sources(nd, srcs, N, T, False, seed=case + 7)
    K = sum(c for _, c in srcs)
    D, H, W = _dims(tsp)
    vt = D * H * W
    dz = _rnd(T)(torch.randn((N, Cout) + tuple(tsp), generator=torch.Generator().manual_seed(3), dtype=torch.float64))
    B = torch.cat([_rnd(T)(F.interpolate(x, size=list(tsp), mode=ref.mode(nd), align_corners=False)) for x in xs], 1)
    want = torch.einsum('nc...,nk...->ck', dz, B)
    slab = torch.empty(nv.lib().iunet_sf_wgrad_slab_floats(N, D, H, W, K, Cout), device='cuda')
    G = torch.empty(Cout * K, device='cuda')
    dzb = _store(dz, T)
    nv.call('iunet_sf_wgrad', CODE[T], nd, len(srcs), *_tables(nd, srcs, keep, N), None, None, _P(dzb), Cout * vt, _P(slab), _P(G),
            N, D, H, W, Cout, nv.stream())
    torch.cuda.synchronize()
    err = (G.cpu().double().reshape(Cout, K) - want).abs().max().item()
    print(f'{T} wgrad case {case}: max err {err:.2e}')
    # (the kernel interpolates in fp32, the reference in float64: a resampled value may round to the neighbouring 16-bit number)
    assert err <= (2e-3 if T == torch.float16 else 1.6e-2) * max(1.0, want.abs().max().item())
    G2 = torch.empty_like(G)
    nv.call('iunet_sf_wgrad', CODE[T], nd, len(srcs), *_tables(nd, srcs, keep, N), None, None, _P(dzb), Cout * vt, _P(slab), _P(G2),
            N, D, H, W, Cout, nv.stream())
    torch.cuda.synchronize()
    assert torch.equal(G, G2)


@pytest.mark.parametrize('T', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('nd,tsp,ssp', [(2, (5, 7), (20, 28)), (2, (5, 7), (10, 14)), (2, (6, 3), (6, 3)), (2, (8, 6), (1, 2)),
                                        (2, (16, 24), (2, 3)), (2, (24, 16), (3, 2)), (3, (3, 5, 2), (12, 20, 8)),
                                        (3, (8, 4, 16), (2, 1, 2)), (3, (16, 8, 8), (2, 1, 1)), (3, (4, 6, 2), (2, 3, 1))])
def test_adjoint(T, nd, tsp, ssp):
    from interactive_unet import _native as nv
    N, C = 2, 16
    u = _rnd(T)(torch.randn((N, C) + tsp, generator=torch.Generator().manual_seed(1), dtype=torch.float64))
    x = torch.zeros((N, C) + ssp, dtype=torch.float64, requires_grad=True)
    (F.interpolate(x, size=list(tsp), mode=ref.mode(nd), align_corners=False) * u).sum().backward()
    want = x.grad
    Dt, Ht, Wt = _dims(tsp)
    Ds, Hs, Ws = _dims(ssp)
    dx = torch.empty(N * C * Ds * Hs * Ws, dtype=T, device='cuda')
    ub = _store(u, T)
    nv.call('iunet_sf_adjoint', CODE[T], nd, _P(ub), C * Dt * Ht * Wt, Dt, Ht, Wt, _P(dx), C * Ds * Hs * Ws, Ds, Hs, Ws, C, N,
            nv.stream())
    torch.cuda.synchronize()
    got = _load(dx, T, C, ssp)
    err = (got - want).abs().max().item()
    tol = (2 ** -10 if T == torch.float16 else 2 ** -7) * max(1.0, want.abs().max().item())
    print(f'{T} adjoint {tsp} <- {ssp}: max err {err:.2e}')
    assert err <= tol


@pytest.mark.parametrize('L,C', [(4, 64), (3, 32), (6, 32)])
def test_param_grads_and_pack(L, C):
    from interactive_unet import _native as nv
    g = torch.Generator().manual_seed(L)
    ch = [32 * 2 ** l for l in range(L)]
    N = 3
    K = sum(ch)
    p = {'fuse.conv.weight': torch.randn((C, L * C), generator=g, dtype=torch.float64) / (L * C) ** 0.5}
    for l in range(L):
        p[f'mlp{l}.weight'] = torch.randn((C, ch[l]), generator=g, dtype=torch.float64) / ch[l] ** 0.5
        p[f'mlp{l}.bias'] = torch.randn(C, generator=g, dtype=torch.float64)
    G = torch.randn((C, K), generator=g, dtype=torch.float64)
    rs = torch.randn((N, C), generator=g, dtype=torch.float64)
    pr = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    M, beta = ref.collapsed_ops(pr, L)
    offs = [sum(ch[:l]) for l in range(L)]
    (sum((M[l] * G[:, offs[l]:offs[l] + ch[l]]).sum() for l in range(L)) + (beta * rs.sum(0)).sum()).backward()
    dev = {k: v.float().cuda() for k, v in p.items()}
    Gd, rsd = G.float().cuda(), rs.float().cuda()
    grads = {k: torch.full_like(v, float('nan')) for k, v in dev.items()}
    ws = nv.ptr_array([dev[f'mlp{l}.weight'] for l in range(L)])
    bs = nv.ptr_array([dev[f'mlp{l}.bias'] for l in range(L)])
    nv.call('iunet_sf_param_grads', L, C, nv.int_array(ch), _P(dev['fuse.conv.weight']), ws, bs, _P(Gd), _P(rsd), N,
            nv.ptr_array([grads[f'mlp{l}.weight'] for l in range(L)]), nv.ptr_array([grads[f'mlp{l}.bias'] for l in range(L)]),
            _P(grads['fuse.conv.weight']), nv.stream())
    # the operators: unfolded M / M^T / beta, and the eval fold
    Mk = torch.empty(C * K, device='cuda')
    MT = torch.empty(K * C, device='cuda')
    bk = torch.empty(C, device='cuda')
    nv.call('iunet_sf_pack', 2, L, C, nv.int_array(ch), _P(dev['fuse.conv.weight']), ws, bs, None, None, None, None, 0.0, _P(Mk), _P(MT),
            _P(bk), nv.stream())
    gam, bnb, mean, var = 0.5 + torch.rand(C, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    Mf = torch.empty(C * K, dtype=torch.float16, device='cuda')
    bn = [t.cuda() for t in (gam, bnb, mean, var)]
    bf = torch.empty(C, device='cuda')
    nv.call('iunet_sf_pack', 0, L, C, nv.int_array(ch), _P(dev['fuse.conv.weight']), ws, bs, _P(bn[0]), _P(bn[1]), _P(bn[2]),
            _P(bn[3]), 1e-5, _P(Mf), None, _P(bf), nv.stream())
    torch.cuda.synchronize()
    for k in p:
        err = (grads[k].cpu().double() - pr[k].grad).abs().max().item()
        assert err <= 1e-4 * max(1.0, pr[k].grad.abs().max().item()), (k, err)
    Mcat = torch.cat([m.detach() for m in M], 1)
    assert (Mk.cpu().double().reshape(C, K) - Mcat).abs().max().item() <= 1e-5
    assert (MT.cpu().double().reshape(K, C) - Mcat.t()).abs().max().item() <= 1e-5
    assert (bk.cpu().double() - beta.detach()).abs().max().item() <= 1e-5
    s = gam.double() / torch.sqrt(var.double() + 1e-5)
    assert (Mf.cpu().double().reshape(C, K) - s[:, None] * Mcat).abs().max().item() <= 2e-3 * Mcat.abs().max().item() * s.max().item()
    assert (bf.cpu().double() - (s * (beta.detach() - mean.double()) + bnb.double())).abs().max().item() <= 1e-4


# ---------------------------------------------------------------------------------------------- 2. forwards
def _margin_ok(cls, r):
    top2 = r.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 2e-3
    return bool((cls[sure] == r.argmax(1)[sure]).all())


@pytest.mark.parametrize('dim,levels,C,shape', [(2, 4, 256, (2, 128, 96)), (3, 4, 64, (1, 32, 48, 32)), (3, 5, 64, (1, 32, 32, 48)),
                                                (2, 3, 96, (2, 40, 24))])
def test_forward_parity(dim, levels, C, shape):
    from interactive_unet.engine_segformer import SegformerEngine, SegformerEngineF32
    ncls = 3
    p = ref.init_params(dim, levels, 32, 1, ncls, C, seed=11, randomize_bn=True)
    N, sp = shape[0], shape[1:]
    x = torch.tensor(np.random.default_rng(2).integers(0, 256, (N, 1) + sp, dtype=np.uint8))
    r64 = ref.forward_logits(p, x.double() / 255.0, dim, levels).float()
    D, H, W = _dims(sp)
    vox = D * H * W
    xs = (vox, vox, H * W, W, 1)
    e = SegformerEngineF32(dim, levels, 32, 1, ncls, decoder_channels=C)
    e.load_eval({k: v.cuda() for k, v in p.items()})
    logits = torch.empty((N, ncls) + sp, device='cuda')
    cls = torch.empty((N, vox), dtype=torch.uint8, device='cuda')
    e.infer(x.cuda(), xs, N, D, H, W, logits=logits, cls=cls)
    torch.cuda.synchronize()
    err = (logits.cpu() - r64).abs().max().item()
    print(f'{dim}-D L={levels} C={C}: fp32 form max |logit - ref| = {err:.2e}')
    assert err <= 1e-4
    assert _margin_ok(cls.cpu().long().reshape(N, *sp), r64)
    pref = torch.softmax(r64.double(), 1)
    for T, gate in ((torch.float16, 5e-3), (torch.bfloat16, 3e-2)):
        same = torch.softmax(ref.forward_logits(p, x.double() / 255.0, dim, levels, act=T), 1)
        e16 = SegformerEngine(dim, levels, 32, 1, ncls, T, decoder_channels=C)
        e16.load_eval({k: v.cuda() for k, v in p.items()})
        probs = torch.empty((N, ncls) + sp, device='cuda')
        e16.infer(x.cuda(), xs, N, D, H, W, probs=probs)
        torch.cuda.synchronize()
        dp = (probs.cpu().double() - pref).abs().max().item()
        print(f'{dim}-D L={levels} C={C}: {T} max |dprob| = {dp:.2e} (gate {gate:.0e}; same-rounding reference '
              f'{(same - pref).abs().max().item():.2e})')
        assert dp <= gate


# ---------------------------------------------------------------------------------------------- 3. one step against CPU autograd
def _batch(dim, N, sp, ncls=2, seed=0):
    rng = np.random.default_rng(seed)
    img = rng.random((N, 1) + sp).astype(np.float32)
    k = torch.ones((1, 1) + (5,) * dim) / 5 ** dim
    img = (F.conv2d if dim == 2 else F.conv3d)(torch.tensor(img), k, padding=2).numpy()
    img = (img - img.min()) / (img.max() - img.min())
    lab = img[:, 0] > 0.5
    y = np.stack([~lab, lab], 1).astype(np.float32)
    wt = np.repeat((rng.random((N, 1) + sp) > 0.2).astype(np.float32), ncls, 1)
    return torch.tensor(img), torch.tensor(y * wt), torch.tensor(wt)


@pytest.mark.parametrize('dim,sp,dtype,C,N', [(2, (64, 96), 'fp16', 128, 2), (3, (16, 32, 32), 'bf16', 64, 2), (2, (64, 64), 'fp16', 64, 1)])
def test_train_step_vs_autograd(dim, sp, dtype, C, N):
    from interactive_unet.train_engine_segformer import SegformerTrainEngine
    ncls, L = 2, 4
    p0 = ref.init_params(dim, L, 32, 1, ncls, C, seed=5)
    g = torch.Generator().manual_seed(9)
    for l in range(L):
        p0[f'mlp{l}.bias'] = 0.2 * torch.randn(C, generator=g)
    X, y, wt = _batch(dim, N, sp, seed=1)
    act = torch.float16 if dtype == 'fp16' else torch.bfloat16
    axes = (0,) + tuple(range(2, 2 + dim))
    runs = []
    for _ in range(2):
        m = _model(dim, L, act_dtype=dtype, decoder_segmentation_channels=C)
        m.load_named(p0)
        m = m.cuda()
        te = SegformerTrainEngine(m, lr=1e-3, loss_scale=(256.0 if dtype == 'fp16' else 1.0))
        out = te.train_step(X, y, wt)
        torch.cuda.synchronize()
        runs.append((out, te.grad.cpu().clone(), te.flat.cpu().clone(), te, m))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2]), 'not deterministic'
    out, _, _, te, m = runs[0]

    def oracle(a):
        pr = {k: v.clone().double().requires_grad_(not unet_ref.is_buffer(k)) for k, v in p0.items()}
        st = {}
        probs = torch.softmax(ref.forward_logits(pr, X, dim, L, training=True, act=a, stats=st), 1)
        lv = metrics_ref.loss('mcc_ce', probs.detach().numpy(), y.numpy(), wt.numpy(), axes=axes)
        probs.backward(torch.tensor(metrics_ref.loss_grad('mcc_ce', probs.detach().numpy(), y.numpy(), wt.numpy(), axes=axes)))
        return pr, st, lv
    pr64, _, lv64 = oracle(None)
    pr, stats, lv = oracle(act)
    print(f'{dim}-D {dtype} N={N}: native loss {out["Loss"]:.5f} vs reference (same rounding) {lv:.5f} vs float64 {lv64:.5f}')
    assert abs(out['Loss'] - lv) < (2e-3 if dtype == 'fp16' else 1e-2)
    cosine = lambda a, b: F.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0).item()
    worst = {}
    for name in te.names:
        gn = te.g(name).cpu().reshape(pr[name].shape) / te.loss_scale
        if name.startswith('mlp') and name.endswith('.bias'):
            # zero in exact arithmetic (fuse.bn follows): held by magnitude against the level's weight gradient
            gw = te.g(name.replace('.bias', '.weight')).cpu() / te.loss_scale
            assert gn.norm() <= 1e-2 * gw.norm(), (name, gn.norm().item(), gw.norm().item())
            continue
        c_native, c_ref = cosine(gn, pr64[name].grad), cosine(pr[name].grad, pr64[name].grad)
        enc = name.startswith('enc')
        kind = 'encoder' if enc else 'decoder / head'
        worst[kind] = min(worst.get(kind, 1.0), c_native - c_ref)
        tol = (0.06 if enc else 0.02) if dtype == 'fp16' else (0.35 if enc else 0.04)
        assert c_native > c_ref - tol, (name, c_native, c_ref)
    print('   worst cos(native, float64) - cos(reference, float64):', {k: round(v, 4) for k, v in worst.items()})
    for bn in ('enc0.bn1', 'fuse.bn'):
        mean, var = stats[bn]
        err = (m.tensor(bn + '.running_mean').cpu().double() - 0.1 * mean).abs().max().item()
        print(f'   {bn}: max |running mean - reference| = {err:.2e}')
        assert torch.allclose(m.tensor(bn + '.running_mean').cpu().double(), 0.1 * mean, atol=2e-3, rtol=2e-2), bn
        assert torch.allclose(m.tensor(bn + '.running_var').cpu().double(), 0.9 + 0.1 * var, rtol=2e-2, atol=2e-2), bn


# ---------------------------------------------------------------------------------------------- 4. the public interface
def test_module_training_and_validation():
    m = _model(2, 4, decoder_segmentation_channels=64).cuda()
    X, y, wt = _batch(2, 2, (64, 64), seed=3)
    te = m.train_engine()
    losses = [te.train_step(X, y, wt)['Loss'] for _ in range(8)]
    print('loss over eight steps:', ' '.join(f'{v:.4f}' for v in losses))
    assert all(np.isfinite(losses)) and min(losses[-3:]) < losses[0]
    val = m.validation_step((X[:1], y[:1], wt[:1]))
    assert np.isfinite(val.item())
    for prm in m.parameters():
        prm.grad = None
    loss = m.training_step((X, y, wt))
    scale = te.loss_scale
    loss.backward()
    flat = te.grad * (1.0 / scale)
    for n in te.names:
        g = m.tensor(n).grad
        assert g is not None, n
        assert torch.equal(g, flat[te.offsets[n][0]:te.offsets[n][0] + te.offsets[n][1]].view(g.shape)), n


def test_trainer_and_prediction(tmp_path, monkeypatch):
    from interactive_unet import trainer, predict
    from interactive_unet.unet import UNet
    monkeypatch.chdir(tmp_path)
    X, y, wt = _batch(2, 2, (64, 64), seed=4)
    loader = [(X, y, wt)] * 2
    m = trainer.train_model(lr=1e-3, batch_size=2, epochs=2, architecture='Segformer', pretrained=False, train_loader=loader,
                            val_loader=loader[:1])
    assert os.path.isfile(os.path.join('model', 'model.ckpt'))
    r = UNet.load_from_checkpoint(checkpoint_path=os.path.join('model', 'model.ckpt')).cuda()
    assert r.architecture == 'Segformer' and r.decoder_segmentation_channels == 256
    p = {k: v.detach().cpu() for k, v in r.named_tensors().items()}
    xin = X[:1]
    got = r(xin.cuda()).cpu()
    want = torch.softmax(ref.forward_logits(p, xin.double(), 2, 4), 1)
    assert (got.double() - want).abs().max().item() <= 1e-3
    assert predict.find_max_batch_size(r, input_size=256) >= 4
    img = (np.random.default_rng(8).random((64, 96)) * 255).astype(np.uint8)
    rgb = predict.predict_slice(img, model=r)
    assert tuple(np.asarray(rgb.cpu() if torch.is_tensor(rgb) else rgb).shape) == (64, 96, 3)
    blk = torch.rand((32, 32, 32), generator=torch.Generator().manual_seed(5))
    got = predict.predict_block(r, blk, num_classes=2, batch_size=32)
    acc = 0
    for axis in (0, 1, 2):
        sl = blk.movedim(axis, 0)[:, None]
        pr = torch.softmax(ref.forward_logits(p, sl.double(), 2, 4), 1).float()
        acc = acc + pr.permute(0, 2, 3, 1).movedim(0, axis)
    err = np.abs(got - (acc / 3).numpy()).max()
    print(f'2.5-D block: max |dprob| vs reference {err:.2e}')
    assert err <= 1e-3
    vol = (np.random.default_rng(6).random((40, 48, 56)) * 255).astype(np.uint8)
    m3 = _model(3, 4, decoder_segmentation_channels=64).cuda()
    for mod in (r, m3):
        q = predict.predict_volume_array(mod, vol, input_size=32, num_classes=2)
        torch.cuda.synchronize()
        assert q.numel() == vol.size * 2 and q.dtype == torch.uint8
    mt = _model(2, 4, infer_dtype='fp16').cuda()
    mt.load_named(p)
    pt = mt(xin.cuda()).cpu().double()
    assert (pt - want).abs().max().item() <= 5e-3
