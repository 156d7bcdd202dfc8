"""U-Net++ on the MI355X: the summed-gradient BatchNorm + ReLU backward (iunet_bn_relu_sum_bwd), the nested forwards against the CPU
reference, the L = 2 identity with the U-Net, one training step against CPU autograd, and the public interface."""
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import unet_ref, metrics_ref
from tests import unetpp_ref

pytestmark = pytest.mark.gpu


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


def _model(dim=2, levels=4, base=32, ncls=2, **kw):
    from interactive_unet.unet import UNet
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return UNet(architecture='U-Net++', num_classes=ncls, dim=dim, levels=levels, base=base, pretrained=False, **kw)


# ---------------------------------------------------------------------------------------------- 1. the kernel
def _sum_bwd_case(nd, T, K, pool, sp, C=32, N=2, seed=0):
    from interactive_unet import _native as nv
    g = torch.Generator().manual_seed(seed)
    dt = nv.DTYPE_CODE[T]
    y = (torch.randn((N, C) + sp, generator=g) * 1.5 + 0.3).to(T).float()
    axes = (0,) + tuple(range(2, 2 + len(sp)))
    mean, var = y.mean(axes), y.var(axes, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    gamma = 0.75 + 0.5 * torch.rand(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    scale, shift = gamma * invstd, beta - mean * gamma * invstd
    # sources: slot k % 2 of a 2-slot buffer (sample stride 2 C vox), as the level buffers hand them to the kernel
    srcs = [(torch.randn((N, C) + sp, generator=g) * 0.1).to(T).float() for _ in range(K)]
    bufs = []
    for k in range(K):
        other = (torch.randn((N, C) + sp, generator=g) * 0.1).to(T).float()
        pair = [other, srcs[k]] if k % 2 else [srcs[k], other]
        bufs.append(_blocked(torch.cat(pair, 1), T).cuda())
    vox = int(np.prod(sp))
    psp = tuple(s // 2 for s in sp) if nd == 3 else (1, sp[0] // 2, sp[1] // 2)[1:]
    dpool = (torch.randn((N, C) + psp, generator=g) * 0.1).to(T).float() if pool else None
    f32 = lambda t: t.float().cuda().contiguous()
    yb = _blocked(y, T).cuda()
    dy = torch.empty_like(yb)
    dgam, dbet = torch.empty(C, device='cuda'), torch.empty(C, device='cuda')
    slab = torch.empty(nv.lib().iunet_bn_bwd_num_parts(N, vox) * C * 2, device='cuda')
    coef = torch.empty(3 * C, device='cuda')
    es = 2
    import ctypes
    ptrs = (ctypes.c_void_p * K)(*[b.data_ptr() + (k % 2) * C * vox * es for k, b in enumerate(bufs)])
    sss = nv.ll_array([2 * C * vox] * K)
    dpb = _blocked(dpool, T).cuda() if pool else None
    D, H, W = sp if nd == 3 else (1,) + sp
    args = (f32(mean), f32(invstd), f32(gamma), f32(scale), f32(shift))
    nv.call('iunet_bn_relu_sum_bwd', dt, nd, K, ptrs, sss, nv.ptr(dpb), (C * vox) // (8 if nd == 3 else 4), nv.ptr(yb), C * vox,
            nv.ptr(dy), C * vox, *[nv.ptr(a) for a in args], nv.ptr(dgam), nv.ptr(dbet), nv.ptr(slab), nv.ptr(coef), C, N, D, H, W,
            nv.stream())
    torch.cuda.synchronize()
    got = (_unblocked(dy.cpu().float(), C, sp), dgam.cpu(), dbet.cpu())
    # K = 1: the existing kernels on the same operands
    same = None
    if K == 1:
        dy1, dg1, db1 = torch.empty_like(yb), torch.empty(C, device='cuda'), torch.empty(C, device='cuda')
        src0 = ctypes.c_void_p(ptrs[0])
        if pool:
            nv.call('iunet_bn_relu_pool_bwd', dt, nd, src0, 2 * C * vox, nv.ptr(dpb), (C * vox) // (8 if nd == 3 else 4), nv.ptr(yb), C * vox,
                    nv.ptr(dy1), C * vox, nv.ptr(args[0]), nv.ptr(args[1]), nv.ptr(args[2]), nv.ptr(args[3]), nv.ptr(args[4]),
                    nv.ptr(dg1), nv.ptr(db1), nv.ptr(slab), nv.ptr(coef), C, N, *(psp if nd == 3 else (1,) + psp), nv.stream())
        else:
            nv.call('iunet_bn_relu_bwd', dt, src0, 2 * C * vox, None, C * vox, nv.ptr(yb), C * vox, nv.ptr(dy1), C * vox,
                    nv.ptr(args[0]), nv.ptr(args[1]), nv.ptr(args[2]), nv.ptr(args[3]), nv.ptr(args[4]),
                    nv.ptr(dg1), nv.ptr(db1), nv.ptr(slab), nv.ptr(coef), C, N, vox, nv.stream())
        torch.cuda.synchronize()
        same = torch.equal(dy1, dy) and torch.equal(dg1, dgam) and torch.equal(db1, dbet)
    # CPU autograd of relu(bn(y)) with dz = sum of the sources (+ the max-pool route of dpool to each window's first maximum)
    yd = y.double().requires_grad_()
    shp = [1, -1] + [1] * len(sp)
    m, v_ = yd.mean(axes), yd.var(axes, unbiased=False)
    z = F.relu((yd - m.view(shp)) / torch.sqrt(v_.view(shp) + 1e-5) * gamma.double().view(shp) + beta.double().view(shp))
    dz = sum(s.double() for s in srcs)
    if pool:
        zs = (scale.view(shp) * y + shift.view(shp)).clamp_min(0).to(T).float()      # z as the forward stored it
        zt = zs.detach().requires_grad_()
        pl = (F.max_pool3d if nd == 3 else F.max_pool2d)(zt, 2)
        pl.backward(dpool)
        dz = dz + zt.grad.double()
    z.backward(dz)
    ref_dy = yd.grad
    ref_dbeta = (dz * (z > 0)).sum(axes)
    xh = (y.double() - m.detach().view(shp)) / torch.sqrt(v_.detach().view(shp) + 1e-5)
    ref_dgamma = (dz * (z > 0) * xh).sum(axes)
    return got, (ref_dy, ref_dgamma, ref_dbeta), same


@pytest.mark.parametrize('K', [1, 2, 3, 5, 8])
@pytest.mark.parametrize('pool', [False, True])
@pytest.mark.parametrize('nd,sp', [(2, (46, 90)), (3, (6, 18, 34))])       # voxel counts off the 2 048-voxel tile
@pytest.mark.parametrize('T', [torch.float16, torch.bfloat16])
def test_bn_relu_sum_bwd(K, pool, nd, sp, T):
    got, ref, same = _sum_bwd_case(nd, T, K, pool, sp, seed=K * 7 + nd)
    tol = 2e-2 if T == torch.float16 else 6e-2
    for name, a, b in zip(('dy', 'dgamma', 'dbeta'), got, ref):
        err = ((a.double() - b).norm() / (b.norm() + 1e-30)).item()
        print(f'K={K} pool={pool} {nd}-D {T}: {name} relative error {err:.2e}')
        assert err < tol, (name, err)
    if K == 1:
        assert same, 'K = 1 differs from iunet_bn_relu_bwd / iunet_bn_relu_pool_bwd'


# ---------------------------------------------------------------------------------------------- 2. forward parity
def _margin_ok(cls, ref):
    top2 = ref.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 2e-3
    return bool((cls[sure] == ref.argmax(1)[sure]).all())


@pytest.mark.parametrize('dim,levels,base,ncls,shape', [(2, 4, 32, 2, (2, 256, 256)), (3, 4, 32, 2, (1, 64, 64, 64)),
                                                        (3, 5, 64, 4, (1, 32, 32, 48))])
def test_forward_parity(dim, levels, base, ncls, shape):
    from interactive_unet.engine_nested import NestedEngine, NestedEngineF32
    p = unetpp_ref.init_params(dim, levels, base, 1, ncls, seed=11, randomize_bn=True)
    N, sp = shape[0], shape[1:]
    x = torch.tensor(np.random.default_rng(2).integers(0, 256, (N, 1) + sp, dtype=np.uint8))
    ref = unetpp_ref.forward_logits(p, x.double() / 255.0, dim, levels, dtype=torch.float64).float()
    D, H, W = sp if dim == 3 else (1,) + sp
    vox = D * H * W
    xs = (vox, vox, H * W, W, 1)
    e = NestedEngineF32(dim, levels, base, 1, ncls)
    e.load_eval({k: v.cuda() for k, v in p.items()})
    logits = torch.empty((N, ncls) + sp, device='cuda')
    cls = torch.empty((N, vox), dtype=torch.uint8, device='cuda')
    e.infer(x.cuda(), xs, N, D, H, W, logits=logits, cls=cls)
    torch.cuda.synchronize()
    err = (logits.cpu() - ref).abs().max().item()
    print(f'{dim}-D L={levels} base {base}: fp32 form max |logit - ref| = {err:.2e}')
    assert err <= 1e-3
    assert _margin_ok(cls.cpu().long().reshape(N, *sp), ref)
    pref = torch.softmax(ref, 1)
    for T, gate in ((torch.float16, 5e-3), (torch.bfloat16, 3e-2)):
        e16 = NestedEngine(dim, levels, base, 1, ncls, T)
        e16.load_eval({k: v.cuda() for k, v in p.items()})
        probs = torch.empty((N, ncls) + sp, device='cuda')
        e16.infer(x.cuda(), xs, N, D, H, W, probs=probs)
        torch.cuda.synchronize()
        dp = (probs.cpu() - pref).abs().max().item()
        print(f'{dim}-D L={levels} base {base}: {T} max |dprob| = {dp:.2e}')
        assert dp <= gate


# ---------------------------------------------------------------------------------------------- 3. L = 2 is the U-Net
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


@pytest.mark.parametrize('dim,sp', [(2, (64, 96)), (3, (16, 32, 32))])
def test_two_levels_equal_unet(dim, sp):
    from interactive_unet.unet import UNet
    from interactive_unet.engine import Engine
    from interactive_unet.engine_nested import NestedEngine
    from interactive_unet.train_engine import TrainEngine
    from interactive_unet.train_engine_nested import NestedTrainEngine
    p = unetpp_ref.init_params(dim, 2, 32, 1, 2, seed=9, randomize_bn=True)
    pu = unetpp_ref.to_unet_names(p)
    N = 2
    X, y, wt = _batch(dim, N, sp)
    D, H, W = sp if dim == 3 else (1,) + sp
    vox = D * H * W
    outs = []
    for eng, pp in ((NestedEngine(dim, 2, 32, 1, 2, torch.float16), p), (Engine(dim, 2, 32, 1, 2, torch.float16), pu)):
        eng.use_graph = False
        eng.load_eval({k: v.cuda() for k, v in pp.items()})
        lg = torch.empty((N, 2) + sp, device='cuda')
        eng.infer(X.cuda(), (vox, vox, H * W, W, 1), N, D, H, W, logits=lg)
        outs.append(lg.cpu())
    assert torch.equal(outs[0], outs[1]), 'nested forward at L = 2 differs from the U-Net'
    res = []
    for nested in (True, False):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            m = UNet(architecture='U-Net++' if nested else 'U-Net', dim=dim, levels=2, act_dtype='fp16', pretrained=False)
        m.load_named(p if nested else pu)
        m = m.cuda()
        te = (NestedTrainEngine if nested else TrainEngine)(m, lr=1e-3, loss_scale=256.0)
        te.use_handle = False
        out = te.train_step(X, y, wt)
        torch.cuda.synchronize()
        res.append((out, te.grad.cpu().clone(), te.flat.cpu().clone(),
                    torch.cat([m.tensor(n).cpu() for n in m._names if n.endswith('running_mean') or n.endswith('running_var')])))
    assert res[0][0] == res[1][0]
    for a, b, what in zip(res[0][1:], res[1][1:], ('gradient', 'parameters', 'running statistics')):
        assert torch.equal(a, b), f'{what} after one step at L = 2 differ from the U-Net'


# ---------------------------------------------------------------------------------------------- 4. one step against CPU autograd
@pytest.mark.parametrize('dim,sp,dtype', [(2, (64, 96), 'fp16'), (3, (16, 32, 32), 'bf16')])
def test_train_step_vs_autograd(dim, sp, dtype):
    from interactive_unet.train_engine_nested import NestedTrainEngine
    N, ncls, L = 2, 2, 4
    p0 = unetpp_ref.init_params(dim, L, 32, 1, ncls, seed=5)
    X, y, wt = _batch(dim, N, sp, seed=1)
    act = torch.float16 if dtype == 'fp16' else torch.bfloat16
    axes = (0,) + tuple(range(2, 2 + dim))

    def oracle(act_dtype):
        pr = {k: v.clone().requires_grad_(not unet_ref.is_buffer(k)) for k, v in p0.items()}
        st = {}
        probs = torch.softmax(unetpp_ref.forward_logits(pr, X, dim, L, training=True, act_dtype=act_dtype, bn_stats_out=st), 1)
        lv = metrics_ref.loss('mcc_ce', probs.detach().numpy(), y.numpy(), wt.numpy(), axes=axes)
        probs.backward(torch.tensor(metrics_ref.loss_grad('mcc_ce', probs.detach().numpy(), y.numpy(), wt.numpy(), axes=axes)).float())
        return pr, st, lv
    pr32, stats, lv32 = oracle(None)
    pr, _, lv = oracle(act)
    runs = []
    for _ in range(2):
        m = _model(dim, L, act_dtype=dtype)
        m.load_named(p0)
        m = m.cuda()
        te = NestedTrainEngine(m, lr=1e-3, loss_scale=(256.0 if dtype == 'fp16' else 1.0))
        out = te.train_step(X, y, wt)
        torch.cuda.synchronize()
        runs.append((out, te.grad.cpu().clone(), te.flat.cpu().clone(), te, m))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2]), 'not deterministic'
    out, _, _, te, m = runs[0]
    print(f'{dim}-D {dtype}: native loss {out["Loss"]:.5f} vs reference (same rounding) {lv:.5f} vs fp32 {lv32:.5f}')
    assert abs(out['Loss'] - lv) < (2e-3 if dtype == 'fp16' else 1e-2)
    cosine = lambda a, b: F.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0).item()
    worst = 1.0
    for name in te.names:
        gn = te.g(name).cpu().reshape(pr[name].shape) / te.loss_scale
        c_native, c_ref = cosine(gn, pr32[name].grad), cosine(pr[name].grad, pr32[name].grad)
        worst = min(worst, c_native)
        assert c_native > c_ref - (0.02 if dtype == 'fp16' else 0.04), (name, c_native, c_ref)
        assert c_native > 0.85, (name, c_native)
        if name.startswith('head') or name.startswith(f'dec0_{L - 1}.conv') or name.startswith(f'dec0_{L - 1}.bn'):
            # (the shallow tensors, as test_full_train_step_vs_autograd holds dec0.conv / dec0.bn; up.weight's gradient reads X^{1,L-2})
            assert c_native > (0.9995 if dtype == 'fp16' else 0.999), (name, c_native)
        nrm = (gn.norm() / (pr32[name].grad.norm() + 1e-20)).item()
        assert 0.9 < nrm < 1.1, (name, nrm)
    print(f'   min cos(native, fp32) = {worst:.4f}')
    for bn in ('enc0.bn1', f'dec0_{L - 1}.bn2', 'dec1_1.bn1'):
        mean, var = stats[bn]
        assert torch.allclose(m.tensor(bn + '.running_mean').cpu(), 0.1 * mean, atol=2e-3), bn


# ---------------------------------------------------------------------------------------------- 5. the public interface
def test_training_lowers_loss_and_autograd_grads():
    m = _model(2, 4).cuda()
    X, y, wt = _batch(2, 2, (64, 64), seed=3)
    te = m.train_engine()
    losses = [te.train_step(X, y, wt)['Loss'] for _ in range(10)]
    print('loss over ten steps:', ' '.join(f'{v:.4f}' for v in losses))
    assert losses[-1] < losses[0]
    for prm in m.parameters():
        prm.grad = None
    loss = m.training_step((X, y, wt))
    scale = te.loss_scale
    loss.backward()
    flat = te.grad * (1.0 / scale)          # the engine's gradient of the loss (step_backward's unscaling)
    for n in te.names:
        g = m.tensor(n).grad
        assert g is not None, n
        ref = flat[te.offsets[n][0]:te.offsets[n][0] + te.offsets[n][1]].view(g.shape)
        assert torch.equal(g, ref), n


def test_trainer_and_prediction(tmp_path, monkeypatch):
    from interactive_unet import trainer, predict
    from interactive_unet.unet import UNet
    monkeypatch.chdir(tmp_path)
    X, y, wt = _batch(2, 2, (64, 64), seed=4)
    loader = [(X, y, wt)] * 2
    m = trainer.train_model(lr=1e-3, epochs=2, architecture='U-Net++', pretrained=False, train_loader=loader, val_loader=loader[:1])
    assert os.path.isfile(os.path.join('model', 'model.ckpt'))
    r = UNet.load_from_checkpoint(checkpoint_path=os.path.join('model', 'model.ckpt')).cuda()
    assert r.architecture == 'U-Net++'
    xin = X[:1].cuda()
    a, b = m.cuda()(xin), r(xin)
    # (the checkpoint is the best-validation epoch; the module may have moved one epoch past it)
    if torch.equal(torch.cat([t.reshape(-1) for t in m.named_tensors().values()]).cpu(),
                   torch.cat([t.reshape(-1) for t in r.named_tensors().values()]).cpu()):
        assert torch.equal(a, b)
    assert predict.find_max_batch_size(r, input_size=256) >= 4
    # 2.5-D block and a 3-D volume through predict_volume_array against the CPU reference (fp32 form)
    p = {k: v.detach().cpu() for k, v in r.named_tensors().items()}
    blk = torch.rand((32, 32, 32), generator=torch.Generator().manual_seed(5))
    got = predict.predict_block(r, blk, num_classes=2, batch_size=32)
    ref = 0
    for axis in (0, 1, 2):
        sl = blk.movedim(axis, 0)[:, None]
        pr = unetpp_ref.forward(p, sl.double(), 2, 4, dtype=torch.float64).float()
        ref = ref + pr.permute(0, 2, 3, 1).movedim(0, axis)
    ref = ref / 3
    err = np.abs(got - ref.numpy()).max()
    print(f'2.5-D block: max |dprob| vs reference {err:.2e}')
    assert err <= 1e-3
    vol = (np.random.default_rng(6).random((40, 48, 56)) * 255).astype(np.uint8)
    m3 = _model(3, 4).cuda()
    for mod in (r, m3):                 # 2.5-D blocks through the 2-D net, direct blocks through the 3-D net
        q = predict.predict_volume_array(mod, vol, input_size=32, num_classes=2)
        torch.cuda.synchronize()
        assert q.numel() == vol.size * 2 and q.dtype == torch.uint8
    v3 = torch.rand((1, 1, 32, 32, 32), generator=torch.Generator().manual_seed(7))
    p3 = {k: v.detach().cpu() for k, v in m3.named_tensors().items()}
    err3 = (m3(v3.cuda()).cpu() - unetpp_ref.forward(p3, v3.double(), 3, 4, dtype=torch.float64).float()).abs().max().item()
    print(f'3-D forward through the module: max |dprob| vs reference {err3:.2e}')
    assert err3 <= 1e-3
