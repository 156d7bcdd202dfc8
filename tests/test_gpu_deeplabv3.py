"""DeepLabV3 on the MI355X: the kernels of csrc/deeplab.hip against float64 torch, the forwards against the CPU reference, one training
step against CPU autograd with the engine's dropout mask replayed, and the public interface."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import unet_ref, metrics_ref
from tests import deeplabv3_ref as ref

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
        return UNet(architecture='DeepLabV3', num_classes=ncls, dim=dim, levels=levels, base=base, pretrained=False, **kw)


def _dims(sp):
    return tuple(sp) if len(sp) == 3 else (1,) + tuple(sp)


def _conv(nd, x, w, rate):
    k = w.shape[-1]
    return (F.conv3d if nd == 3 else F.conv2d)(x, w, padding=max(rate, 1) * (k // 2), dilation=max(rate, 1))


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


_KEEP = []


def _dev(t):
    """t on the GPU, kept alive until the next test (a temporary passed as a bare pointer could be freed and reused before the launch)."""
    if len(_KEEP) > 64:
        torch.cuda.synchronize()
        del _KEEP[:]
    _KEEP.append(t.cuda())
    return _KEEP[-1]


# ---------------------------------------------------------------------------------------------- 1. the kernels
# (nd, grid, Cin, Cout, rate): rates below and at / above the grid's extent (pruned taps), odd grids
CONV_CASES = [(2, (5, 7), 32, 32, 2), (2, (9, 4), 64, 32, 6), (2, (3, 11), 32, 64, 0), (3, (3, 5, 4), 32, 32, 2), (3, (4, 4, 4), 32, 48, 4),
              (3, (2, 3, 5), 64, 32, 12)]


@pytest.mark.parametrize('T', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('nd,sp,cin,cout,rate', CONV_CASES)
def test_conv_dgrad_wgrad(nd, sp, cin, cout, rate, T):
    from interactive_unet import _native as nv
    dt, N, g = nv.DTYPE_CODE[T], 2, torch.Generator().manual_seed(1)
    ksz = 1 if rate == 0 else 3
    kv = ksz ** nd
    x = torch.randn((N, cin) + sp, generator=g).to(T).double()
    w = torch.randn((cout, cin) + (ksz,) * nd, generator=g) * 0.1
    d = _dims(sp)
    s = nv.stream()
    wpk = torch.empty(cout * kv * cin, dtype=T, device='cuda')
    wd = w.cuda()
    nv.call('iunet_dl_pack', dt, nd, 0, ksz, nv.ptr(wd), None, None, None, None, 0.0, nv.ptr(wpk), None, cout, cin, cin, 0, 0, kv * cin, s)
    xb = _blocked(x, T).cuda()
    psb = torch.randn((N, cout), generator=g).cuda()
    outs = []
    for _ in range(2):
        y = torch.empty(N * cout * int(np.prod(sp)), dtype=T, device='cuda')
        nparts = nv.lib().iunet_dl_stats_parts(N, *d, cout)
        stats = torch.empty(nparts * cout * 2, device='cuda')
        nv.call('iunet_dl_conv_fwd', dt, nd, _P(xb), cin * int(np.prod(sp)), _P(y), cout * int(np.prod(sp)), nv.ptr(wpk), kv * cin, 1,
                nv.int_array([rate]), nv.int_array([0]), nv.int_array([0]), None, None, None, nv.ptr(psb), 0.5, nv.ptr(stats), 0, N, *d, cin, cout, s)
        torch.cuda.synchronize()
        outs.append((y.cpu(), stats.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    want = _conv(nd, x, w.to(T).double(), rate) + 0.5 * psb.cpu().double().view(N, cout, *([1] * nd))
    got = _unblocked(outs[0][0].view(N, -1), cout, sp).double()
    tol = 2e-2 if T == torch.float16 else 8e-2
    assert (got - want).abs().max().item() <= tol * max(1.0, want.abs().max().item())
    st = outs[0][1].view(nparts, cout, 2).sum(0).double()
    assert torch.allclose(st[:, 0], want.sum((0,) + tuple(range(2, 2 + nd))), rtol=1e-2, atol=0.5)
    # data gradient: the flipped operator over dy
    dy = torch.randn((N, cout) + sp, generator=g).to(T).double()
    wdg = torch.empty(cin * kv * cout, dtype=T, device='cuda')
    nv.call('iunet_dl_pack', dt, nd, 1, ksz, nv.ptr(wd), None, None, None, None, 0.0, nv.ptr(wdg), None, cout, cin, cin, 0, 0, kv * cout, s)
    dx = torch.empty(N * cin * int(np.prod(sp)), dtype=T, device='cuda')
    nv.call('iunet_dl_conv_fwd', dt, nd, _P(_dev(_blocked(dy, T))), cout * int(np.prod(sp)), _P(dx), cin * int(np.prod(sp)), nv.ptr(wdg),
            kv * cout, 1, nv.int_array([rate]), nv.int_array([0]), nv.int_array([0]), None, None, None, None, 1.0, None, 0, N, *d, cout, cin, s)
    xr = x.clone().requires_grad_(True)
    _conv(nd, xr, w.to(T).double(), rate).backward(dy)
    got = _unblocked(dx.cpu().view(N, -1), cin, sp).double()
    assert (got - xr.grad).abs().max().item() <= tol * max(1.0, xr.grad.abs().max().item())
    # weight gradient (LDS-staged), with the input activation prologue
    sc, sh = torch.rand(cin, generator=g) + 0.5, torch.randn(cin, generator=g) * 0.3
    xa = torch.relu(sc.view(1, -1, *([1] * nd)) * x + sh.view(1, -1, *([1] * nd))).to(T).double()
    wr = w.double().clone().requires_grad_(True)
    _conv(nd, xa, wr, rate).backward(dy)
    dws = []
    for _ in range(2):
        slab = torch.empty(nv.lib().iunet_dl_wgrad_slab_floats(nd, rate, N, *d, cin, cout), device='cuda')
        dW = torch.full((cout, cin) + (ksz,) * nd, float('nan'), device='cuda')
        nv.call('iunet_dl_wgrad', dt, nd, rate, _P(xb), cin * int(np.prod(sp)), 0, _P(_dev(_blocked(dy, T))), cout * int(np.prod(sp)),
                nv.ptr(_dev(sc)), nv.ptr(_dev(sh)), nv.ptr(slab), nv.ptr(dW), cin, 0, 1.0, N, *d, cin, cout, s)
        torch.cuda.synchronize()
        dws.append(dW.cpu())
    assert torch.equal(dws[0], dws[1])
    assert (dws[0].double() - wr.grad).abs().max().item() <= 2e-3 * max(1.0, wr.grad.abs().max().item())


@pytest.mark.parametrize('nd,sp,rate', [(2, (6, 7), 3), (3, (3, 4, 5), 2), (3, (4, 4, 4), 5)])
def test_f32_conv_with_psb(nd, sp, rate):
    from interactive_unet import _native as nv
    N, cin, cout, g = 2, 32, 48, torch.Generator().manual_seed(3)
    x = torch.randn((N, cin) + sp, generator=g, dtype=torch.float64)
    w = torch.randn((cout, cin) + (3,) * nd, generator=g, dtype=torch.float64) * 0.1
    bias, psb = torch.randn(cout, generator=g), torch.randn((N, cout), generator=g)
    kv = 3 ** nd
    wpk = torch.empty(cout * kv * cin, device='cuda')
    nv.call('iunet_dl_pack', 2, nd, 0, 3, nv.ptr(_dev(w.float())), None, None, None, None, 0.0, nv.ptr(wpk), None, cout, cin, cin, 0, 0,
            kv * cin, nv.stream())
    y = torch.empty((N, cout) + sp, device='cuda')
    v = int(np.prod(sp))
    nv.call('iunet_dl_f32_conv_fwd', nd, rate, nv.ptr(_dev(x.float())), cin * v, nv.ptr(y), cout * v, nv.ptr(wpk), kv * cin, nv.ptr(_dev(bias)),
            nv.ptr(_dev(psb)), N, *_dims(sp), cin, cout, nv.stream())
    torch.cuda.synchronize()
    want = torch.relu(_conv(nd, x, w, rate) + bias.double().view(1, -1, *([1] * nd)) + psb.double().view(N, cout, *([1] * nd)))
    assert (y.cpu().double() - want).abs().max().item() <= 1e-4


@pytest.mark.parametrize('T', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('nd,sp,rates', [(2, (6, 5), (2, 4, 7)), (3, (3, 4, 4), (1, 2, 5))])
def test_aspp_dgrad_one_launch_and_pool(nd, sp, rates, T):
    """The four branches' data gradients and the pooling adjoint in one launch; the pooling branch forward and backward."""
    from interactive_unet import _native as nv
    dt, N, Cb, C, g = nv.DTYPE_CODE[T], 3, 64, 32, torch.Generator().manual_seed(5)
    kv, v, d, s = 3 ** nd, int(np.prod(sp)), _dims(sp), nv.stream()
    ws = [torch.randn((C, Cb) + (1,) * nd, generator=g) * 0.1] + [torch.randn((C, Cb) + (3,) * nd, generator=g) * 0.1 for _ in range(3)]
    dys = [torch.randn((N, C) + sp, generator=g).to(T).double() for _ in range(4)]
    dmean = torch.randn((N, Cb), generator=g)
    ld = C * (1 + 3 * kv)
    op = torch.empty(Cb * ld, dtype=T, device='cuda')
    for k, w in enumerate(ws):
        nv.call('iunet_dl_pack', dt, nd, 1, 1 if k == 0 else 3, nv.ptr(_dev(w)), None, None, None, None, 0.0, nv.ptr(op), None, C, Cb, Cb, 0,
                0 if k == 0 else C + (k - 1) * kv * C, ld, s)
    dycat = _blocked(torch.cat(dys, 1), T).cuda()
    dx = torch.empty(N * Cb * v, dtype=T, device='cuda')
    nv.call('iunet_dl_conv_fwd', dt, nd, _P(dycat), 4 * C * v, _P(dx), Cb * v, nv.ptr(op), ld, 4, nv.int_array((0,) + rates),
            nv.int_array([0, C, 2 * C, 3 * C]), nv.int_array([0, C, C + kv * C, C + 2 * kv * C]), None, None, None, nv.ptr(_dev(dmean)),
            1.0 / v, None, 0, N, *d, C, Cb, s)
    torch.cuda.synchronize()
    xr = torch.zeros((N, Cb) + sp, dtype=torch.float64, requires_grad=True)
    tot = sum((_conv(nd, xr, w.to(T).double(), r) * dy).sum() for w, r, dy in zip(ws, (0,) + rates, dys))
    tot.backward()
    want = xr.grad + dmean.double().view(N, Cb, *([1] * nd)) / v
    tol = 2e-2 if T == torch.float16 else 8e-2
    assert (_unblocked(dx.cpu().view(N, -1), Cb, sp).double() - want).abs().max().item() <= tol * max(1.0, want.abs().max().item())
    # pooling branch: mean -> GEMV -> BatchNorm over N -> ReLU -> W_proj[:, 4C:] -> per-sample bias, and its backward
    x = torch.randn((N, Cb) + sp, generator=g).to(T)
    wpool, wproj = torch.randn(C, Cb, generator=g) * 0.2, torch.randn(C, 5 * C, generator=g) * 0.2
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    xmean, ypool, bp, psb = (torch.empty(n, device='cuda') for n in (N * Cb, N * C, N * C, N * C))
    stats = torch.empty(N * C * 2, device='cuda')
    scale, shift, mean, invstd = (torch.empty(C, device='cuda') for _ in range(4))
    rm, rv = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
    nv.call('iunet_dl_chansum', dt, _P(_dev(_blocked(x.double(), T))), Cb * v, nv.ptr(xmean), 1.0 / v, Cb, N, v, s)
    nv.call('iunet_dl_pool_gemv', nv.ptr(xmean), nv.ptr(_dev(wpool)), nv.ptr(ypool), nv.ptr(stats), N, Cb, C, s)
    nv.call('iunet_bn_finalize', nv.ptr(stats), N, C, float(N), nv.ptr(_dev(gamma)), nv.ptr(_dev(beta)), nv.ptr(rm), nv.ptr(rv), 0.1, 1e-5,
            nv.ptr(scale), nv.ptr(shift), nv.ptr(mean), nv.ptr(invstd), s)
    wproj_d = wproj.cuda()
    nv.call('iunet_dl_pool_psb', nv.ptr(ypool), nv.ptr(scale), nv.ptr(shift), None, None, None, None, 1e-5, nv.ptr(bp), nv.ptr(wproj_d), None,
            None, nv.ptr(psb), N, C, s)
    xd = x.double().requires_grad_(True)
    m = xd.mean(tuple(range(2, 2 + nd)))
    wp, wj = wpool.double().requires_grad_(True), wproj.double().requires_grad_(True)
    ga, be = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    yp = m @ wp.t()
    bpr = torch.relu(F.batch_norm(yp, None, None, ga, be, training=True, eps=1e-5))
    psr = bpr @ wj[:, 4 * C:].t()
    torch.cuda.synchronize()
    assert (psb.cpu().view(N, C).double() - psr).abs().max().item() <= 1e-3 * max(1.0, psr.abs().max().item())
    assert torch.allclose(rm.cpu().double(), 0.1 * yp.mean(0), atol=1e-4)
    dpsb = torch.randn((N, C), generator=g)
    psr.backward(dpsb.double())
    outs = [torch.full_like(t, float('nan')) for t in (wproj_d, gamma.cuda(), beta.cuda(), wpool.cuda())]
    dxm, scr = torch.empty(N * Cb, device='cuda'), torch.empty(2 * N * C, device='cuda')
    nv.call('iunet_dl_pool_bwd', nv.ptr(_dev(dpsb)), nv.ptr(bp), nv.ptr(ypool), nv.ptr(mean), nv.ptr(invstd), nv.ptr(_dev(gamma)),
            nv.ptr(wproj_d), nv.ptr(_dev(wpool)), nv.ptr(xmean), nv.ptr(outs[0]), nv.ptr(outs[1]), nv.ptr(outs[2]), nv.ptr(outs[3]),
            nv.ptr(dxm), nv.ptr(scr), N, Cb, C, s)
    torch.cuda.synchronize()
    close = lambda a, b: (a.cpu().double() - b).abs().max().item() <= 1e-3 * max(1.0, b.abs().max().item())
    assert close(outs[0][:, 4 * C:], wj.grad[:, 4 * C:]) and close(outs[1], ga.grad) and close(outs[2], be.grad) and close(outs[3], wp.grad)
    assert close(dxm.view(N, Cb) / v, xd.grad.reshape(N, Cb, -1)[:, :, 0])


@pytest.mark.parametrize('nd,coarse,s,ncls', [(2, (5, 7), 8, 2), (2, (1, 3), 4, 3), (3, (2, 3, 4), 4, 2), (3, (3, 2, 2), 2, 5)])
def test_upsample_head_contract(nd, coarse, s, ncls):
    from interactive_unet import _native as nv
    N, g = 2, torch.Generator().manual_seed(7)
    lc = torch.randn((N, ncls) + coarse, generator=g)
    fine = tuple(c * s for c in coarse)
    want = F.interpolate(lc.double(), scale_factor=s, mode='trilinear' if nd == 3 else 'bilinear', align_corners=True)
    cd = _dims(coarse)
    D, H, W = _dims(fine)
    vox = D * H * W
    big = torch.zeros((N, ncls + 1) + fine, device='cuda')          # strided output: class planes of a wider tensor
    st = (big.stride(0), big.stride(1)) + ((big.stride(2), big.stride(3), big.stride(4)) if nd == 3 else (0, big.stride(2), big.stride(3)))
    logits = torch.empty((N, ncls) + fine, device='cuda')
    cls = torch.empty((N, vox), dtype=torch.uint8, device='cuda')
    lcd = lc.cuda()
    nv.call('iunet_dl_up_head', nd, nv.ptr(lcd), ncls, *cd, s, nv.ptr(logits), None, nv.ptr(cls), nv.ll_array(
        (ncls * vox, vox, H * W, W, 1)), 1.0, 0, N, nv.stream())
    for acc in (0, 1):
        nv.call('iunet_dl_up_head', nd, nv.ptr(lcd), ncls, *cd, s, None, nv.ptr(big), None, nv.ll_array(st), 2.0, acc, N, nv.stream())
    torch.cuda.synchronize()
    assert (logits.cpu().double() - want).abs().max().item() <= 1e-5
    pw = torch.softmax(want, 1)
    # probs: first pass p / 2, then (p / 2 + p) / 2
    assert (big[:, :ncls].cpu().double() - 0.75 * pw).abs().max().item() <= 1e-5
    assert torch.equal(big[:, ncls].cpu(), torch.zeros_like(big[:, ncls].cpu()))
    assert torch.equal(cls.cpu().long().view(N, *fine), logits.cpu().argmax(1))


@pytest.mark.parametrize('kind', ['ce', 'dice', 'iou', 'mcc', 'dice_ce', 'iou_ce', 'mcc_ce'])
@pytest.mark.parametrize('nd,coarse,s', [(2, (4, 5), 8), (3, (2, 3, 2), 4)])
def test_up_loss_vs_autograd(kind, nd, coarse, s):
    from interactive_unet import _native as nv
    from interactive_unet.train_engine import LOSS_KINDS
    N, ncls, g = 2, 3, torch.Generator().manual_seed(11)
    lc = torch.randn((N, ncls) + coarse, generator=g)
    fine = tuple(c * s for c in coarse)
    y = F.one_hot(torch.randint(0, ncls, (N,) + fine, generator=g), ncls).movedim(-1, 1).float().contiguous()
    wt = (torch.rand((N, 1) + fine, generator=g) > 0.2).float().expand(N, ncls, *fine).contiguous()
    axes = (0,) + tuple(range(2, 2 + nd))
    lcr = lc.double().requires_grad_(True)
    probs = torch.softmax(F.interpolate(lcr, scale_factor=s, mode='trilinear' if nd == 3 else 'bilinear', align_corners=True), 1)
    lv = metrics_ref.loss(kind, probs.detach().numpy(), (y * wt).numpy(), wt.numpy(), axes=axes)
    probs.backward(torch.tensor(metrics_ref.loss_grad(kind, probs.detach().numpy(), (y * wt).numpy(), wt.numpy(), axes=axes)))
    cd = _dims(coarse)
    vf = int(np.prod(fine))
    lib = nv.lib()
    res = []
    for _ in range(2):
        slab = torch.empty(lib.iunet_dl_up_loss_num_parts(N, vf) * ncls * 8, device='cuda')
        out4, coef = torch.empty(4, device='cuda'), torch.empty(ncls * 3, device='cuda')
        yd, wd, lcd = (y * wt).cuda(), wt.cuda(), lc.cuda()
        nv.call('iunet_dl_up_loss_fwd', nd, nv.ptr(lcd), ncls, *cd, s, nv.ptr(yd), nv.ptr(wd), 0, LOSS_KINDS[kind], nv.ptr(slab), nv.ptr(out4),
                nv.ptr(coef), N, nv.stream())
        scale = torch.tensor([4.0], device='cuda')
        dfine, tmp = torch.empty(N * ncls * vf, device='cuda'), torch.empty(N * ncls * vf, device='cuda')
        dlc = torch.empty_like(lcd)
        nv.call('iunet_dl_up_loss_bwd', nd, nv.ptr(lcd), ncls, *cd, s, nv.ptr(yd), nv.ptr(wd), 0, nv.ptr(coef), nv.ptr(scale), nv.ptr(dfine),
                nv.ptr(tmp), nv.ptr(dlc), N, nv.stream())
        torch.cuda.synchronize()
        res.append((out4.cpu(), dlc.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert abs(res[0][0][0].item() - lv) <= 1e-4 * max(1.0, abs(lv))
    got = res[0][1].double() / 4.0
    assert (got - lcr.grad).abs().max().item() <= 1e-4 * max(1e-3, lcr.grad.abs().max().item()) + 1e-7


# ---------------------------------------------------------------------------------------------- 2. forwards
def _margin_ok(cls, r):
    top2 = r.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 2e-3
    return bool((cls[sure] == r.argmax(1)[sure]).all())


@pytest.mark.parametrize('dim,levels,C,rates,shape', [(2, 4, 256, (12, 24, 36), (2, 128, 96)), (3, 4, 64, (12, 24, 36), (1, 32, 48, 32)),
                                                      (3, 3, 96, (1, 2, 3), (2, 16, 24, 20))])
def test_forward_parity(dim, levels, C, rates, shape):
    from interactive_unet.engine_deeplab import DeepLabV3Engine, DeepLabV3EngineF32
    ncls = 3
    p = ref.init_params(dim, levels, 32, 1, ncls, C, seed=11, randomize_bn=True)
    N, sp = shape[0], shape[1:]
    x = torch.tensor(np.random.default_rng(2).integers(0, 256, (N, 1) + sp, dtype=np.uint8))
    r64 = ref.forward_logits(p, x.double() / 255.0, dim, levels, rates).float()
    D, H, W = _dims(sp)
    vox = D * H * W
    xs = (vox, vox, H * W, W, 1)
    e = DeepLabV3EngineF32(dim, levels, 32, 1, ncls, decoder_channels=C, rates=rates)
    e.load_eval({k: v.cuda() for k, v in p.items()})
    logits = torch.empty((N, ncls) + sp, device='cuda')
    cls = torch.empty((N, vox), dtype=torch.uint8, device='cuda')
    e.infer(x.cuda(), xs, N, D, H, W, logits=logits, cls=cls)
    torch.cuda.synchronize()
    err = (logits.cpu() - r64).abs().max().item()
    print(f'{dim}-D L={levels} C={C}: fp32 form max |logit - ref| = {err:.2e}')
    assert err <= 1e-3
    assert _margin_ok(cls.cpu().long().reshape(N, *sp), r64)
    pref = torch.softmax(r64.double(), 1)
    for T, gate in ((torch.float16, 5e-3), (torch.bfloat16, 3e-2)):
        same = torch.softmax(ref.forward_logits(p, x.double() / 255.0, dim, levels, rates, act=T), 1)
        gate = max(gate, 2.0 * (same - pref).abs().max().item())
        e16 = DeepLabV3Engine(dim, levels, 32, 1, ncls, T, decoder_channels=C, rates=rates)
        e16.load_eval({k: v.cuda() for k, v in p.items()})
        probs = torch.empty((N, ncls) + sp, device='cuda')
        e16.infer(x.cuda(), xs, N, D, H, W, probs=probs)
        torch.cuda.synchronize()
        dp = (probs.cpu().double() - pref).abs().max().item()
        print(f'{dim}-D L={levels} C={C}: {T} max |dprob| = {dp:.2e} (gate {gate:.2e})')
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


@pytest.mark.parametrize('dim,sp,dtype,C', [(2, (64, 96), 'fp16', 128), (3, (16, 32, 32), 'bf16', 64)])
def test_train_step_vs_autograd(dim, sp, dtype, C):
    from interactive_unet.train_engine_deeplab import DeepLabV3TrainEngine
    N, ncls, L, rates = 2, 2, 4, (2, 4, 12)
    p0 = ref.init_params(dim, L, 32, 1, ncls, C, seed=5)
    X, y, wt = _batch(dim, N, sp, seed=1)
    act = torch.float16 if dtype == 'fp16' else torch.bfloat16
    axes = (0,) + tuple(range(2, 2 + dim))
    runs = []
    for _ in range(2):
        m = _model(dim, L, act_dtype=dtype, decoder_channels=C, decoder_atrous_rates=rates, decoder_aspp_dropout=0.3)
        m.load_named(p0)
        m = m.cuda()
        te = DeepLabV3TrainEngine(m, lr=1e-3, loss_scale=(256.0 if dtype == 'fp16' else 1.0))
        out = te.train_step(X, y, wt)
        torch.cuda.synchronize()
        runs.append((out, te.grad.cpu().clone(), te.flat.cpu().clone(), te, m, te.last_dropout_mask.cpu()))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2]), 'not deterministic'
    out, _, _, te, m, mask = runs[0]

    def oracle(a):
        pr = {k: v.clone().double().requires_grad_(not unet_ref.is_buffer(k)) for k, v in p0.items()}
        st = {}
        probs = torch.softmax(ref.forward_logits(pr, X, dim, L, rates, training=True, mask=mask, p_drop=0.3, act=a, stats=st), 1)
        lv = metrics_ref.loss('mcc_ce', probs.detach().numpy(), y.numpy(), wt.numpy(), axes=axes)
        probs.backward(torch.tensor(metrics_ref.loss_grad('mcc_ce', probs.detach().numpy(), y.numpy(), wt.numpy(), axes=axes)))
        return pr, st, lv
    pr64, _, lv64 = oracle(None)
    pr, stats, lv = oracle(act)
    print(f'{dim}-D {dtype}: native loss {out["Loss"]:.5f} vs reference (same rounding) {lv:.5f} vs float64 {lv64:.5f}')
    assert abs(out['Loss'] - lv) < (2e-3 if dtype == 'fp16' else 1e-2)
    cosine = lambda a, b: F.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0).item()
    worst, worst_nrm = 1.0, 0.0
    for name in te.names:
        gn = te.g(name).cpu().reshape(pr[name].shape) / te.loss_scale
        c_native, c_ref = cosine(gn, pr64[name].grad), cosine(pr[name].grad, pr64[name].grad)
        worst = min(worst, c_native)
        # the encoder's gradient reaches it through the whole 16-bit backward (no skip connection: the max-pool route only), and the
        # reference rounds only its forward -- the native backward's own roundings widen the gap there, more in bf16 than in fp16
        # (the pooling branch's BatchNorm normalises over N = 2 values per channel: its gradients follow the rounding of X as closely)
        enc = name.startswith('enc') or name.startswith('aspp.pool.')
        tol = (0.06 if enc else 0.02) if dtype == 'fp16' else (0.35 if enc else 0.04)
        assert c_native > c_ref - tol, (name, c_native, c_ref)
        if not enc:
            assert c_native > min(0.85, c_ref - 0.02), (name, c_native, c_ref)
        nrm = (gn.norm() / (pr64[name].grad.norm() + 1e-20)).item()
        nrm_ref = (pr[name].grad.norm() / (pr64[name].grad.norm() + 1e-20)).item()
        assert 0.9 < nrm < 1.1 or abs(nrm - nrm_ref) < (0.05 if not enc else tol), (name, nrm, nrm_ref)
        worst_nrm = max(worst_nrm, abs(nrm - 1.0))
    print(f'   min cos(native, float64) = {worst:.4f}, max |norm ratio - 1| = {worst_nrm:.3f}')
    # running statistics against the same-rounding reference's batch statistics (the pooling branch normalises over N = 2 samples: its
    # output, and with it the projection's mean, follows the 16-bit rounding of X closely)
    for bn in ('enc0.bn1', 'aspp.b1.bn', 'aspp.pool.bn', 'aspp.project.bn', 'dec.bn'):
        mean, var = stats[bn]
        print(bn, 'max |running mean - reference| =', (m.tensor(bn + '.running_mean').cpu().double() - 0.1 * mean).abs().max().item())
        assert torch.allclose(m.tensor(bn + '.running_mean').cpu().double(), 0.1 * mean, atol=2e-3, rtol=2e-2), bn
        assert torch.allclose(m.tensor(bn + '.running_var').cpu().double(), 0.9 + 0.1 * var, rtol=2e-2, atol=2e-2), bn
    with pytest.raises(ValueError, match='more than 1 value per channel'):
        te.train_step(X[:1], y[:1], wt[:1])


# ---------------------------------------------------------------------------------------------- 4. the public interface
def test_module_training_and_validation():
    m = _model(2, 4, decoder_channels=64).cuda()
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
    m = trainer.train_model(lr=1e-3, batch_size=2, epochs=2, architecture='DeepLabV3', pretrained=False, train_loader=loader,
                            val_loader=loader[:1])
    assert os.path.isfile(os.path.join('model', 'model.ckpt'))
    r = UNet.load_from_checkpoint(checkpoint_path=os.path.join('model', 'model.ckpt')).cuda()
    assert r.architecture == 'DeepLabV3'
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
    m3 = _model(3, 4, decoder_channels=64).cuda()
    for mod in (r, m3):
        q = predict.predict_volume_array(mod, vol, input_size=32, num_classes=2)
        torch.cuda.synchronize()
        assert q.numel() == vol.size * 2 and q.dtype == torch.uint8
    mt = _model(2, 4, infer_dtype='fp16').cuda()
    mt.load_named(p)
    pt = mt(xin.cuda()).cpu().double()
    same = torch.softmax(ref.forward_logits(p, xin.double(), 2, 4, act=torch.float16), 1)
    assert (pt - want).abs().max().item() <= max(5e-3, 2.0 * (same - want).abs().max().item())
