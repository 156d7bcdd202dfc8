"""LinkNet on the MI355X: the decoder-block kernels of csrc/linknet.hip against float64 torch, the forwards against the CPU reference,
one training step against CPU autograd, and the public interface."""
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import unet_ref, metrics_ref
from tests import linknet_ref

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
        return UNet(architecture='LinkNet', num_classes=ncls, dim=dim, levels=levels, base=base, pretrained=False, **kw)


def _dims(sp):
    return sp if len(sp) == 3 else (1,) + tuple(sp)


def _vox(sp):
    return int(np.prod(sp))


# ---------------------------------------------------------------------------------------------- 1. the kernels
KERNEL_CASES = [(2, (5, 7), 16, 32), (2, (1, 9), 32, 16), (3, (3, 1, 5), 16, 16), (3, (2, 3, 4), 32, 48)]


def _ref_op(kind, nd, x, w):
    """float64: kind 0 1x1 conv (w [Cout][Cin]); 1 ConvTranspose k4 s2 p1 (w [Cin][Cout][4^d]); 2 its data gradient applied to x = dy."""
    conv, convT = (F.conv2d, F.conv_transpose2d) if nd == 2 else (F.conv3d, F.conv_transpose3d)
    if kind == 0:
        return conv(x, w.view(*w.shape[:2], *([1] * nd)))
    if kind == 1:
        return convT(x, w, stride=2, padding=1)
    return conv(x, w, stride=2, padding=1)          # the adjoint of the transposed conv: the strided conv with the same weights


@pytest.mark.parametrize('T', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('nd,sp,cin,cout', KERNEL_CASES)
@pytest.mark.parametrize('kind', [0, 1, 2])
def test_conv_fwd_kernels(kind, nd, sp, cin, cout, T):
    """Every gather of iunet_lk_conv_fwd, raw (+ statistics -> iunet_bn_finalize) and with the eval epilogue (+ bias, ReLU, + skip);
    the input activation (prologue) gives the bits of iunet_bn_relu_fwd."""
    from interactive_unet import _native as nv
    g = torch.Generator().manual_seed(kind * 100 + cin + nd)
    N, dt = 2, nv.DTYPE_CODE[T]
    D, H, W = _dims(sp)
    up = tuple(2 * s for s in sp)
    xin_sp, out_sp = (sp, sp) if kind == 0 else (sp, up) if kind == 1 else (up, sp)
    x = (torch.randn((N, cin) + xin_sp, generator=g)).to(T).float()
    if kind == 0:
        w = torch.randn((cout, cin), generator=g) / cin ** 0.5
        pk_kind, pk_co, pk_ci = 0, cout, cin
    elif kind == 1:
        w = torch.randn((cin, cout) + (4,) * nd, generator=g) / (cin * 2 ** nd) ** 0.5
        pk_kind, pk_co, pk_ci = 2, cout, cin
    else:                                             # data gradient of a convT with Cin = cout, Cout = cin (this call's channels)
        w = torch.randn((cout, cin) + (4,) * nd, generator=g) / (cin * 4 ** nd) ** 0.5
        pk_kind, pk_co, pk_ci = 3, cin, cout
    wq = w.to(T).float()
    wd = w.cuda()
    wpk = torch.empty(nv.lib().iunet_lk_pack_elems(nd, pk_kind, pk_co, pk_ci), dtype=T, device='cuda')
    nv.call('iunet_lk_pack', dt, nd, pk_kind, nv.ptr(wd), None, None, None, None, 0.0, nv.ptr(wpk), None, pk_co, pk_ci, nv.stream())
    xb = _blocked(x, T).cuda()
    vin, vout = _vox(xin_sp), _vox(out_sp)
    scale = (0.5 + torch.rand(cin, generator=g)).cuda()
    shift = (0.3 * torch.randn(cin, generator=g)).cuda()
    act = kind != 2
    # raw output with statistics, input through relu(scale x + shift)
    y = torch.empty(N * cout * vout, dtype=T, device='cuda')
    nparts = nv.lib().iunet_lk_stats_parts(nd, kind, N, D, H, W, cout)
    stats = torch.full((nparts * cout * 2,), float('nan'), device='cuda')
    nv.call('iunet_lk_conv_fwd', dt, nd, kind, nv.ptr(xb), cin * vin, nv.ptr(y), cout * vout, nv.ptr(wpk),
            nv.ptr(scale) if act else None, nv.ptr(shift) if act else None, None, None, 0, nv.ptr(stats), 0, N, D, H, W, cin, cout, nv.stream())
    xa = x
    if act:
        shp = [1, -1] + [1] * nd
        xa = (scale.cpu().view(shp) * x + shift.cpu().view(shp)).clamp_min(0).to(T).float()
        # the prologue's bits: the same call on the tensor iunet_bn_relu_fwd stores
        z = torch.empty_like(xb)
        nv.call('iunet_bn_relu_fwd', dt, nv.ptr(xb), cin * vin, nv.ptr(z), cin * vin, nv.ptr(scale), nv.ptr(shift), cin, N, vin, nv.stream())
        y2 = torch.empty_like(y)
        nv.call('iunet_lk_conv_fwd', dt, nd, kind, nv.ptr(z), cin * vin, nv.ptr(y2), cout * vout, nv.ptr(wpk), None, None, None, None, 0,
                None, 0, N, D, H, W, cin, cout, nv.stream())
        torch.cuda.synchronize()
        assert torch.equal(y, y2), 'input activation differs from iunet_bn_relu_fwd + plain launch'
        assert torch.equal(_unblocked(z.cpu(), cin, xin_sp).float(), xa)
    ref = _ref_op(kind, nd, xa.double(), wq.double())
    got = _unblocked(y.cpu().view(N, -1), cout, out_sp).double()
    tol = (2e-3 if T == torch.float16 else 1.6e-2) * ref.abs().max().item()
    assert (got - ref).abs().max().item() <= tol, (got - ref).abs().max().item()
    # statistics -> batch mean / variance
    mean, invstd = torch.empty(cout, device='cuda'), torch.empty(cout, device='cuda')
    sc, sh = torch.empty(cout, device='cuda'), torch.empty(cout, device='cuda')
    ones, zeros = torch.ones(cout, device='cuda'), torch.zeros(cout, device='cuda')
    nv.call('iunet_bn_finalize', nv.ptr(stats), nparts, cout, float(N * vout), nv.ptr(ones), nv.ptr(zeros), None, None, 0.1, 1e-5,
            nv.ptr(sc), nv.ptr(sh), nv.ptr(mean), nv.ptr(invstd), nv.stream())
    torch.cuda.synchronize()
    axes = (0,) + tuple(range(2, 2 + nd))
    rm, rv = ref.mean(axes), ref.var(axes, unbiased=False)
    big = ref.abs().max().item()
    assert torch.allclose(mean.cpu().double(), rm, atol=(1e-3 if T == torch.float16 else 1e-2) * big)
    assert torch.allclose(1.0 / invstd.cpu().double() ** 2 - 1e-5, rv, rtol=2e-2 if T == torch.float16 else 5e-2, atol=1e-3 * big * big)
    # eval epilogue: relu(acc + bias) + skip
    if kind != 2:
        bias = (0.2 * torch.randn(cout, generator=g)).cuda()
        skip = torch.randn((N, cout) + out_sp, generator=g).to(T).float()
        sb = _blocked(skip, T).cuda()
        y3 = torch.empty_like(y)
        nv.call('iunet_lk_conv_fwd', dt, nd, kind, nv.ptr(xb), cin * vin, nv.ptr(y3), cout * vout, nv.ptr(wpk), None, None, nv.ptr(bias),
                nv.ptr(sb), cout * vout, None, 1, N, D, H, W, cin, cout, nv.stream())
        torch.cuda.synchronize()
        shp = [1, -1] + [1] * nd
        ref3 = (_ref_op(kind, nd, x.double(), wq.double()) + bias.cpu().double().view(shp)).clamp_min(0) + skip.double()
        got3 = _unblocked(y3.cpu().view(N, -1), cout, out_sp).double()
        assert (got3 - ref3).abs().max().item() <= (2e-3 if T == torch.float16 else 1.6e-2) * ref3.abs().max().item()


@pytest.mark.parametrize('T', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('nd,sp,cin,cout', KERNEL_CASES)
@pytest.mark.parametrize('kind', [0, 1])
def test_wgrad_kernels(kind, nd, sp, cin, cout, T):
    from interactive_unet import _native as nv
    g = torch.Generator().manual_seed(kind * 31 + cin + nd)
    N, dt = 2, nv.DTYPE_CODE[T]
    D, H, W = _dims(sp)
    out_sp = sp if kind == 0 else tuple(2 * s for s in sp)
    x = torch.randn((N, cin) + tuple(sp), generator=g).to(T).float()
    dy = torch.randn((N, cout) + out_sp, generator=g).to(T).float()
    scale = (0.5 + torch.rand(cin, generator=g)).cuda()
    shift = (0.3 * torch.randn(cin, generator=g)).cuda()
    xb, dyb = _blocked(x, T).cuda(), _blocked(dy, T).cuda()
    nslab = nv.lib().iunet_lk_wgrad_slab_floats(nd, kind, N, D, H, W, cin, cout)
    slab = torch.empty(nslab, device='cuda')
    wshape = (cout, cin) if kind == 0 else (cin, cout) + (4,) * nd
    dW = torch.full(wshape, float('nan'), device='cuda')
    nv.call('iunet_lk_wgrad', dt, nd, kind, nv.ptr(xb), cin * _vox(sp), nv.ptr(dyb), cout * _vox(out_sp), nv.ptr(scale), nv.ptr(shift),
            nv.ptr(slab), nv.ptr(dW), 0.5, N, D, H, W, cin, cout, nv.stream())
    torch.cuda.synchronize()
    shp = [1, -1] + [1] * nd
    xa = (scale.cpu().view(shp) * x + shift.cpu().view(shp)).clamp_min(0).to(T).double().requires_grad_(False)
    wr = torch.zeros(wshape, dtype=torch.float64, requires_grad=True)
    _ref_op(kind, nd, xa, wr).backward(dy.double())
    ref = 0.5 * wr.grad
    err = (dW.cpu().double() - ref).abs().max().item()
    assert err <= 1e-4 * ref.abs().max().item() + 1e-6, err
    # twice: the same bits
    dW2 = torch.empty_like(dW)
    nv.call('iunet_lk_wgrad', dt, nd, kind, nv.ptr(xb), cin * _vox(sp), nv.ptr(dyb), cout * _vox(out_sp), nv.ptr(scale), nv.ptr(shift),
            nv.ptr(slab), nv.ptr(dW2), 0.5, N, D, H, W, cin, cout, nv.stream())
    torch.cuda.synchronize()
    assert torch.equal(dW, dW2)


@pytest.mark.parametrize('T', [torch.float16, torch.bfloat16])
def test_bn_relu_add(T):
    from interactive_unet import _native as nv
    g = torch.Generator().manual_seed(3)
    N, C, sp = 2, 32, (7, 9)
    y = torch.randn((N, C) + sp, generator=g).to(T).float()
    s = torch.randn((N, C) + sp, generator=g).to(T).float()
    sc, sh = 0.5 + torch.rand(C, generator=g), 0.3 * torch.randn(C, generator=g)
    out = torch.empty(N * C * 63, dtype=T, device='cuda')
    yb, sb, scd, shd = _blocked(y, T).cuda(), _blocked(s, T).cuda(), sc.cuda(), sh.cuda()     # (alive until the launch has run)
    nv.call('iunet_lk_bn_relu_add', nv.DTYPE_CODE[T], nv.ptr(yb), C * 63, nv.ptr(sb), C * 63, nv.ptr(out), C * 63, nv.ptr(scd), nv.ptr(shd),
            C, N, 63, nv.stream())
    torch.cuda.synchronize()
    shp = [1, -1, 1, 1]
    a = (sh.double().view(shp) + sc.double().view(shp) * y.double()).float().clamp_min(0)      # fmaf: one rounding to fp32
    want = (a + s).to(T)                                                                          # fp32 sum, one rounding to T
    assert torch.equal(_unblocked(out.cpu().view(N, -1), C, sp), want)


@pytest.mark.parametrize('nd,sp,cin,cout', KERNEL_CASES)
@pytest.mark.parametrize('kind', [0, 1])
def test_f32_kernels(kind, nd, sp, cin, cout):
    from interactive_unet import _native as nv
    g = torch.Generator().manual_seed(kind * 7 + cin)
    N = 2
    D, H, W = _dims(sp)
    out_sp = sp if kind == 0 else tuple(2 * s for s in sp)
    x = torch.randn((N, cin) + tuple(sp), generator=g)
    w = torch.randn((cout, cin) if kind == 0 else (cin, cout) + (4,) * nd, generator=g) / cin ** 0.5
    gam, bet = 0.5 + torch.rand(cout, generator=g), 0.2 * torch.randn(cout, generator=g)
    mu, var = 0.2 * torch.randn(cout, generator=g), 0.5 + torch.rand(cout, generator=g)
    pk_kind = 0 if kind == 0 else 2
    wpk = torch.empty(nv.lib().iunet_lk_pack_elems(nd, pk_kind, cout, cin), device='cuda')
    bias = torch.empty(cout, device='cuda')
    dev = [t.cuda() for t in (w, gam, bet, mu, var)]          # (alive until the launches have run)
    nv.call('iunet_lk_pack', 2, nd, pk_kind, *[nv.ptr(t) for t in dev], 1e-5, nv.ptr(wpk), nv.ptr(bias), cout, cin, nv.stream())
    skip = torch.randn((N, cout) + out_sp, generator=g) if kind == 0 else None
    skd = None if skip is None else skip.cuda()
    xd = x.cuda()
    y = torch.empty((N, cout) + out_sp, device='cuda')
    nv.call('iunet_lk_f32_conv_fwd', nd, kind, nv.ptr(xd), cin * _vox(sp), nv.ptr(y), cout * _vox(out_sp), nv.ptr(wpk), nv.ptr(bias),
            nv.ptr(skd), cout * _vox(out_sp), N, D, H, W, cin, cout, nv.stream())
    torch.cuda.synchronize()
    a = gam.double() / torch.sqrt(var.double() + 1e-5)
    shp = [1, -1] + [1] * nd
    ref = (_ref_op(kind, nd, x.double(), w.double()) * a.view(shp) + (bet.double() - mu.double() * a).view(shp)).clamp_min(0)
    if skip is not None:
        ref = ref + skip.double()
    assert (y.cpu().double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()


# ---------------------------------------------------------------------------------------------- 2. forward parity
def _margin_ok(cls, ref):
    top2 = ref.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 2e-3
    return bool((cls[sure] == ref.argmax(1)[sure]).all())


@pytest.mark.parametrize('dim,levels,base,ncls,shape', [(2, 4, 32, 2, (2, 256, 256)), (3, 4, 32, 2, (1, 64, 64, 64)),
                                                        (3, 5, 64, 4, (1, 32, 32, 48))])
def test_forward_parity(dim, levels, base, ncls, shape):
    from interactive_unet.engine_linknet import LinkNetEngine, LinkNetEngineF32
    p = linknet_ref.init_params(dim, levels, base, 1, ncls, seed=11, randomize_bn=True)
    N, sp = shape[0], shape[1:]
    x = torch.tensor(np.random.default_rng(2).integers(0, 256, (N, 1) + sp, dtype=np.uint8))
    ref = linknet_ref.forward_logits(p, x.double() / 255.0, dim, levels, dtype=torch.float64).float()
    D, H, W = sp if dim == 3 else (1,) + sp
    vox = D * H * W
    xs = (vox, vox, H * W, W, 1)
    e = LinkNetEngineF32(dim, levels, base, 1, ncls)
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
        # the 16-bit format itself: the CPU reference rounding at the same points is off the float64 one by this much (2-D 2 x 256^2, fp16:
        # 1.2e-2, bf16: 8.2e-2 -- above the 5e-3 / 3e-2 promised for the U-Net: the skip adds carry the rounding of every level up)
        same = torch.softmax(linknet_ref.forward_logits(p, x.float() / 255.0, dim, levels, act_dtype=T), 1)
        gate = max(gate, 2.0 * (same.double() - pref.double()).abs().max().item())
        e16 = LinkNetEngine(dim, levels, base, 1, ncls, T)
        e16.load_eval({k: v.cuda() for k, v in p.items()})
        probs = torch.empty((N, ncls) + sp, device='cuda')
        e16.infer(x.cuda(), xs, N, D, H, W, probs=probs)
        torch.cuda.synchronize()
        dp = (probs.cpu() - pref).abs().max().item()
        print(f'{dim}-D L={levels} base {base}: {T} max |dprob| = {dp:.2e}')
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


@pytest.mark.parametrize('dim,sp,dtype', [(2, (64, 96), 'fp16'), (3, (16, 32, 32), 'bf16')])
def test_train_step_vs_autograd(dim, sp, dtype):
    from interactive_unet.train_engine_linknet import LinkNetTrainEngine
    N, ncls, L = 2, 2, 4
    p0 = linknet_ref.init_params(dim, L, 32, 1, ncls, seed=5)
    X, y, wt = _batch(dim, N, sp, seed=1)
    act = torch.float16 if dtype == 'fp16' else torch.bfloat16
    axes = (0,) + tuple(range(2, 2 + dim))

    def oracle(act_dtype):
        pr = {k: v.clone().requires_grad_(not unet_ref.is_buffer(k)) for k, v in p0.items()}
        st = {}
        probs = torch.softmax(linknet_ref.forward_logits(pr, X, dim, L, training=True, act_dtype=act_dtype, bn_stats_out=st), 1)
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
        te = LinkNetTrainEngine(m, lr=1e-3, loss_scale=(256.0 if dtype == 'fp16' else 1.0))
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
        assert c_native > min(0.85, c_ref - 0.02), (name, c_native, c_ref)      # (3-D bf16: the reference's enc2.conv1 is below 0.85)
        if name.startswith('head') or name.startswith('dec0.'):
            # (dec0.conv1 / bn1 / up read D^1 through two 16-channel BatchNorms: the same-rounding reference itself is at 0.998 there)
            assert c_native > min(0.9995 if dtype == 'fp16' else 0.999, c_ref - (1e-3 if dtype == 'fp16' else 4e-3)), (name, c_native, c_ref)
        nrm = (gn.norm() / (pr32[name].grad.norm() + 1e-20)).item()
        assert 0.9 < nrm < 1.1, (name, nrm)
    print(f'   min cos(native, fp32) = {worst:.4f}')
    for bn in ('enc0.bn1', 'dec0.bn1', 'dec0.bn2', 'dec0.bn3', f'dec{L - 2}.bn2'):
        mean, var = stats[bn]
        assert torch.allclose(m.tensor(bn + '.running_mean').cpu(), 0.1 * mean, atol=2e-3), bn
        assert torch.allclose(m.tensor(bn + '.running_var').cpu(), 0.9 + 0.1 * var, rtol=2e-2, atol=2e-2), bn


# ---------------------------------------------------------------------------------------------- 4. the public interface
def test_training_lowers_loss_and_autograd_grads():
    m = _model(2, 4).cuda()
    X, y, wt = _batch(2, 2, (64, 64), seed=3)
    te = m.train_engine()
    losses = [te.train_step(X, y, wt)['Loss'] for _ in range(10)]
    print('loss over ten steps:', ' '.join(f'{v:.4f}' for v in losses))
    assert losses[-1] < losses[0]
    val = te.eval_step(X, y, wt)
    assert np.isfinite(val['Loss'])
    for prm in m.parameters():
        prm.grad = None
    loss = m.training_step((X, y, wt))
    scale = te.loss_scale
    loss.backward()
    flat = te.grad * (1.0 / scale)
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
    m = trainer.train_model(lr=1e-3, epochs=2, architecture='LinkNet', pretrained=False, train_loader=loader, val_loader=loader[:1])
    assert os.path.isfile(os.path.join('model', 'model.ckpt'))
    r = UNet.load_from_checkpoint(checkpoint_path=os.path.join('model', 'model.ckpt')).cuda()
    assert r.architecture == 'LinkNet'
    xin = X[:1].cuda()
    a, b = m.cuda()(xin), r(xin)
    if torch.equal(torch.cat([t.reshape(-1) for t in m.named_tensors().values()]).cpu(),
                   torch.cat([t.reshape(-1) for t in r.named_tensors().values()]).cpu()):
        assert torch.equal(a, b)
    assert predict.find_max_batch_size(r, input_size=256) >= 4
    img = (np.random.default_rng(8).random((64, 96)) * 255).astype(np.uint8)
    rgb = predict.predict_slice(img, model=r)
    assert tuple(np.asarray(rgb.cpu() if torch.is_tensor(rgb) else rgb).shape) == (64, 96, 3)
    p = {k: v.detach().cpu() for k, v in r.named_tensors().items()}
    blk = torch.rand((32, 32, 32), generator=torch.Generator().manual_seed(5))
    got = predict.predict_block(r, blk, num_classes=2, batch_size=32)
    ref = 0
    for axis in (0, 1, 2):
        sl = blk.movedim(axis, 0)[:, None]
        pr = linknet_ref.forward(p, sl.double(), 2, 4, dtype=torch.float64).float()
        ref = ref + pr.permute(0, 2, 3, 1).movedim(0, axis)
    ref = ref / 3
    err = np.abs(got - ref.numpy()).max()
    print(f'2.5-D block: max |dprob| vs reference {err:.2e}')
    assert err <= 1e-3
    vol = (np.random.default_rng(6).random((40, 48, 56)) * 255).astype(np.uint8)
    m3 = _model(3, 4).cuda()
    for mod in (r, m3):
        q = predict.predict_volume_array(mod, vol, input_size=32, num_classes=2)
        torch.cuda.synchronize()
        assert q.numel() == vol.size * 2 and q.dtype == torch.uint8
    v3 = torch.rand((1, 1, 32, 32, 32), generator=torch.Generator().manual_seed(7))
    p3 = {k: v.detach().cpu() for k, v in m3.named_tensors().items()}
    err3 = (m3(v3.cuda()).cpu() - linknet_ref.forward(p3, v3.double(), 3, 4, dtype=torch.float64).float()).abs().max().item()
    print(f'3-D forward through the module: max |dprob| vs reference {err3:.2e}')
    assert err3 <= 1e-3
    for T in ('fp16', 'bf16'):
        mt = _model(2, 4, infer_dtype=T).cuda()
        mt.load_named(p)
        pt = mt(xin).cpu()
        r64 = linknet_ref.forward(p, X[:1].double(), 2, 4, dtype=torch.float64)
        same = linknet_ref.forward(p, X[:1], 2, 4, act_dtype=torch.float16 if T == 'fp16' else torch.bfloat16)
        gate = max(5e-3 if T == 'fp16' else 3e-2, 2.0 * (same.double() - r64).abs().max().item())
        assert (pt.double() - r64).abs().max().item() <= gate
