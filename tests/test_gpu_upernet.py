"""UPerNet on the MI355X: the kernels of csrc/upernet.hip against float64 torch, the forwards against the CPU reference, one training step
against CPU autograd, and the public interface."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import unet_ref, metrics_ref
from tests import upernet_ref as ref

pytestmark = pytest.mark.gpu

CODE = {torch.float16: 0, torch.bfloat16: 1, torch.float32: 2}
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}        # unit roundoff of the 16-bit formats
DTYPES = [torch.float16, torch.bfloat16, torch.float32]
POISON = 3.0
PAD = 40                                                          # elements between two samples' payloads (keeps 16-byte alignment)


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


def _rnd(T):
    return (lambda t: t) if T == torch.float32 else (lambda t: t.to(T).double())


def _dims(sp):
    return tuple(sp) if len(sp) == 3 else (1,) + tuple(sp)


def _vox(sp):
    return int(np.prod(sp))


def _P(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off * t.element_size())


class Slot:
    """C channels at channel offset 8 of a poisoned tensor of C + 16 channels whose sample stride exceeds its payload."""

    def __init__(self, N, C, sp, T, payload=None):
        self.N, self.C, self.sp, self.T, self.v = N, C, sp, T, _vox(sp)
        self.ss = (C + 16) * self.v + PAD
        self.off = 8 * self.v
        self.buf = torch.full((N * self.ss,), POISON, dtype=T)
        if payload is not None:
            flat = (_blocked(payload, T) if T != torch.float32 else payload.to(T).contiguous()).reshape(N, -1)
            for n in range(N):
                self.buf[n * self.ss + self.off:n * self.ss + self.off + C * self.v] = flat[n]
        self.buf = self.buf.cuda()

    def ptr(self):
        return _P(self.buf, self.off)

    def read(self):
        """(the slot's content as float64 [N, C, *sp], whether every element outside the slot still holds the poison)."""
        b = self.buf.cpu().reshape(self.N, self.ss)
        inside = torch.zeros(self.ss, dtype=torch.bool)
        inside[self.off:self.off + self.C * self.v] = True
        clean = bool((b[:, ~inside] == POISON).all())
        return _load(b[:, inside].contiguous(), self.T, self.C, self.sp), clean


def _gate(T, want):
    """One rounding of an fp32 sum: 16-bit |got - ref| <= 2 u |ref| + 1e-6 max |ref|; the fp32 form 5e-7 max |ref|."""
    m = want.abs().max().item()
    return 5e-7 * m if T == torch.float32 else 2 * U[T] * want.abs() + 1e-6 * m


def _act_bits(sc, sh, x, T):
    """relu(scale x + shift) with iunet_bn_relu_fwd's bits: the fp32 fma (the float64 value rounded once to fp32), the ReLU, then T."""
    shp = (1, -1) + (1,) * (x.dim() - 2)
    return _rnd(T)(torch.relu((sc.double().view(shp) * x + sh.double().view(shp)).float().double()))


# ---------------------------------------------------------------------------------------------- (a) resize into a slot
RESIZE = [(2, (1, 1), (5, 3)), (2, (2, 2), (5, 3)), (2, (3, 3), (6, 10)), (2, (6, 6), (5, 3)), (2, (6, 10), (12, 20)), (2, (3, 5), (12, 20)),
          (2, (12, 20), (12, 20)), (3, (1, 1, 1), (2, 4, 3)), (3, (6, 6, 6), (2, 4, 3)), (3, (2, 4, 3), (4, 8, 6))]


def _resize_call(nv, T, nd, src, src_ss, ssp, act, base, dst, dst_ss, tsp, C, N):
    sc, sh = (None, None) if act is None else (_P(act[0]), _P(act[1]))
    bp, b_ss, bsc, bsh = (None, 0, None, None) if base is None else base
    nv.call('iunet_pn_resize', CODE[T], nd, src, src_ss, *_dims(ssp), sc, sh, bp, b_ss, bsc, bsh, dst, dst_ss, *_dims(tsp), C, N, nv.stream())


@pytest.mark.parametrize('T', DTYPES, ids=['fp16', 'bf16', 'fp32'])
@pytest.mark.parametrize('case', range(len(RESIZE)), ids=[f'{c[1]}to{c[2]}'.replace(' ', '') for c in RESIZE])
def test_resize(T, case):
    from interactive_unet import _native as nv
    nd, ssp, tsp = RESIZE[case]
    N = 2
    worst = 0.0
    for C in (8, 64):
        g = torch.Generator().manual_seed(10 * case + C)
        x = _rnd(T)(torch.randn((N, C) + ssp, generator=g, dtype=torch.float64))
        b = _rnd(T)(torch.randn((N, C) + tsp, generator=g, dtype=torch.float64))
        sc, sh = 0.5 + torch.rand(C, generator=g), 0.3 * torch.randn(C, generator=g)
        bsc, bsh = 0.5 + torch.rand(C, generator=g), 0.3 * torch.randn(C, generator=g)
        dev = [t.cuda() for t in (sc, sh, bsc, bsh)]
        xs = Slot(N, C, ssp, T, payload=x)                   # the source is a slot of a wider tensor too
        for variant in ('plain', 'prologue', 'base', 'raw base'):
            src = _act_bits(sc, sh, x, T) if variant == 'prologue' else x
            want = F.interpolate(src, size=list(tsp), mode=ref.mode(nd), align_corners=False)
            base = None
            if variant in ('base', 'raw base'):
                bs = Slot(N, C, tsp, T, payload=b)
                base = (bs.ptr(), bs.ss, _P(dev[2]), _P(dev[3])) if variant == 'raw base' else (bs.ptr(), bs.ss, None, None)
                want = want + (_act_bits(bsc, bsh, b, T) if variant == 'raw base' else b)
            out = Slot(N, C, tsp, T)
            _resize_call(nv, T, nd, xs.ptr(), xs.ss, ssp, dev[:2] if variant == 'prologue' else None, base, out.ptr(), out.ss, tsp, C, N)
            torch.cuda.synchronize()
            got, clean = out.read()
            assert clean, f'{variant}: bytes outside the slot changed'
            err, gate = (got - want).abs(), _gate(T, want)
            worst = max(worst, (err / gate).max().item())
            assert bool((err <= gate).all()), (variant, C, err.max().item())
    print(f'{T} {ssp} -> {tsp}: worst |got - ref| / gate = {worst:.3f}')


def test_resize_identity_is_a_copy_in_place_base_and_repeat():
    """The identity resize copies bit for bit; base == dst (the lateral added in place) works; a repeated launch is bit-equal."""
    from interactive_unet import _native as nv
    T, N, C, sp, ssp = torch.float16, 2, 16, (6, 10), (3, 5)
    g = torch.Generator().manual_seed(0)
    x = torch.randn((N, C) + sp, generator=g, dtype=torch.float64).to(T)
    xb = _store(x.double(), T)
    out = torch.zeros_like(xb)
    _resize_call(nv, T, 2, _P(xb), C * 60, sp, None, None, _P(out), C * 60, sp, C, N)
    torch.cuda.synchronize()
    assert torch.equal(out, xb)
    s = _rnd(T)(torch.randn((N, C) + ssp, generator=g, dtype=torch.float64))
    sb = _store(s, T)
    outs = []
    for _ in range(2):
        y = xb.clone()
        _resize_call(nv, T, 2, _P(sb), C * 15, ssp, None, (_P(y), C * 60, None, None), _P(y), C * 60, sp, C, N)
        torch.cuda.synchronize()
        outs.append(y)
    assert torch.equal(outs[0], outs[1])
    want = x.double() + F.interpolate(s, size=list(sp), mode='bilinear', align_corners=False)
    assert bool(((_load(outs[0], T, C, sp) - want).abs() <= _gate(T, want)).all())


# ---------------------------------------------------------------------------------------------- (b) its adjoint
# the resize cases, and grids on both sides of the threshold (512 candidate target voxels per source voxel) from which the adjoint runs as
# one workgroup per source voxel: 22 x 22 = 484 below it, 22 x 24 = 528, 23 x 23 = 529 and 8 x 8 x 8 = 512 at or above it
ADJOINT = RESIZE + [(2, (2, 2), (22, 22)), (2, (2, 2), (22, 24)), (2, (1, 1), (23, 23)), (2, (6, 6), (40, 36)), (2, (6, 6), (64, 60)), (3, (2, 1, 2), (8, 8, 8)),
                    (3, (1, 1, 1), (8, 8, 9))]


@pytest.mark.parametrize('T', DTYPES[:2], ids=['fp16', 'bf16'])
@pytest.mark.parametrize('case', range(len(ADJOINT)), ids=[f'{c[1]}to{c[2]}'.replace(' ', '') for c in ADJOINT])
def test_adjoint(T, case):
    """dx = [dx +] R^T(u) against float64 autograd (tests/test_gpu_segformer.py::test_adjoint's tolerance), and <R x, u> = <x, R^T u> on the
    kernels' own outputs: each side is a sum of products with one factor rounded once (relative error u, the fp32 sums far below it), so the
    two sides differ by at most u (sum |R x . u| + sum |x . R^T u|); the gate allows twice that."""
    from interactive_unet import _native as nv
    nd, ssp, tsp = ADJOINT[case]
    N, C = 2, 16
    g = torch.Generator().manual_seed(case)
    u = _rnd(T)(torch.randn((N, C) + tsp, generator=g, dtype=torch.float64))
    d0 = _rnd(T)(torch.randn((N, C) + ssp, generator=g, dtype=torch.float64))
    x = torch.zeros((N, C) + ssp, dtype=torch.float64, requires_grad=True)
    (F.interpolate(x, size=list(tsp), mode=ref.mode(nd), align_corners=False) * u).sum().backward()
    us = Slot(N, C, tsp, T, payload=u)
    for accumulate in (0, 1):
        want = x.grad + (d0 if accumulate else 0)
        outs = []
        for _ in range(2):
            dx = Slot(N, C, ssp, T, payload=d0)
            nv.call('iunet_pn_resize_adjoint', CODE[T], nd, us.ptr(), us.ss, *_dims(tsp), dx.ptr(), dx.ss, *_dims(ssp), C, N, accumulate, nv.stream())
            torch.cuda.synchronize()
            outs.append(dx.buf.clone())
        assert torch.equal(outs[0], outs[1])
        got, clean = dx.read()
        assert clean
        err = (got - want).abs().max().item()
        tol = (2 ** -10 if T == torch.float16 else 2 ** -7) * max(1.0, want.abs().max().item())
        print(f'{T} adjoint {tsp} -> {ssp} accumulate={accumulate}: max err {err:.2e} (tol {tol:.1e})')
        assert err <= tol
        if not accumulate:
            rtu = got
    xin = _rnd(T)(torch.randn((N, C) + ssp, generator=g, dtype=torch.float64))
    xb, rx = _store(xin, T), torch.empty(N * C * _vox(tsp), dtype=T, device='cuda')
    _resize_call(nv, T, nd, _P(xb), C * _vox(ssp), ssp, None, None, _P(rx), C * _vox(tsp), tsp, C, N)
    torch.cuda.synchronize()
    a, b = _load(rx, T, C, tsp) * u, xin * rtu
    assert abs(a.sum().item() - b.sum().item()) <= 2 * U[T] * (a.abs().sum().item() + b.abs().sum().item())


# ---------------------------------------------------------------------------------------------- (b') the two users of csrc/resample.h
# Segformer evaluates the source index in fp32 (resample_axis_f32), UPerNet on the integers (resample_axis_exact).  Between grids whose
# ratio is a power of two both are exact: the same i0 and l1, and where the remainder is 0 they differ only in an i1 whose weight is 0.
# The tap walk, the adjoint's gather order and its zero-weight skips are shared code, so the two architectures' entry points must return
# the same BYTES there.  (target grid, source grids): ratios 1/2, 1, 2 and 4.
DYADIC = [(2, (6, 10), ssp) for ssp in ((3, 5), (6, 10), (12, 20), (24, 40))] + [(3, (2, 4, 6), ssp) for ssp in ((1, 2, 3), (2, 4, 6), (4, 8, 12))]
DYADIC_IDS = [f'{c[2]}to{c[1]}'.replace(' ', '') for c in DYADIC]


def _adj_extent(nin, nout):
    """pn_adj_extent of csrc/resample.h: the candidate target indices per source index on one axis."""
    return min((2 * nout + nin - 1) // nin + 3, nout)


@pytest.mark.parametrize('T', DTYPES[:2], ids=['fp16', 'bf16'])
@pytest.mark.parametrize('case', range(len(DYADIC)), ids=DYADIC_IDS)
def test_dyadic_adjoint_is_segformers_bit_for_bit(T, case):
    from interactive_unet import _native as nv
    nd, tsp, ssp = DYADIC[case]
    N, C = 2, 16
    cand = int(np.prod([_adj_extent(s, t) for s, t in zip(ssp, tsp)]))
    assert cand < 512, 'iunet_pn_resize_adjoint must take its thread-per-voxel form, the only one iunet_sf_adjoint has'
    u = _rnd(T)(torch.randn((N, C) + tsp, generator=torch.Generator().manual_seed(50 + case), dtype=torch.float64))
    us = Slot(N, C, tsp, T, payload=u)
    pn, sf = Slot(N, C, ssp, T), Slot(N, C, ssp, T)
    nv.call('iunet_pn_resize_adjoint', CODE[T], nd, us.ptr(), us.ss, *_dims(tsp), pn.ptr(), pn.ss, *_dims(ssp), C, N, 0, nv.stream())
    nv.call('iunet_sf_adjoint', CODE[T], nd, us.ptr(), us.ss, *_dims(tsp), sf.ptr(), sf.ss, *_dims(ssp), C, N, nv.stream())
    torch.cuda.synchronize()
    assert bool(pn.read()[0].abs().sum() > 0) and torch.equal(pn.buf.view(torch.int16), sf.buf.view(torch.int16))


@pytest.mark.parametrize('T', DTYPES, ids=['fp16', 'bf16', 'fp32'])
@pytest.mark.parametrize('case', range(len(DYADIC)), ids=DYADIC_IDS)
def test_dyadic_resize_is_segformers_gather_bit_for_bit(T, case):
    """iunet_sf_gemm of one source against the identity operator with a zero bias stores its gathered tile: the matrix product with the
    identity is exact, and the second rounding to T changes nothing (the fp32 kernel stores the tile unrounded)."""
    from interactive_unet import _native as nv
    nd, tsp, ssp = DYADIC[case]
    N, C = 2, 32
    g = torch.Generator().manual_seed(70 + case)
    x = _rnd(T)(torch.randn((N, C) + ssp, generator=g, dtype=torch.float64))
    act = [(0.5 + torch.rand(C, generator=g)).cuda(), (0.3 * torch.randn(C, generator=g)).cuda()]
    xs = Slot(N, C, ssp, T, payload=x)
    eye, zero = torch.eye(C, dtype=T, device='cuda'), torch.zeros(C, device='cuda')
    tabs = (nv.ptr_array([xs.ptr().value]), nv.ll_array([xs.ss]), nv.int_array([C]), nv.int_array(list(_dims(ssp))))
    for prologue in (None, act):
        pn, sf = Slot(N, C, tsp, T), Slot(N, C, tsp, T)
        _resize_call(nv, T, nd, xs.ptr(), xs.ss, ssp, prologue, None, pn.ptr(), pn.ss, tsp, C, N)
        sc, sh = (None, None) if prologue is None else (nv.ptr_array([act[0]]), nv.ptr_array([act[1]]))
        nv.call('iunet_sf_gemm', CODE[T], nd, 1, *tabs, sc, sh, _P(eye), _P(zero), sf.ptr(), sf.ss, None, 0, N, *_dims(tsp), C, nv.stream())
        torch.cuda.synchronize()
        bits = torch.int32 if T == torch.float32 else torch.int16
        assert bool(pn.read()[0].abs().sum() > 0) and torch.equal(pn.buf.view(bits), sf.buf.view(bits)), f'prologue {prologue is not None}'


# ---------------------------------------------------------------------------------------------- (c) adaptive average pooling
POOL = [(2, (6, 10)), (2, (5, 3)), (2, (2, 3)), (2, (1, 1)), (3, (2, 4, 3))]


def _pool(x, s, nd):
    return ref.pool(x, s, nd)


@pytest.mark.parametrize('T', DTYPES, ids=['fp16', 'bf16', 'fp32'])
@pytest.mark.parametrize('nd,sp', POOL, ids=[str(c[1]).replace(' ', '') for c in POOL])
def test_pool_forward(T, nd, sp):
    from interactive_unet import _native as nv
    N, C = 2, 16
    x = _rnd(T)(torch.randn((N, C) + sp, generator=torch.Generator().manual_seed(len(sp) + sp[0]), dtype=torch.float64))
    xs = Slot(N, C, sp, T, payload=x)
    runs = []
    for _ in range(2):
        outs = [Slot(N, C, (s,) * nd, T) for s in ref.POOL_SIZES]
        nv.call('iunet_pn_pool', CODE[T], nd, xs.ptr(), xs.ss, *_dims(sp), nv.ptr_array([o.ptr().value for o in outs]),
                nv.ll_array([o.ss for o in outs]), C, N, nv.stream())
        torch.cuda.synchronize()
        runs.append(outs)
    for s, o, o2 in zip(ref.POOL_SIZES, *runs):
        assert torch.equal(o.buf, o2.buf)
        got, clean = o.read()
        assert clean, s
        want = _pool(x, s, nd)
        err, gate = (got - want).abs(), _gate(T, want)
        print(f'{T} pool {sp} -> {s}: worst |got - ref| / gate = {(err / gate).max().item():.3f}')
        assert bool((err <= gate).all()), s


@pytest.mark.parametrize('T', DTYPES[:2], ids=['fp16', 'bf16'])
@pytest.mark.parametrize('nd,sp', POOL, ids=[str(c[1]).replace(' ', '') for c in POOL])
def test_pool_backward(T, nd, sp):
    from interactive_unet import _native as nv
    N, C = 2, 16
    g = torch.Generator().manual_seed(7 + sp[0])
    du = _rnd(T)(torch.randn((N, C) + sp, generator=g, dtype=torch.float64))
    da = [_rnd(T)(torch.randn((N, C) + (s,) * nd, generator=g, dtype=torch.float64)) for s in ref.POOL_SIZES]
    x = torch.zeros((N, C) + sp, dtype=torch.float64, requires_grad=True)
    ((x * du).sum() + sum((_pool(x, s, nd) * a).sum() for s, a in zip(ref.POOL_SIZES, da))).backward()
    dus = Slot(N, C, sp, T, payload=du)
    das = [Slot(N, C, (s,) * nd, T, payload=a) for s, a in zip(ref.POOL_SIZES, da)]
    tabs = nv.ptr_array([a.ptr().value for a in das]), nv.ll_array([a.ss for a in das])
    for with_du in (True, False):
        want = x.grad if with_du else x.grad - du
        outs = []
        for _ in range(2):
            dx = Slot(N, C, sp, T)
            nv.call('iunet_pn_pool_bwd', CODE[T], nd, dus.ptr() if with_du else None, dus.ss, *tabs, dx.ptr(), dx.ss, *_dims(sp), C, N, nv.stream())
            torch.cuda.synchronize()
            outs.append(dx.buf.clone())
        assert torch.equal(outs[0], outs[1])
        got, clean = dx.read()
        assert clean
        err, gate = (got - want).abs(), _gate(T, want)
        print(f'{T} pool backward {sp} du={with_du}: worst |got - ref| / gate = {(err / gate).max().item():.3f}')
        assert bool((err <= gate).all())


@pytest.mark.parametrize('T', DTYPES[:2], ids=['fp16', 'bf16'])
def test_bias_relu_backward(T):
    from interactive_unet import _native as nv
    N, C, v = 3, 64, 1
    g = torch.Generator().manual_seed(2)
    y = _rnd(T)(torch.randn((N, C, 1, 1), generator=g, dtype=torch.float64))
    dz = _rnd(T)(torch.randn((N, C, 1, 1), generator=g, dtype=torch.float64))
    bias = 0.3 * torch.randn(C, generator=g)
    q = _act_bits(torch.ones(C), bias, y, T)
    want = dz * (q > 0)
    yb, dzb, dy, db = _store(y, T), _store(dz, T), torch.zeros(N * C * v, dtype=T, device='cuda'), torch.zeros(C, device='cuda')
    bd = bias.cuda()
    nv.call('iunet_pn_bias_relu_bwd', CODE[T], _P(dzb), C * v, _P(yb), C * v, _P(bd), _P(dy), C * v, _P(db), C, N, v, nv.stream())
    torch.cuda.synchronize()
    assert torch.equal(_load(dy, T, C, (1, 1)), want)
    assert (db.cpu().double() - want.sum((0, 2, 3))).abs().max().item() <= 1e-6 * max(1.0, want.abs().sum((0, 2, 3)).max().item())


# ---------------------------------------------------------------------------------------------- (d) forwards
def _model(dim=2, levels=4, base=32, ncls=2, **kw):
    from interactive_unet.unet import UNet
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return UNet(architecture='UPerNet', num_classes=ncls, dim=dim, levels=levels, base=base, pretrained=False, **kw)


def _margin_ok(cls, r):
    top2 = r.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 2e-3
    return bool((cls[sure] == r.argmax(1)[sure]).all())


@pytest.mark.parametrize('dim,levels,C,shape', [(2, 4, 256, (2, 48, 80)), (2, 4, 64, (1, 40, 24)), (2, 5, 64, (1, 64, 96)), (2, 6, 32, (1, 64, 96)),
                                                (3, 4, 64, (1, 16, 32, 24)), (3, 5, 32, (1, 32, 32, 48))])
def test_forward_parity(dim, levels, C, shape):
    from interactive_unet.engine_upernet import UPerNetEngine, UPerNetEngineF32
    ncls = 3
    p = ref.init_params(dim, levels, 32, 1, ncls, C, seed=11, randomize_bn=True)
    N, sp = shape[0], shape[1:]
    x = torch.tensor(np.random.default_rng(2).integers(0, 256, (N, 1) + sp, dtype=np.uint8))
    r64 = ref.forward_logits(p, x.double() / 255.0, dim, levels).float()
    D, H, W = _dims(sp)
    vox = D * H * W
    xs = (vox, vox, H * W, W, 1)
    e = UPerNetEngineF32(dim, levels, 32, 1, ncls, decoder_channels=C)
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
        e16 = UPerNetEngine(dim, levels, 32, 1, ncls, T, decoder_channels=C)
        e16.load_eval({k: v.cuda() for k, v in p.items()})
        probs = torch.empty((N, ncls) + sp, device='cuda')
        e16.infer(x.cuda(), xs, N, D, H, W, probs=probs)
        torch.cuda.synchronize()
        dp = (probs.cpu().double() - pref).abs().max().item()
        print(f'{dim}-D L={levels} C={C}: {T} max |dprob| = {dp:.2e} (gate {gate:.0e}; same-rounding reference '
              f'{(same - pref).abs().max().item():.2e})')
        assert dp <= gate


# ---------------------------------------------------------------------------------------------- (e) one step against CPU autograd
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
    from interactive_unet.train_engine_upernet import UPerNetTrainEngine
    ncls, L = 2, 4
    p0 = ref.init_params(dim, L, 32, 1, ncls, C, seed=5)
    p0['psp.b1.conv.bias'] = 0.2 * torch.randn(p0['psp.b1.conv.bias'].shape, generator=torch.Generator().manual_seed(9))
    X, y, wt = _batch(dim, N, sp, seed=1)
    act = torch.float16 if dtype == 'fp16' else torch.bfloat16
    axes = (0,) + tuple(range(2, 2 + dim))
    runs = []
    for _ in range(2):
        m = _model(dim, L, act_dtype=dtype, decoder_channels=C)
        m.load_named(p0)
        m = m.cuda()
        te = UPerNetTrainEngine(m, lr=1e-3, loss_scale=(256.0 if dtype == 'fp16' else 1.0))
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
    worst, failed = {}, []
    for name in te.names:
        gn = te.g(name).cpu().reshape(pr[name].shape) / te.loss_scale
        c_native, c_ref = cosine(gn, pr64[name].grad), cosine(pr[name].grad, pr64[name].grad)
        # (psp.b1 .. b3 are normalised over very few values per channel; they hold the decoder's rule all the same: DESIGN has the cosines)
        enc = name.startswith('enc')
        kind = 'encoder' if enc else 'psp.b1-3' if name.startswith(('psp.b1.', 'psp.b2.', 'psp.b3.')) else 'decoder / head'
        if c_native - c_ref < worst.get(kind, (1.0,))[0]:
            worst[kind] = (round(c_native - c_ref, 4), name, round(c_native, 4), round(c_ref, 4))
        tol = (0.06 if enc else 0.02) if dtype == 'fp16' else (0.35 if enc else 0.04)
        if not c_native > c_ref - tol:
            failed.append((name, c_native, c_ref))
    print('   worst cos(native, float64) - cos(reference, float64):', worst)
    assert not failed, failed
    for bn in ('enc0.bn1', 'psp.out.bn', 'lat2.bn', 'fuse.bn'):
        mean, var = stats[bn]
        err = (m.tensor(bn + '.running_mean').cpu().double() - 0.1 * mean).abs().max().item()
        print(f'   {bn}: max |running mean - reference| = {err:.2e}')
        assert torch.allclose(m.tensor(bn + '.running_mean').cpu().double(), 0.1 * mean, atol=2e-3, rtol=2e-2), bn
        assert torch.allclose(m.tensor(bn + '.running_var').cpu().double(), 0.9 + 0.1 * var, rtol=2e-2, atol=2e-2), bn


# ---------------------------------------------------------------------------------------------- (f) the public interface
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
    m = trainer.train_model(lr=1e-3, batch_size=2, epochs=2, architecture='UPerNet', pretrained=False, train_loader=loader,
                            val_loader=loader[:1])
    assert os.path.isfile(os.path.join('model', 'model.ckpt'))
    r = UNet.load_from_checkpoint(checkpoint_path=os.path.join('model', 'model.ckpt')).cuda()
    assert r.architecture == 'UPerNet' and r.decoder_channels == 256
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
    assert (pt - want).abs().max().item() <= 5e-3
