"""Segformer against U-Net at the same shape: the 16-bit training step (MCC+CE, GPU time from HIP events, mean of n runs after warm-up) at
8 x 512^2 fp16 and at 2 x 128^3 bf16 (BASELINE config C3's shape), and one S^3 2.5-D block prediction (every axis' slices through the
2-D net) in each model's default prediction form (Segformer fp32, U-Net split precision) and in fp16.  Both training steps are sequenced
from Python (the U-Net's C handle off), so the comparison is of the launches, not of the sequencing.  It also prints the shape bounds of
the new kernels (bytes at 6.3 TB/s, dense FLOPs at 2.5 PFLOP/s for 16-bit): `python tools/bench_segformer.py bounds` needs no GPU.
`python tools/bench_segformer.py adjoint` times iunet_sf_adjoint alone, per level, at the grids of its bound.
    python tools/bench_segformer.py [block | bounds | adjoint]"""
import math, os, sys, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'interactive-unet_amd'))

HBM = 6.3e12            # bytes / s
MFMA16 = 2.5e15         # dense 16-bit FLOP / s


def bounds(dim, N, sp, C=256, levels=4, base=32, es=2):
    """{kernel: (bytes, flops)} of the new kernels of one training step, from shapes alone."""
    ch = [base * 2 ** l for l in range(levels)]
    vox = [N * math.prod(x >> l for x in sp) for l in range(levels)]
    vt = vox[2]
    K = sum(ch)
    src = sum(c * v for c, v in zip(ch, vox)) * es          # every encoder output read once (the taps hit the caches)
    out = {}
    out['sf_gemm (forward)'] = (src + C * vt * es + C * K * es, 2.0 * C * K * vt)
    out['sf_wgrad'] = (src + C * vt * es, 2.0 * C * K * vt)
    out['dl_conv_fwd (U = M^T dZ)'] = (C * vt * es + K * vt * es, 2.0 * C * K * vt)
    out['sf_adjoint (all levels)'] = (K * vt * es + src, 0.0)
    out['sf_pack + sf_param_grads'] = (4 * (levels * C * C + C * K) * 3, 2.0 * 3 * C * C * K)
    out['literal smp order (forward, for comparison)'] = (sum(C * v * es * 2 for v in vox) + levels * C * vt * es * 2, 2.0 * C * K * max(vox))
    return out


def print_bounds():
    for dim, N, sp in ((2, 8, (512, 512)), (3, 2, (128, 128, 128))):
        print(f'bounds at {dim}-D {N} x {sp}, C = 256, L = 4 (16-bit):')
        for k, (b, f) in bounds(dim, N, sp).items():
            print(f'  {k:45s} {b / 1e6:10.1f} MB {b / HBM * 1e6:8.1f} us   {f / 1e9:8.1f} GFLOP {f / MFMA16 * 1e6:8.1f} us')


def time_adjoint(levels=4, base=32, n=20, warm=3):
    """iunet_sf_adjoint alone, per level, at the grids of the 'sf_adjoint (all levels)' bound: u [N][ch_l] on T, dx on level l's grid."""
    import ctypes
    import torch
    from interactive_unet import _native as nv
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    for dim, N, sp, T in ((2, 8, (512, 512), torch.float16), (3, 2, (128, 128, 128), torch.bfloat16)):
        tg = [x >> 2 for x in sp]
        Dt, Ht, Wt = tg if dim == 3 else [1] + tg
        ts = []
        for l in range(levels):
            C, sg = base * 2 ** l, [x >> l for x in sp]
            Ds, Hs, Ws = sg if dim == 3 else [1] + sg
            u = torch.randn(N * C * Dt * Ht * Wt, device='cuda').to(T)
            dx = torch.empty(N * C * Ds * Hs * Ws, dtype=T, device='cuda')
            fn = lambda: nv.call('iunet_sf_adjoint', nv.DTYPE_CODE[T], dim, P(u), C * Dt * Ht * Wt, Dt, Ht, Wt, P(dx), C * Ds * Hs * Ws, Ds, Hs, Ws,
                                 C, N, nv.stream())
            for _ in range(warm):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / n * 1e3)
        b = bounds(dim, N, sp, levels=levels, base=base)['sf_adjoint (all levels)'][0]
        print(f'sf_adjoint {dim}-D {N} x {sp} {str(T)[6:]}: levels ' + ' + '.join(f'{t:.1f}' for t in ts) +
              f' = {sum(ts):.1f} us   (bound {b / HBM * 1e6:.1f} us)')


def main():
    import torch
    from interactive_unet.unet import UNet
    from interactive_unet import predict
    BLK = int(sys.argv[1]) if len(sys.argv) > 1 else 128

    def timed(fn, n=10, warm=3):
        for _ in range(warm):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def model(arch, dim, **kw):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            return UNet(architecture=arch, dim=dim, pretrained=False, **kw).cuda()

    torch.manual_seed(0)
    rows = []
    for dim, N, sp, act in ((2, 8, (512, 512), 'fp16'), (3, 2, (128, 128, 128), 'bf16')):
        X = torch.rand((N, 1) + sp, device='cuda')
        lab = X[:, 0] > 0.5
        y = torch.stack([~lab, lab], 1).half()
        w = torch.ones_like(y)
        t = {}
        for arch in ('U-Net', 'Segformer'):
            m = model(arch, dim, act_dtype=act)
            te = m.train_engine()
            te.use_handle = False
            t[arch] = timed(lambda: te.train_step(X, y, w, sync=False))
            del te, m
            torch.cuda.empty_cache()
        rows.append((f'train step {dim}-D {N} x {sp} {act}', t))
    blk = torch.rand((BLK,) * 3, device='cuda')
    for form in ('default', 'fp16'):
        t = {}
        for arch in ('U-Net', 'Segformer'):
            kw = {} if form == 'default' else dict(infer_dtype='fp16')
            m = model(arch, 2, **kw).eval()
            out = torch.zeros((BLK,) * 3 + (2,), device='cuda')
            t[arch] = timed(lambda: predict.predict_block_device(m, blk, out, num_classes=2, batch_size=BLK), n=5, warm=2)
        rows.append((f'2.5-D block {BLK}^3, {form} form', t))
    for name, t in rows:
        print(f'{name:45s} U-Net {t["U-Net"]:9.2f} ms   Segformer {t["Segformer"]:9.2f} ms   Segformer / U-Net {t["Segformer"] / t["U-Net"]:.3f}')
    print_bounds()


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'bounds':
        print_bounds()
    elif len(sys.argv) > 1 and sys.argv[1] == 'adjoint':
        time_adjoint()
    else:
        main()
