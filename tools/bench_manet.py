"""MA-Net against U-Net at the same shape: the 16-bit training step (MCC+CE, GPU time from HIP events, mean of n runs after warm-up) at
8 x 512^2 fp16 and 2 x 128^3 bf16 (L = 4, base 32: T = 4096 tokens and Cb = 256 in both), both sequenced from Python (the U-Net's C handle
off), and the kernels of csrc/manet.hip at those shapes, each on its own: the call time (HIP events around n back-to-back launches), for
the attention kernels beside the matrix work they do (recomputed products included), for the gated upsampling beside the bytes it has to
move at 6.3 TB/s.  The U-Net's step measured in the same run is the yardstick.
    python tools/bench_manet.py"""
import math, os, sys, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'interactive-unet_amd'))

HBM = 6.3e12            # bytes / s
SHAPES = ((2, 8, (512, 512), 'fp16'), (3, 2, (128, 128, 128), 'bf16'))
K, CH = 64, 128         # query / key width; channels of the second product per workgroup


def attention_flops(T, Cb, N):
    """Multiply-adds x 2 of (forward, row launch, column launch, fp32 forward) as the kernels run them: the forward recomputes S per 128
    channels; the row launch computes S and dP twice and dKc once; the column launch computes S per 128 channels of dV and once more with dP
    for dQ."""
    pair, nch = 2.0 * N * T * T, Cb // CH
    return (pair * (nch * K + Cb), pair * (2 * (K + Cb) + K), pair * (nch * (K + CH) + 2 * K + Cb), pair * (nch * K + Cb))


def main():
    import torch
    from interactive_unet.unet import UNet
    from interactive_unet import _native as nv

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

    torch.manual_seed(0)
    levels, base = 4, 32
    ch = [base * 2 ** l for l in range(levels)]
    for dim, N, sp, act in SHAPES:
        X = torch.rand((N, 1) + sp, device='cuda')
        lab = X[:, 0] > 0.5
        y = torch.stack([~lab, lab], 1).half()
        w = torch.ones_like(y)
        t = {}
        for arch in ('U-Net', 'MA-Net'):
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                m = UNet(architecture=arch, dim=dim, pretrained=False, act_dtype=act).cuda()
            te = m.train_engine()
            te.use_handle = False
            t[arch] = timed(lambda: te.train_step(X, y, w, sync=False))
            del te, m
            torch.cuda.empty_cache()
        unet = t['U-Net']
        print(f'train step {dim}-D {N} x {sp} {act}: U-Net {unet:9.2f} ms   MA-Net {t["MA-Net"]:9.2f} ms   MA-Net / U-Net {t["MA-Net"] / unet:.3f}')
        Tt = torch.float16 if act == 'fp16' else torch.bfloat16
        code, s = nv.DTYPE_CODE[Tt], nv.stream()
        grids = [tuple(x >> l for x in sp) if dim == 3 else (1,) + tuple(x >> l for x in sp) for l in range(levels)]
        T, Cb = math.prod(grids[-1]), ch[-1]
        rnd = lambda n, dt=Tt, f=1.0: (f * torch.randn(n, device='cuda')).to(dt)
        total = 0.0
        for dt, name in ((Tt, act), (torch.float32, 'fp32')):
            q, k = rnd(N * K * T, dt, 0.35), rnd(N * K * T, dt, 0.35)               # |S| of a few units: a softmax that is neither flat nor one-hot
            v, x, dy, yo, dv = [rnd(N * Cb * T, dt) for _ in range(5)]
            dq, dk = rnd(N * K * T, dt), rnd(N * K * T, dt)
            bq, bk, bv = rnd(K, torch.float32, 0.1), rnd(K, torch.float32, 0.1), rnd(Cb, torch.float32, 0.1)
            lse, delta = torch.empty(N * T, device='cuda'), torch.empty(N * T, device='cuda')
            io = (nv.ptr(q), K * T, nv.ptr(bq), nv.ptr(k), K * T, nv.ptr(bk), nv.ptr(v), Cb * T)
            fl = attention_flops(T, Cb, N)
            if dt == torch.float32:
                rows = [('attention forward, fp32', fl[3], lambda: nv.call('iunet_ma_f32_attn_fwd', *io, nv.ptr(x), Cb * T, nv.ptr(bv), nv.ptr(yo),
                                                                            Cb * T, nv.ptr(lse), Cb, T, N, s))]
            else:
                fwd = lambda: nv.call('iunet_ma_attn_fwd', code, *io, nv.ptr(x), Cb * T, nv.ptr(bv), nv.ptr(yo), Cb * T, nv.ptr(lse), Cb, T, N, s)
                bwd = lambda: nv.call('iunet_ma_attn_bwd', code, *io, nv.ptr(dy), Cb * T, nv.ptr(lse), nv.ptr(delta), nv.ptr(dq), K * T, nv.ptr(dk),
                                      K * T, nv.ptr(dv), Cb * T, Cb, T, N, s)
                rows = [(f'attention forward, {name}', fl[0], fwd), (f'attention backward (both launches), {name}', fl[1] + fl[2], bwd)]
            for label, flops, fn in rows:
                ms = timed(fn, n=20, warm=3)
                if dt != torch.float32:
                    total += ms
                print(f'  {label:46s} T {T} Cb {Cb} N {N}: {ms * 1e3:9.1f} us  {flops / ms / 1e9:7.1f} TFLOP/s  = {ms / unet:.3f} of the U-Net step')
        for l in range(levels - 2, -1, -1):                  # the gated upsampling into dec{l}'s concat buffer and its backward
            g, c = grids[l + 1], ch[l]
            vc, vf = math.prod(g), math.prod(grids[l])
            h, u, dh = rnd(N * c * vc), rnd(N * 2 * c * vf), rnd(N * c * vc)
            sc, gate, dg = torch.ones(c, device='cuda'), torch.rand(N * c, device='cuda') + 0.5, torch.empty(N * c, device='cuda')
            part = torch.empty(nv.answer(nv.lib().iunet_ma_up_gate_dg_parts(dim, N, *g, c)) * N * c, device='cuda')
            calls = [(f'up-gate into dec{l}', N * c * (vc + vf) * 2,
                      lambda: nv.call('iunet_ma_up_gate', code, dim, nv.ptr(h), c * vc, nv.ptr(sc), nv.ptr(sc), nv.ptr(gate), nv.ptr(u), 2 * c * vf,
                                      *g, c, N, s)),
                     (f'up-gate backward dec{l}: dg', N * c * (vc + vf) * 2,
                      lambda: nv.call('iunet_ma_up_gate_dg', code, dim, nv.ptr(u), 2 * c * vf, nv.ptr(h), c * vc, nv.ptr(sc), nv.ptr(sc),
                                      nv.ptr(part), nv.ptr(dg), *g, c, N, s)),
                     (f'up-gate backward dec{l}: dh', N * c * (vc + vf) * 2,
                      lambda: nv.call('iunet_ma_up_gate_bwd', code, dim, nv.ptr(u), 2 * c * vf, nv.ptr(gate), nv.ptr(dg), nv.ptr(dh), c * vc,
                                      *g, c, N, s))]
            for label, nbytes, fn in calls:
                us = timed(fn, n=50, warm=5) * 1e3
                total += us / 1e3
                print(f'  {label:46s} {nbytes / 1e6:8.2f} MB  bound {nbytes / HBM * 1e6:7.2f} us  call {us:8.2f} us')
        print(f'  a partial sum (the attention forward and backward and the three up-gate kernels per block; not the gates, the means, the '
              f'mean-gradient adds or any conv): {total:.2f} ms = {total / t["MA-Net"]:.3f} of the MA-Net step')


if __name__ == '__main__':
    main()
