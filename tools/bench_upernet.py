"""UPerNet against U-Net at the same shape: the 16-bit training step (MCC+CE, GPU time from HIP events, mean of n runs after warm-up) at
8 x 512^2 fp16 and at 2 x 128^3 bf16 (BASELINE config C3's shape), both sequenced from Python (the U-Net's C handle off), and every new
kernel of csrc/upernet.hip on its own at those shapes: the call time (HIP events around n back-to-back launches) beside the bytes the
kernel has to move at 6.3 TB/s.  None of them has matrix work: the memory bound is the bound.  `python tools/bench_upernet.py bounds`
prints the shape bounds alone and needs no GPU.
    python tools/bench_upernet.py [bounds]"""
import math, os, sys, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'interactive-unet_amd'))

HBM = 6.3e12            # bytes / s
SHAPES = ((2, 8, (512, 512), 'fp16'), (3, 2, (128, 128, 128), 'bf16'))
SIZES = (1, 2, 3, 6)


def grids(dim, sp, levels):
    return [tuple(x >> l for x in sp) if dim == 3 else (1,) + tuple(x >> l for x in sp) for l in range(levels)]


def launches(dim, N, sp, C=256, levels=4, base=32):
    """[(name, entry point, bytes moved, shape arguments)] of every launch of the new kernels in one training step (L = 4: one lateral)."""
    ch = [base * 2 ** l for l in range(levels)]
    g = grids(dim, sp, levels)
    v = [math.prod(x) for x in g]
    B, Cb, Cq, es = levels - 1, ch[-1], ch[-1] // 4, 2
    bins = sum(s ** dim for s in SIZES)
    out = [('pool: A_s of X^B', 'pool', N * Cb * (v[B] + bins) * es, (g[B], Cb)),
           ('resize: X^B into U (identity)', 'resize', 2 * N * Cb * v[B] * es, (g[B], g[B], Cb, False))]
    for s in SIZES:
        gs = (s,) * 3 if dim == 3 else (1, s, s)
        out.append((f'resize: act(Q_{s}) into U', 'resize', N * Cq * (s ** dim + v[B]) * es, (gs, g[B], Cq, True)))
        out.append((f'adjoint: dU slot -> dQ_{s}', 'adjoint', N * Cq * (s ** dim + v[B]) * es, (g[B], gs, Cq, False)))
    for l in range(B - 1, 1, -1):
        out.append((f'resize: P^{l} = act(lat{l}) + R(P^{l + 1})', 'resize_base', N * C * (v[l + 1] + 2 * v[l]) * es, (g[l + 1], g[l], C, False)))
        out.append((f'adjoint: dV slot -> dP^{l + 1}', 'adjoint', N * C * (v[2] + v[l + 1]) * es, (g[2], g[l + 1], C, False)))
        out.append((f'adjoint: dP^{l} -> dP^{l + 1} (accumulate)', 'adjoint', N * C * (v[l] + 2 * v[l + 1]) * es, (g[l], g[l + 1], C, True)))
    for l in range(B, 2, -1):
        out.append((f'resize: P^{l} into V', 'resize', N * C * (v[l] + v[2]) * es, (g[l], g[2], C, False)))
    out.append(('pool backward: dX^B', 'pool_bwd', N * Cb * (2 * v[B] + bins) * es, (g[B], Cb)))
    return out


def print_bounds():
    for dim, N, sp, _ in SHAPES:
        rows = launches(dim, N, sp)
        print(f'memory bounds at {dim}-D {N} x {sp}, C = 256, L = 4 (16-bit): {sum(r[2] for r in rows) / 1e6:.1f} MB in {len(rows)} launches')
        for name, _, b, _ in rows:
            print(f'  {name:50s} {b / 1e6:9.2f} MB {b / HBM * 1e6:8.2f} us')


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

    def model(arch, dim, **kw):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            return UNet(architecture=arch, dim=dim, pretrained=False, **kw).cuda()

    torch.manual_seed(0)
    for dim, N, sp, act in SHAPES:
        X = torch.rand((N, 1) + sp, device='cuda')
        lab = X[:, 0] > 0.5
        y = torch.stack([~lab, lab], 1).half()
        w = torch.ones_like(y)
        t = {}
        for arch in ('U-Net', 'UPerNet'):
            m = model(arch, dim, act_dtype=act)
            te = m.train_engine()
            te.use_handle = False
            t[arch] = timed(lambda: te.train_step(X, y, w, sync=False))
            del te, m
            torch.cuda.empty_cache()
        print(f'train step {dim}-D {N} x {sp} {act}: U-Net {t["U-Net"]:9.2f} ms   UPerNet {t["UPerNet"]:9.2f} ms   '
              f'UPerNet / U-Net {t["UPerNet"] / t["U-Net"]:.3f}')
        T = torch.float16 if act == 'fp16' else torch.bfloat16
        code = nv.DTYPE_CODE[T]
        buf = lambda c, g: torch.randn(N * c * math.prod(g), device='cuda').to(T)
        total_t = total_b = 0.0
        for name, kind, nbytes, args in launches(dim, N, sp):
            s = nv.stream()
            if kind in ('resize', 'resize_base'):
                gs, gt, c, pro = args
                src, dst = buf(c, gs), buf(c, gt)
                sc = torch.ones(c, device='cuda') if pro else None
                base = buf(c, gt) if kind == 'resize_base' else None
                bsc = torch.ones(c, device='cuda') if base is not None else None
                fn = lambda: nv.call('iunet_pn_resize', code, dim, nv.ptr(src), c * math.prod(gs), *gs, nv.ptr(sc), nv.ptr(sc), nv.ptr(base),
                                     c * math.prod(gt), nv.ptr(bsc), nv.ptr(bsc), nv.ptr(dst), c * math.prod(gt), *gt, c, N, s)
            elif kind == 'adjoint':
                gt, gs, c, acc = args
                u, dx = buf(c, gt), buf(c, gs)
                fn = lambda: nv.call('iunet_pn_resize_adjoint', code, dim, nv.ptr(u), c * math.prod(gt), *gt, nv.ptr(dx), c * math.prod(gs), *gs, c, N,
                                     int(acc), s)
            else:
                g, c = args
                x, dx = buf(c, g), buf(c, g)
                a = [buf(c, (q,) * dim) for q in SIZES]
                tabs = nv.ptr_array(a), nv.ll_array([c * q ** dim for q in SIZES])
                if kind == 'pool':
                    fn = lambda: nv.call('iunet_pn_pool', code, dim, nv.ptr(x), c * math.prod(g), *g, *tabs, c, N, s)
                else:
                    fn = lambda: nv.call('iunet_pn_pool_bwd', code, dim, nv.ptr(x), c * math.prod(g), *tabs, nv.ptr(dx), c * math.prod(g), *g, c, N, s)
            us = timed(fn, n=50, warm=5) * 1e3
            total_t, total_b = total_t + us, total_b + nbytes
            print(f'  {name:50s} {nbytes / 1e6:9.2f} MB  bound {nbytes / HBM * 1e6:7.2f} us  call {us:8.2f} us  bound / call {100 * nbytes / HBM * 1e6 / us:5.1f} %')
        print(f'  the new kernels together: {total_t:.1f} us per step ({100 * total_t / 1e3 / t["UPerNet"]:.1f} % of the UPerNet step), '
              f'{total_b / HBM * 1e6:.1f} us at the memory bound')


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == 'bounds':
        print_bounds()
    else:
        main()
