"""Time the exact distance transform and the ball morphology built on it at the size the app would use: a 512^3 volume.
  * inputs, generated on the device from a fixed seed: the blob class map of bench_components.smooth_field, its 2-class predicted volume,
    the class map as random p = 0.5 noise, and a single seed in one corner (every distance is long);
  * iunet_edt_sq, iunet_edt_sq_mask and iunet_edt_select, each against its byte bound over 5 TB/s, the copy rate the other sections
    use.  Per voxel: pass X reads C bytes (4 for the distance map iunet_edt_sq_mask thresholds) and writes 4, + 1 for cls; passes Y and Z
    read 4 and write 4 in place, plus the stack of Meijster's envelope in the workspace -- at most one push (2 + 2 + 4 bytes written) per
    entry, and one entry read back (8 bytes) per pop and per parabola left at the end: between 0 and 16 bytes per voxel and pass, which
    depends on the data and is not part of the bound (the bound is what any method must move: 4 + 4); select reads 4 + 1 and writes 1;
  * opening, closing and fill_holes end to end through interactive_unet/morphology.py (allocations included);
  * scipy.ndimage.distance_transform_edt and binary_opening of the blob class map on the host, timed once.
HIP events around `--iters` back-to-back calls after warm-up, `--reps` times: median and spread.  The entry points' launches are not
separated by events; a kernel trace of `--once` (one warm and one measured call of each entry point, no events) gives the time per pass.
   python tools/bench_morphology.py [--volume 512] [--iters 3] [--reps 7] [--once] [--no-host]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'interactive-unet_amd')); sys.path.insert(0, ROOT)
import numpy as np
import torch
from interactive_unet import morphology, _native as nv
from tools.bench_components import HBM, fmt, smooth_field, timed


def pass_bytes(Z, Y, X, C, with_cls):
    """The byte bound of each pass, from the shapes: {pass: bytes}.  An axis of one entry has no column pass."""
    vox = Z * Y * X
    out = {'X': vox * (C + 4 + (1 if with_cls else 0))}
    if Y > 1: out['Y'] = vox * 8
    if Z > 1: out['Z'] = vox * 8
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--volume', type=int, default=512); ap.add_argument('--iters', type=int, default=3); ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--once', action='store_true'); ap.add_argument('--no-host', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'the measurement needs the GPU'
    V = a.volume
    vox = V ** 3
    g = torch.Generator(device='cuda').manual_seed(0)
    f = smooth_field(V, g)
    q = (f.clamp(0, 1) * 255).round().to(torch.uint8)
    blobs = (f > f.median()).to(torch.uint8)
    pred = torch.stack([255 - q, q], dim=-1).contiguous()
    noise = (torch.rand((V, V, V), device='cuda', generator=g) < 0.5).to(torch.uint8)
    corner = torch.zeros((V, V, V), dtype=torch.uint8, device='cuda')
    corner[0, 0, 0] = 1
    del f, q
    print(f'volume {V}^3 = {vox / 1e6:.1f} M voxels; HIP events, median of {a.reps} x {a.iters} back-to-back calls')
    d2 = torch.empty((V, V, V), dtype=torch.int32, device='cuda')
    d3 = torch.empty((V, V, V), dtype=torch.int32, device='cuda')
    cls = torch.empty((V, V, V), dtype=torch.uint8, device='cuda')
    out = torch.empty((V, V, V), dtype=torch.uint8, device='cuda')
    need = nv.lib().iunet_edt_ws_bytes(V, V, V)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    print(f'workspace {need / 2 ** 20:.0f} MiB (8 bytes per voxel) + d2 {4 * vox / 2 ** 20:.0f} MiB; one transform holds '
          f'{(need + 5 * vox) / 2 ** 20:.0f} MiB beside its source, an opening or closing {(need + 9 * vox) / 2 ** 20:.0f} MiB')
    r2 = 9
    for name, src, invert in (('blobs, class map', blobs, 1), ('blobs, predicted volume x 2', pred, 1), ('noise p = 0.5, class map', noise, 0),
                              ('one seed in a corner, class map', corner, 0)):
        C = 1 if src.ndim == 3 else src.shape[3]
        edt = lambda: nv.call('iunet_edt_sq', nv.ptr(src), V, V, V, C, 1, invert, nv.ptr(d2), nv.ptr(cls), nv.ptr(ws), need, nv.stream())
        msk = lambda: nv.call('iunet_edt_sq_mask', nv.ptr(d2), V, V, V, r2, 1, nv.ptr(d3), nv.ptr(ws), need, nv.stream())
        sel = lambda: nv.call('iunet_edt_select', nv.ptr(d3), nv.ptr(cls), V, V, V, r2, 1, 1, 0, nv.ptr(out), nv.stream())
        edt(); msk(); sel()
        finite = d2[d2 < morphology.INF]
        print(f'{name} (invert {invert}): largest squared distance {int(finite.max())}, {int((d2 == 0).sum()) / vox * 100:.0f} % seeds; '
              f'after the threshold at r2 = {r2}: {int((d3 == 0).sum()) / vox * 100:.0f} % seeds')
        del finite
        if a.once:
            edt(); msk(); sel(); torch.cuda.synchronize()
            continue
        pe, pm = pass_bytes(V, V, V, C, True), pass_bytes(V, V, V, 4, False)
        for what, fn, per in (('edt_sq (3 launches)', edt, sum(pe.values())), ('edt_sq_mask (3 launches)', msk, sum(pm.values())),
                              ('edt_select', sel, vox * 6)):
            us = timed(fn, a.iters, a.reps)
            bound = per / HBM * 1e6
            print(f'  {what}: {fmt(us)}; byte bound {bound:.0f} us = {per / vox:.0f} bytes per voxel / 5 TB/s -> {100 * bound / np.median(us):.0f} % of it')
        print('  edt_sq\'s bound by pass, us: ' + ', '.join(f'{k} {v / HBM * 1e6:.0f}' for k, v in pe.items()) +
              '; edt_sq_mask\'s: ' + ', '.join(f'{k} {v / HBM * 1e6:.0f}' for k, v in pm.items()) +
              '; the stacks add 0 .. 16 bytes per voxel to Y and Z, by the data')
    if a.once:
        return
    del d2, d3, cls, out, ws
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    for what, fn in (('opening(blobs, 1, 3)', lambda: morphology.opening(blobs, 1, 3)), ('closing(blobs, 1, 3)', lambda: morphology.closing(blobs, 1, 3)),
                     ('closing(predicted volume, 1, 3)', lambda: morphology.closing(pred, 1, 3)),
                     ('fill_holes(blobs, 1)', lambda: morphology.fill_holes(blobs, 1))):
        ms = [t / 1e3 for t in timed(fn, 1, a.reps, warm=1)]
        print(f'{what} end to end (allocations included): {np.median(ms):.2f} ms (min {min(ms):.2f}, max {max(ms):.2f}); '
              f'peak memory above the inputs {(torch.cuda.max_memory_allocated() - base) / 2 ** 20:.0f} MiB')
        torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    if not a.no_host:
        from scipy import ndimage
        host = blobs.cpu().numpy().astype(bool)
        t0 = time.time()
        ndimage.distance_transform_edt(host)
        t1 = time.time()
        g3 = np.arange(-3, 4)
        ball = (g3[:, None, None] ** 2 + g3[None, :, None] ** 2 + g3[None, None, :] ** 2) <= 9
        ndimage.binary_opening(host, ball)
        print(f'scipy.ndimage on the host (one core, once), the blob class map: distance_transform_edt {t1 - t0:.1f} s, '
              f'binary_opening by the ball of radius 3 {time.time() - t1:.1f} s')


if __name__ == '__main__':
    main()
