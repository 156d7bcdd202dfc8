"""Time the connected-component labelling at the size the app would use: a 512^3 volume.
  * inputs, generated on the device from a fixed seed: a class map from thresholded smoothed noise (blobs: long runs along x, few seams),
    the 2-class predicted volume of the same field, and the class map as random p = 0.5 noise (the many-seams worst case);
  * iunet_cc_label (its six launches together), iunet_cc_table and iunet_cc_filter, each against its byte bound over 5 TB/s, the copy
    rate the other sections use: per voxel, tile pass C read + 4 written (+ 1 for cls, + 1 for the key map at C >= 2), seam pass 1 read,
    flatten 4 + 4, rank 4, apply 4 + 4; table 4; filter 4 + 1 + 1;
  * label + table + remove_small end to end through interactive_unet/components.py (remove_small labels again: two labellings);
  * scipy.ndimage.label of the same class map on the host, timed once.
HIP events around `--iters` back-to-back calls after warm-up, `--reps` times: median and spread.  The entry point's launches are not
separated by events; a kernel trace of `--once` (one warm and one measured call of each entry point, no events) gives the time per pass.
   python tools/bench_components.py [--volume 512] [--iters 3] [--reps 7] [--once] [--no-host]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'interactive-unet_amd')); sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F
from interactive_unet import components, _native as nv

HBM = 5e12        # bytes / s: the figure DESIGN.md uses for HBM passes


def timed(fn, iters, reps, warm=2):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters): fn()
        e1.record(); torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / iters * 1e3)
    return us


def fmt(us):
    return f'{np.median(us):.0f} us (min {min(us):.0f}, max {max(us):.0f})'


def smooth_field(V, g):
    """Uniform noise smoothed by three box filters of 9 voxels, rescaled to [0, 1]: blobs of some tens of voxels."""
    f = torch.rand((1, 1, V, V, V), device='cuda', generator=g)
    for _ in range(3):
        f = F.avg_pool3d(f, 9, stride=1, padding=4, count_include_pad=False)
    f = f[0, 0]
    lo, hi = f.min(), f.max()
    return (f - lo) / (hi - lo)


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
    del f, q
    print(f'volume {V}^3 = {vox / 1e6:.1f} M voxels; HIP events, median of {a.reps} x {a.iters} back-to-back calls')
    labels = torch.empty((V, V, V), dtype=torch.int32, device='cuda')
    cls = torch.empty((V, V, V), dtype=torch.uint8, device='cuda')
    out = torch.empty((V, V, V), dtype=torch.uint8, device='cuda')
    count = torch.empty(1, dtype=torch.int32, device='cuda')
    need = nv.lib().iunet_cc_ws_bytes(V, V, V)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    for name, src, bg in (('blobs, class map', blobs, 0), ('blobs, predicted volume x 2', pred, 0), ('noise p = 0.5, class map', noise, 0)):
        C = 1 if src.ndim == 3 else src.shape[3]
        for conn in (6, 26):
            lab = lambda: nv.call('iunet_cc_label', nv.ptr(src), V, V, V, C, conn, bg, nv.ptr(labels), nv.ptr(cls), nv.ptr(count), nv.ptr(ws), need,
                                  nv.stream())
            lab()
            K = int(count.item())
            sizes = torch.empty(K + 1, dtype=torch.int32, device='cuda'); classes = torch.empty(K + 1, dtype=torch.uint8, device='cuda')
            first = torch.empty(K + 1, dtype=torch.int32, device='cuda')
            tab = lambda: nv.call('iunet_cc_table', nv.ptr(labels), nv.ptr(cls), V, V, V, K, nv.ptr(sizes), nv.ptr(classes), nv.ptr(first), nv.stream())
            tab()
            keep = (sizes >= 64).to(torch.uint8)
            fil = lambda: nv.call('iunet_cc_filter', nv.ptr(labels), nv.ptr(cls), V, V, V, K, nv.ptr(keep), 0, nv.ptr(out), nv.stream())
            passes = {'tile': C + 4 + 1 + (C > 1), 'seam': 1, 'flatten': 8, 'rank': 4, 'apply': 8}
            print(f'{name}, connectivity {conn}: K = {K}, largest {int(sizes.max())} voxels, {int((labels > 0).sum()) / vox * 100:.0f} % foreground')
            if a.once:
                lab(); tab(); fil(); torch.cuda.synchronize()
                continue
            for what, fn, per in (('label (6 launches)', lab, sum(passes.values())), ('table (3 launches)', tab, 4), ('filter', fil, 6)):
                us = timed(fn, a.iters, a.reps)
                bound = vox * per / HBM * 1e6
                print(f'  {what}: {fmt(us)}; byte bound {bound:.0f} us = {per} bytes per voxel / 5 TB/s -> {100 * bound / np.median(us):.0f} % of it')
            print('  label\'s bound by pass, bytes per voxel: ' + ', '.join(f'{k} {v}' for k, v in passes.items()))
    if a.once:
        return

    def end_to_end():
        l, K, c = components.label(blobs)
        components.table(l, c, K)
        components.remove_small(blobs, 64)
    ms = [t / 1e3 for t in timed(end_to_end, 1, a.reps, warm=1)]
    print(f'label + table + remove_small end to end (blobs, class map, connectivity 6; allocations and the two count reads included): '
          f'{np.median(ms):.2f} ms (min {min(ms):.2f}, max {max(ms):.2f})')
    if not a.no_host:
        from scipy import ndimage
        host = blobs.cpu().numpy()
        t0 = time.time()
        _, k = ndimage.label(host)
        print(f'scipy.ndimage.label of the same class map on the host (one core, once): {time.time() - t0:.1f} s, K = {k}')


if __name__ == '__main__':
    main()
