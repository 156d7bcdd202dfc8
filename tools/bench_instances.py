"""Time the nearest-seed feature transform and the instance splitting built on it at the size the app would use: a
512^3 volume, on the four inputs of tools/bench_morphology.py (the blob class map, its 2-class predicted volume, p = 0.5 noise, one seed in
a corner).
  * iunet_edt_feature beside iunet_edt_sq, measured in the same run on the same input: the plain transform is the yardstick.  Per voxel the
    feature transform moves, beyond the plain one's bytes: pass X writes 4 more (idx); passes Y and Z each write 4 more, and read the
    governing site's idx from the pass before once per parabola of the column's envelope (at most 4 per voxel; it depends on the data);
  * iunet_edt_assign (with and without a group map) and iunet_label_remap against their byte bounds over 5 TB/s, the copy rate the other
    sections use: assign reads idx and d2 (and group) and writes out, 12 (16) bytes per voxel, its gathers through idx not counted; remap
    reads and writes the labels, 8 bytes per voxel;
  * split_touching(blobs, 1, 3) end to end through interactive_unet/instances.py (allocations included) with its peak memory;
  * the host figure for the same volume: scipy.ndimage.distance_transform_edt with indices and ndimage.label, one core, once.
HIP events around `--iters` back-to-back calls after warm-up, `--reps` times: median and spread.  A kernel trace of `--once` (one warm and
one measured call of each entry point, no events) gives the time per pass.
   python tools/bench_instances.py [--volume 512] [--iters 3] [--reps 7] [--once] [--no-host]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'interactive-unet_amd')); sys.path.insert(0, ROOT)
import numpy as np
import torch
from interactive_unet import instances, morphology, _native as nv
from tools.bench_components import HBM, fmt, smooth_field, timed


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
    idx = torch.empty_like(d2)
    plain = torch.empty_like(d2)
    out = torch.empty_like(d2)
    cls = torch.empty((V, V, V), dtype=torch.uint8, device='cuda')
    need = nv.lib().iunet_edt_feature_ws_bytes(V, V, V)
    need_plain = nv.lib().iunet_edt_ws_bytes(V, V, V)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    print(f'workspace {need / 2 ** 20:.0f} MiB (12 bytes per voxel; the plain transform\'s {need_plain / 2 ** 20:.0f} MiB) + d2 and idx '
          f'{8 * vox / 2 ** 20:.0f} MiB')
    for name, src, invert in (('blobs, class map', blobs, 1), ('blobs, predicted volume x 2', pred, 1), ('noise p = 0.5, class map', noise, 0),
                              ('one seed in a corner, class map', corner, 0)):
        C = 1 if src.ndim == 3 else src.shape[3]
        sq = lambda: nv.call('iunet_edt_sq', nv.ptr(src), V, V, V, C, 1, invert, nv.ptr(plain), nv.ptr(cls), nv.ptr(ws), need_plain, nv.stream())
        feat = lambda: nv.call('iunet_edt_feature', nv.ptr(src), V, V, V, C, 1, invert, nv.ptr(d2), nv.ptr(idx), nv.ptr(cls), nv.ptr(ws), need, nv.stream())
        sq(); feat()
        assert torch.equal(d2, plain)
        print(f'{name} (invert {invert}): {int((d2 == 0).sum()) / vox * 100:.0f} % seeds')
        if a.once:
            sq(); feat(); torch.cuda.synchronize()
            continue
        us_sq, us_feat = timed(sq, a.iters, a.reps), timed(feat, a.iters, a.reps)
        b_sq, b_feat = vox * (C + 5 + 16) / HBM * 1e6, vox * (C + 9 + 24) / HBM * 1e6
        print(f'  edt_sq (3 launches): {fmt(us_sq)}; byte bound {b_sq:.0f} us -> {100 * b_sq / np.median(us_sq):.0f} % of it')
        print(f'  edt_feature (3 launches): {fmt(us_feat)}; byte bound {b_feat:.0f} us ({C + 33} bytes per voxel, the reads through the site not '
              f'counted) -> {100 * b_feat / np.median(us_feat):.0f} % of it; {np.median(us_feat) / np.median(us_sq):.2f} x edt_sq, '
              f'+{np.median(us_feat) - np.median(us_sq):.0f} us for +{12 * vox / HBM * 1e6:.0f} us of bytes')
    # assign and remap on the blobs' maps: the cores of the erosion by 3, labelled; the objects as groups
    r2 = 9
    nv.call('iunet_edt_sq', nv.ptr(blobs), V, V, V, 1, 1, 1, nv.ptr(plain), None, nv.ptr(ws), need_plain, nv.stream())
    nv.call('iunet_edt_feature_mask', nv.ptr(plain), V, V, V, r2, 1, nv.ptr(d2), nv.ptr(idx), nv.ptr(ws), need, nv.stream())
    le, ke = instances._label((plain > r2).to(torch.uint8), V, V, V, 6)
    la, ka = instances._label(blobs, V, V, V, 6)
    print(f'blobs eroded by 3: {ke} cores in {ka} objects')
    table = torch.arange(ke + ka + 1, dtype=torch.int32, device='cuda')
    asg = lambda: nv.call('iunet_edt_assign', nv.ptr(idx), nv.ptr(d2), nv.ptr(le), None, 0, V, V, V, r2, nv.ptr(out), nv.stream())
    asg_g = lambda: nv.call('iunet_edt_assign', nv.ptr(idx), nv.ptr(d2), nv.ptr(le), nv.ptr(la), ke, V, V, V, morphology.MAX_SQ, nv.ptr(out), nv.stream())
    rmp = lambda: nv.call('iunet_label_remap', nv.ptr(out), V, V, V, ke + ka, nv.ptr(table), nv.stream())
    asg(); asg_g(); rmp()
    if a.once:
        asg(); asg_g(); rmp(); torch.cuda.synchronize()
        return
    for what, fn, per in (('edt_assign, no group, r2 = 9', asg, 12), ('edt_assign, groups, r2 = 2^31 - 2', asg_g, 16), ('label_remap (identity)', rmp, 8)):
        us = timed(fn, a.iters, a.reps)
        bound = per * vox / HBM * 1e6
        print(f'  {what}: {fmt(us)}; byte bound {bound:.0f} us = {per} bytes per voxel / 5 TB/s -> {100 * bound / np.median(us):.0f} % of it')
    del d2, idx, plain, out, cls, ws, le, la
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    labels, count = instances.split_touching(blobs, 1, 3)
    ms = [t / 1e3 for t in timed(lambda: instances.split_touching(blobs, 1, 3), 1, a.reps, warm=1)]
    print(f'split_touching(blobs, 1, 3) end to end (allocations and three 4-byte read-backs included): {count} instances; {np.median(ms):.2f} ms '
          f'(min {min(ms):.2f}, max {max(ms):.2f}); peak memory above the inputs {(torch.cuda.max_memory_allocated() - base) / 2 ** 20:.0f} MiB')
    if not a.no_host:
        from scipy import ndimage
        host = blobs.cpu().numpy().astype(bool)
        t0 = time.time()
        ndimage.distance_transform_edt(~host, return_indices=True)
        t1 = time.time()
        ndimage.label(host)
        print(f'scipy.ndimage on the host (one core, once), the blob class map: distance_transform_edt with indices {t1 - t0:.1f} s, '
              f'label {time.time() - t1:.1f} s')


if __name__ == '__main__':
    main()
