"""Time the geodesic seeded growth and the instance split built on it at the size the app would use: a 512^3 volume,
the blob class map of tools/bench_morphology.py, its cores of the erosion by 3 (labelled, connectivity 6) as the seeds.
  * iunet_geo_init and iunet_geo_finish against their byte bounds over 5 TB/s, the copy rate the other sections use: init reads src and
    seeds and writes the keys, 13 bytes per voxel; finish reads the keys (and fallback) and writes labels (and g), 12 to 20 bytes per voxel;
  * iunet_geo_relax one round per call, each between two HIP events, until no tile changes: the rounds to rest, the time of the first round
    (every tile active), of every later round beside the tiles it changed, and of all rounds; for the face-step metric the split uses under
    connectivity 6, (3, 0, 0), and for the full chamfer metric (3, 4, 5);
  * geodesic.split_touching(blobs, 1, 3) end to end (allocations and read-backs included) beside instances.split_touching(blobs, 1, 3), the
    yardstick, in the same run on the same input, each with its peak memory.
Nothing here is gated.
   python tools/bench_geodesic.py [--volume 512] [--iters 3] [--reps 7]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'interactive-unet_amd')); sys.path.insert(0, ROOT)
import numpy as np
import torch
from interactive_unet import geodesic, instances, morphology, _native as nv
from tools.bench_components import HBM, fmt, smooth_field, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--volume', type=int, default=512); ap.add_argument('--iters', type=int, default=3); ap.add_argument('--reps', type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'the measurement needs the GPU'
    V = a.volume
    vox = V ** 3
    g = torch.Generator(device='cuda').manual_seed(0)
    f = smooth_field(V, g)
    blobs = (f > f.median()).to(torch.uint8)
    del f
    print(f'volume {V}^3 = {vox / 1e6:.1f} M voxels; HIP events, median of {a.reps} x {a.iters} back-to-back calls')
    r2 = 9
    d_out = morphology._edt(blobs, V, V, V, 1, 1, True, want_cls=False)[0]
    le, ke = instances._label((d_out > r2).to(torch.uint8), V, V, V, 6)
    la, ka = instances._label(blobs, V, V, V, 6)
    del d_out
    print(f'blobs eroded by 3: {ke} cores in {ka} objects')
    need = nv.lib().iunet_geo_ws_bytes(V, V, V)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    labels, dist = torch.empty((V, V, V), dtype=torch.int32, device='cuda'), torch.empty((V, V, V), dtype=torch.int32, device='cuda')
    changed = torch.empty(1, dtype=torch.int32, device='cuda')
    print(f'workspace {need / 2 ** 20:.0f} MiB (8 bytes per voxel and two flags per tile of 8 x 8 x 64)')
    init = lambda: nv.call('iunet_geo_init', nv.ptr(blobs), V, V, V, 1, 1, nv.ptr(le), nv.ptr(ws), need, nv.stream())
    us = timed(init, a.iters, a.reps)
    bound = 13 * vox / HBM * 1e6
    print(f'  geo_init: {fmt(us)}; byte bound {bound:.0f} us = 13 bytes per voxel / 5 TB/s -> {100 * bound / np.median(us):.0f} % of it')
    for weights in ((3, 0, 0), (3, 4, 5)):
        init()
        rounds = []
        while True:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            nv.call('iunet_geo_relax', nv.ptr(ws), need, V, V, V, *weights, 1, nv.ptr(changed), nv.stream())
            e1.record(); torch.cuda.synchronize()
            rounds.append((e0.elapsed_time(e1) * 1e3, int(changed.item())))
            if rounds[-1][1] == 0:
                break
        t = [r[0] for r in rounds]
        print(f'  geo_relax {weights}: {len(t)} rounds to rest (the last finds nothing to do); first round, every tile active: {t[0]:.0f} us; all rounds '
              f'{sum(t) / 1e3:.2f} ms; per round (us, tiles that changed): {[(round(r[0]), r[1]) for r in rounds]}')
    for what, fb, gd, per in (('labels', None, None, 12), ('labels and g', None, dist, 16), ('labels with fallback', la, None, 16), ('labels and g with fallback', la, dist, 20)):
        fin = lambda: nv.call('iunet_geo_finish', nv.ptr(ws), need, V, V, V, nv.ptr(labels), nv.ptr(gd), nv.ptr(fb), ke, nv.stream())
        us = timed(fin, a.iters, a.reps)
        bound = per * vox / HBM * 1e6
        print(f'  geo_finish, {what}: {fmt(us)}; byte bound {bound:.0f} us = {per} bytes per voxel / 5 TB/s -> {100 * bound / np.median(us):.0f} % of it')
    del ws, labels, dist, le, la
    for name, fn in (('geodesic.split_touching', geodesic.split_touching), ('instances.split_touching', instances.split_touching)):
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out, count = fn(blobs, 1, 3)
        sizes = torch.bincount(out.reshape(-1))[1:]
        del out
        ms = [t / 1e3 for t in timed(lambda: fn(blobs, 1, 3), 1, a.reps, warm=1)]
        print(f'{name}(blobs, 1, 3) end to end (allocations and read-backs included): {count} instances, the largest {int(sizes.max())} voxels; '
              f'{np.median(ms):.2f} ms (min {min(ms):.2f}, max {max(ms):.2f}); peak memory above the inputs '
              f'{(torch.cuda.max_memory_allocated() - base) / 2 ** 20:.0f} MiB')


if __name__ == '__main__':
    main()
