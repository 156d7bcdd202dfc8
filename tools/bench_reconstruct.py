"""Time the grayscale reconstruction and the h-maxima split built on it at the size the app would use: a 512^3 volume,
the blob class map of tools/bench_morphology.py, its distance landscape at scale 4.
  * the streaming passes against their byte bounds over 5 TB/s, the copy rate the other sections use: iunet_rec_landscape in place (4 bytes
    read and 4 written per voxel), iunet_rec_init with marker = mask (4 read, 4 written) and with a marker of its own (8 read, 4 written),
    iunet_rec_select (8 read, 1 written);
  * iunet_rec_relax one round per call, each between two HIP events, until no tile changes: the rounds to rest, the time of every round
    beside the tiles it changed, and of all rounds; for hmaxima at h = 1 voxel (connectivity 6) and for the regional-maxima reconstruction
    of its result that follows it in extended_maxima;
  * reconstruction.split_touching(blobs, 1, 1.0) end to end (allocations and read-backs included) beside geodesic.split_touching(blobs, 1, 3),
    the yardstick, in the same run on the same input, each with its instance count and peak memory.
Nothing here is gated.
   python tools/bench_reconstruct.py [--volume 512] [--iters 3] [--reps 7]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'interactive-unet_amd')); sys.path.insert(0, ROOT)
import numpy as np
import torch
from interactive_unet import geodesic, morphology, reconstruction, _native as nv
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
    scale, conn = 4, 6
    d_out = morphology._edt(blobs, V, V, V, 1, 1, True, want_cls=False)[0]
    land = torch.empty_like(d_out)

    def report(what, us, per):
        bound = per * vox / HBM * 1e6
        print(f'  {what}: {fmt(us)}; byte bound {bound:.0f} us = {per} bytes per voxel / 5 TB/s -> {100 * bound / np.median(us):.0f} % of it')

    report('rec_landscape out of place', timed(lambda: nv.call('iunet_rec_landscape', nv.ptr(d_out), V, V, V, scale, reconstruction.OFF, nv.ptr(land), nv.stream()),
                                                a.iters, a.reps), 8)
    scratch = d_out                                                    # in place on its own output again and again: other values, the same bytes
    report('rec_landscape in place', timed(lambda: nv.call('iunet_rec_landscape', nv.ptr(scratch), V, V, V, scale, reconstruction.OFF, nv.ptr(scratch), nv.stream()),
                                            a.iters, a.reps), 8)
    del d_out, scratch
    print(f'landscape at scale {scale}: highest peak {int(land.max())}, {int((land > reconstruction.OFF).sum()) / vox * 100:.0f} % on the class')
    need = nv.lib().iunet_rec_ws_bytes(V, V, V)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    r, r2 = torch.empty_like(land), torch.empty_like(land)
    out = torch.empty((V, V, V), dtype=torch.uint8, device='cuda')
    changed = torch.empty(1, dtype=torch.int32, device='cuda')
    print(f'workspace {need / 2 ** 10:.0f} KiB (two flags per tile of 8 x 8 x 64); the state is r itself, 4 bytes per voxel')
    init = lambda marker, mask, dst, h: nv.call('iunet_rec_init', nv.ptr(marker), nv.ptr(mask), V, V, V, h, 0, nv.ptr(dst), nv.ptr(ws), need, nv.stream())
    report('rec_init, marker = mask', timed(lambda: init(land, land, r, scale), a.iters, a.reps), 8)

    def rounds_of(dst, mask, what):
        rounds = []
        while True:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            nv.call('iunet_rec_relax', nv.ptr(dst), nv.ptr(mask), V, V, V, conn, 0, 1, nv.ptr(changed), nv.ptr(ws), need, nv.stream())
            e1.record(); torch.cuda.synchronize()
            rounds.append((e0.elapsed_time(e1) * 1e3, int(changed.item())))
            if rounds[-1][1] == 0:
                break
        t = [x[0] for x in rounds]
        print(f'  rec_relax, {what}: {len(t)} rounds to rest (the last finds nothing to do); all rounds {sum(t) / 1e3:.2f} ms; per round (us, tiles that '
              f'changed of {need // 8}): {[(round(x[0]), x[1]) for x in rounds]}')

    init(land, land, r, scale)                                         # hmaxima at h = 1 voxel
    rounds_of(r, land, f'hmaxima at h = {scale} (1 voxel), connectivity {conn}')
    report('rec_init, a marker of its own', timed(lambda: init(land, r, r2, 1), a.iters, a.reps), 12)
    init(r, r, r2, 1)                                                  # the regional maxima of the result
    rounds_of(r2, r, 'the regional-maxima reconstruction (h = 1) of that result')
    report('rec_select', timed(lambda: nv.call('iunet_rec_select', nv.ptr(r), nv.ptr(r2), V, V, V, 1, 1, nv.ptr(out), nv.stream()), a.iters, a.reps), 9)
    print(f'extended maxima: {int(out.sum())} voxels')
    del ws, r, r2, out, land
    for name, fn, arg in (('reconstruction.split_touching(blobs, 1, 1.0)', reconstruction.split_touching, 1.0),
                          ('geodesic.split_touching(blobs, 1, 3)', geodesic.split_touching, 3)):
        torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        labels, count = fn(blobs, 1, arg)
        sizes = torch.bincount(labels.reshape(-1))[1:]
        del labels
        ms = [t / 1e3 for t in timed(lambda: fn(blobs, 1, arg), 1, a.reps, warm=1)]
        print(f'{name} end to end (allocations and read-backs included): {count} instances, the largest {int(sizes.max())} voxels, the smallest '
              f'{int(sizes.min())}; {np.median(ms):.2f} ms (min {min(ms):.2f}, max {max(ms):.2f}); peak memory above the inputs '
              f'{(torch.cuda.max_memory_allocated() - base) / 2 ** 20:.0f} MiB')


if __name__ == '__main__':
    main()
