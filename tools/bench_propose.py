"""Time the slice proposal's two kernels at the size the app would use: a 512^3 predicted volume of 2 classes.
  * iunet_uncertainty_volume (u and the brick sums at brick 8; the other brick sizes without weight and image), with and without the
    weight (2 channels) and image (1 channel) volumes, against its byte bound: (C + wch + ich bytes read + 1 written) per voxel
    over 5 TB/s, the copy rate the other sections use;
  * iunet_plane_scores of 256 planes of 256^2 samples on that u -- random orientations through the 32 most uncertain bricks, as
    propose_slices builds them -- and the same number of axis-aligned planes with rows along x;
  * propose.propose_slices end to end (uncertainty, candidate sort, 256 planes built on the host, one scoring launch, ranking).
HIP events around `--iters` back-to-back calls after warm-up, `--reps` times: median and spread.
   python tools/bench_propose.py [--volume 512] [--classes 2] [--width 256] [--planes 256]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'interactive-unet_amd')); sys.path.insert(0, ROOT)
import numpy as np
import torch
from interactive_unet import propose, _native as nv
from interactive_unet.slicer import Slicer

HBM = 5e12        # bytes / s: the figure DESIGN.md uses for HBM passes


def timed(fn, iters, reps, warm=10):
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
    return f'{np.median(us):.1f} us (min {min(us):.1f}, max {max(us):.1f})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--volume', type=int, default=512); ap.add_argument('--classes', type=int, default=2)
    ap.add_argument('--width', type=int, default=256); ap.add_argument('--planes', type=int, default=256)
    ap.add_argument('--iters', type=int, default=20); ap.add_argument('--reps', type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'the measurement needs the GPU'
    V, C, S, P = a.volume, a.classes, a.width, a.planes
    vox = V ** 3
    g = torch.Generator(device='cuda').manual_seed(0)
    # a prediction-like volume: p in [1/2, 1) for the first class, the rest shared out; a quarter of the voxels annotated, a tenth dark
    pred = torch.zeros((V, V, V, C), dtype=torch.uint8, device='cuda')
    pred[..., 0] = torch.randint(128, 256, (V, V, V), dtype=torch.uint8, device='cuda', generator=g)
    pred[..., 1] = 255 - pred[..., 0]
    weight = torch.zeros((V, V, V, 2), dtype=torch.uint8, device='cuda')
    weight[..., 0] = (torch.rand((V, V, V), device='cuda', generator=g) < 0.25).to(torch.uint8) * 255
    image = torch.randint(0, 10, (V, V, V), dtype=torch.uint8, device='cuda', generator=g).clamp_(max=1) * 200
    print(f'predicted volume {V}^3 x {C}; HIP events, median of {a.reps} x {a.iters} back-to-back calls')

    def unc(w, im, brick, u, bricks):
        nv.call('iunet_uncertainty_volume', nv.ptr(pred), V, V, V, C, nv.ptr(w), 0 if w is None else 2, nv.ptr(im), 0 if im is None else 1, brick,
                nv.ptr(u), nv.ptr(bricks), nv.stream())
    u = torch.empty((V, V, V), dtype=torch.uint8, device='cuda')
    for name, w, im in (('pred alone', None, None), ('pred + weight (2 ch) + image (1 ch)', weight, image)):
        per = C + (0 if w is None else 2) + (0 if im is None else 1) + 1
        bound = vox * per / HBM * 1e6
        for brick in (8,) if w is not None else (8, 4, 16, 32):
            bricks = torch.empty([-(-V // brick)] * 3, dtype=torch.int32, device='cuda')
            us = timed(lambda: unc(w, im, brick, u, bricks), a.iters, a.reps)
            print(f'uncertainty, {name}, brick {brick}: {fmt(us)}; byte bound {bound:.1f} us = {vox / 1e6:.1f} M voxels x {per} bytes / 5 TB/s '
                  f'-> {100 * bound / np.median(us):.0f} % of it ({vox * per / np.median(us) / 1e6:.2f} TB/s)')
        bricks = torch.empty([-(-V // 8)] * 3, dtype=torch.int32, device='cuda')
        us = timed(lambda: unc(w, im, 8, None, bricks), a.iters, a.reps)
        print(f'uncertainty, {name}, brick sums only: {fmt(us)}; byte bound {vox * (per - 1) / HBM * 1e6:.1f} us -> '
              f'{100 * vox * (per - 1) / HBM * 1e6 / np.median(us):.0f} % of it')
    u, bricks = propose.uncertainty(pred, weight, image, brick=8)
    origins = propose.candidate_origins(bricks, 8, (V, V, V), 32)
    s = Slicer([V, V, V])
    gen = torch.Generator().manual_seed(0)
    planes = []
    for k in range(P):
        v = torch.randn(3, dtype=torch.float64, generator=gen).numpy()
        s.update_orientation_vectors(v / np.linalg.norm(v))
        planes.append((s.v, s.w, origins[k % len(origins)]))
    aligned = [(np.eye(3)[1], np.eye(3)[2], o) for _, _, o in planes]
    for name, pl in (('random orientations', np.array(planes)), ('axis-aligned, rows along x', np.array(aligned))):
        got = propose.score_planes(u, pl, S).cpu().numpy()
        geoms = torch.from_numpy(np.ascontiguousarray(pl.reshape(-1, 9))).cuda()
        need = nv.lib().iunet_plane_scores_ws_bytes(P, S)
        ws = torch.empty(need, dtype=torch.uint8, device='cuda')
        out = torch.empty((P, 2), dtype=torch.int64, device='cuda')
        us = timed(lambda: nv.call('iunet_plane_scores', nv.ptr(u), V, V, V, nv.ptr(geoms), P, S, -(S // 2), nv.ptr(ws), need, nv.ptr(out),
                                   nv.stream()), a.iters, a.reps)
        inside = int(got[:, 1].sum())
        print(f'plane scores, {P} planes of {S}^2, {name}: {fmt(us)} for both launches; {inside / 1e6:.1f} M of {P * S * S / 1e6:.1f} M samples '
              f'inside = {inside / 1e6:.1f} MB of gathered bytes -> {inside / np.median(us) / 1e3:.1f} G samples/s')
    ms = [t / 1e3 for t in timed(lambda: propose.propose_slices((V, V, V), pred, weight=weight, image=image, slice_width=S, candidates=32,
                                                                 orientations=max(1, P // 32), generator=gen), 3, a.reps, warm=2)]
    print(f'propose_slices end to end (32 candidates x {max(1, P // 32)} orientations): {np.median(ms):.2f} ms (min {min(ms):.2f}, max {max(ms):.2f})')


if __name__ == '__main__':
    main()
