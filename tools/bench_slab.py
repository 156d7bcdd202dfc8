"""Time the oblique slab of the 3-D net's interactive prediction at the size the app would use: a T = 32,
S = 512 slab out of a 512^3 uint8 volume at a random orientation.
  * iunet_slab_gather at spline orders 0 and 1, against its byte bound: bytes written + one byte per gathered sample over 5 TB/s (at order
    1 a sample asks for 8 taps; neighbouring lanes share them and their cache lines, so the taps are what the launch asks for, not what
    reaches HBM);
  * iunet_slab_paste of the same slab's core (margin T / 4, border S / 4, the defaults of predict.update_predicted_volume) over its
    tight box, against (4 C bytes read + C bytes written per kept voxel) / 5 TB/s -- the box's other voxels only compute;
  * predict.predict_slab end to end (gather + forward, default prediction mode) against the whole-volume path's 3-D prediction of the
    same voxel count, four 128^3 blocks through predict.predict_blocks_3d (gather + forward + blend), in the same run.
HIP events around `--iters` back-to-back launches after warm-up, `--reps` times: median and spread.
   python tools/bench_slab.py [--depth 32] [--width 512] [--volume 512] [--classes 2]"""
import argparse, os, sys, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'interactive-unet_amd')); sys.path.insert(0, ROOT)
import numpy as np
import torch
from interactive_unet import predict, _native as nv
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
    ap.add_argument('--depth', type=int, default=32); ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--volume', type=int, default=512); ap.add_argument('--classes', type=int, default=2)
    ap.add_argument('--iters', type=int, default=100); ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--net-iters', type=int, default=5); ap.add_argument('--block', type=int, default=128)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'the measurement needs the GPU'
    T, S, V, C = a.depth, a.width, a.volume, a.classes
    g = torch.Generator(device='cuda').manual_seed(0)
    vol = torch.randint(1, 256, (V, V, V), dtype=torch.uint8, device='cuda', generator=g)
    np.random.seed(0)
    s = Slicer([V, V, V])
    s.randomize()
    s.origin = np.array([V, V, V]) / 2 + np.random.uniform(-3, 3, 3)
    print(f'slab {T} x {S} x {S} of a {V}^3 volume, rotation vector {np.round(s.rot_vec, 3).tolist()}; HIP events, median of {a.reps} x {a.iters} launches')
    vox = T * S * S
    # the same slab axis-aligned: rows (j, the lanes of a wave) along x, the volume's contiguous axis -- and across it, every sample of a
    # row on a cache line of its own
    along, across = Slicer([V, V, V]), Slicer([V, V, V])
    along.u, along.v, along.w = np.eye(3)
    across.u, across.v, across.w = np.eye(3)[[1, 2, 0]]
    for name, sl in (('random orientation', s), ('rows along x', along), ('rows along z', across)):
        for order in (0, 1):
            us = timed(lambda: sl.get_slab(vol, slice_width=S, depth=T, order=order), a.iters, a.reps)
            slab = sl.get_slab(vol, slice_width=S, depth=T, order=order)
            inside = float((slab != 0).float().mean())
            bound = 2 * vox / HBM * 1e6
            print(f'gather, {name}, order {order}: {fmt(us)}; byte bound {bound:.1f} us = ({vox / 1e6:.1f} MB written + {vox / 1e6:.1f} MB of samples) / 5 TB/s '
                  f'-> {100 * bound / np.median(us):.0f} % of it; {vox * (8 if order else 1) / 1e6:.1f} MB of taps at this order; '
                  f'{100 * inside:.1f} % of the samples inside the volume')
    probs = torch.rand((T, S, S, C), dtype=torch.float32, device='cuda', generator=g)
    pred = torch.zeros((V, V, V, C), dtype=torch.uint8, device='cuda')
    margin, border = T // 4, S // 4
    lo, length = s.slab_paste_box(pred.shape, 0, S, T, (margin, T - margin), border)
    us = timed(lambda: predict.update_predicted_volume(pred, probs, s), a.iters, a.reps)
    kept = int((pred.sum(-1) > 0).sum())                 # (random probabilities: a pasted voxel with every byte 0 has probability 255^-C)
    bound = kept * 5 * C / HBM * 1e6
    print(f'paste of the core (planes {margin} .. {T - margin}, border {border}; {C} classes): {fmt(us)}; box {tuple(int(v) for v in length)} = '
          f'{int(np.prod(length)) / 1e6:.1f} M voxels visited, {kept / 1e6:.2f} M written; byte bound {bound:.1f} us = {kept * 5 * C / 1e6:.1f} MB / 5 TB/s '
          f'-> {100 * bound / np.median(us):.0f} % of it')
    # end to end against the whole-volume path's 3-D prediction of the same voxel count
    from interactive_unet.unet import UNet
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = UNet(num_classes=C, dim=3, pretrained=False)
    model.reset_parameters(seed=1)
    model = model.cuda().eval()
    eng = model.engine('eval')
    ms = [u / 1e3 for u in timed(lambda: predict.predict_slab(model, vol, s, slice_width=S, depth=T), a.net_iters, a.reps, warm=3)]
    form = eng.describe()['form'] if hasattr(eng, 'describe') else type(eng).__name__
    B = a.block
    nblk = max(1, vox // B ** 3)
    acc = predict.VolumeAccumulator((V, V, V), C, B, 'cuda')
    coords = [np.array([i * B, 0, 0, (i + 1) * B, B, B]) for i in range(nblk)]
    local = [np.array([0, 0, 0, B, B, B])] * nblk
    run = lambda: predict.predict_blocks_3d(eng, acc, vol, coords, coords, local, 0, nblk)
    mb = [u / 1e3 for u in timed(lambda: eng.run_checked(run) if hasattr(eng, 'run_checked') else run(), a.net_iters, a.reps, warm=3)]
    print(f'predict_slab end to end ({form}): {np.median(ms):.2f} ms (min {min(ms):.2f}, max {max(ms):.2f}) = {vox / np.median(ms) / 1e3:.0f} M voxels/s; '
          f'{nblk} blocks of {B}^3 ({nblk * B ** 3 / 1e6:.1f} M voxels, the slab has {vox / 1e6:.1f} M) through predict_blocks_3d: '
          f'{np.median(mb):.2f} ms (min {min(mb):.2f}, max {max(mb):.2f}) = {nblk * B ** 3 / np.median(mb) / 1e3:.0f} M voxels/s')


if __name__ == '__main__':
    main()
