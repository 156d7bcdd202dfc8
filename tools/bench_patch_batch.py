"""Time the 3-D patch batch producer (interactive_unet.loader.VolumeDataset, iunet_patch_batch) at the shape of the 3-D training
step it feeds -- batch 2, 128^3 patches, 1 channel, 2 classes, randomly rotated and scaled patches of a 256^3 volume -- at spline
orders 0 and 1, against its byte bound (bytes written + bytes gathered over 5 TB/s).  HIP events around `--iters` launches on fixed
descriptors, `--reps` times: median and spread; then the wall time of VolumeDataset.batch with the parameter draw and the
descriptor upload.  --elastic / --color-jitter / --blur-or-noise {blur,noise,mixed} time, after the plain launch, the pipeline of
iunet_patch_batch_extra on fixed drawn parameters the same way (kernel by kernel: run it under
rocprofv3 --kernel-trace --stats); --train-step times the dim = 3 training step on the produced batch in the same run.
   python tools/bench_patch_batch.py [--batch 2] [--patch 128] [--volume 256] [--elastic] [--color-jitter] [--blur-or-noise mixed]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'interactive-unet_amd')); sys.path.insert(0, ROOT)
import numpy as np
import torch
from interactive_unet import loader, _native as nv

HBM = 5e12        # bytes / s: the figure DESIGN.md uses for HBM passes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=2); ap.add_argument('--patch', type=int, default=128)
    ap.add_argument('--volume', type=int, default=256); ap.add_argument('--channels', type=int, default=1)
    ap.add_argument('--classes', type=int, default=2); ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--elastic', action='store_true'); ap.add_argument('--color-jitter', action='store_true')
    ap.add_argument('--blur-or-noise', choices=('blur', 'noise', 'mixed')); ap.add_argument('--train-step', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'the measurement needs the GPU'
    B, S, V, ch, C = a.batch, a.patch, a.volume, a.channels, a.classes
    g = torch.Generator(device='cuda').manual_seed(0)
    image = torch.randint(1, 256, (V, V, V, ch), dtype=torch.uint8, device='cuda', generator=g)
    mask = torch.randint(0, C, (V, V, V), dtype=torch.uint8, device='cuda', generator=g)
    weight = torch.zeros((V, V, V, 2), dtype=torch.uint8, device='cuda')
    weight[V // 3] = weight[:, V // 2] = weight[:, :, 2 * V // 3] = 255            # three annotated slices
    vox = B * S ** 3
    written, gathered = vox * (ch + 2 * C) * 2, {0: vox * (ch + 2), 1: vox * (8 * ch + 2)}
    for order in (0, 1):
        ds = loader.VolumeDataset([(image, mask, weight)], C, patch_size=S, count=B, order=order, generator=torch.Generator().manual_seed(1))
        params = [ds.draw() for _ in range(B)]
        raw = torch.frombuffer(bytearray(bytes(ds.descriptors(params))), dtype=torch.uint8).cuda()
        X, y, w = ds.batch(list(range(B)), params)

        def launch():
            nv.call('iunet_patch_batch', nv.ptr(raw), B, ch, C, S, S, S, order, nv.ptr(ds._lut), nv.ptr(X), nv.ptr(y), nv.ptr(w), nv.stream())

        def timed(fn):
            for _ in range(20): fn()
            torch.cuda.synchronize()
            us = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters): fn()
                e1.record(); torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) / a.iters * 1e3)
            return us
        us = timed(launch)
        t0 = time.time()
        for _ in range(50): ds.batch(list(range(B)))
        torch.cuda.synchronize()
        wall = (time.time() - t0) / 50 * 1e6
        # the bound counts one byte per gathered tap; neighbouring lanes share taps and cache lines, so it is the traffic the launch asks
        # for, not what reaches HBM
        bound = (written + gathered[0]) / HBM * 1e6
        lit = float((w[:, 0] > 0).float().mean())
        print(f'order {order}: batch {B} x {S}^3 from {V}^3, {ch} channel(s), {C} classes: {np.median(us):.1f} us per launch (HIP events, median of '
              f'{a.reps} x {a.iters} launches; min {min(us):.1f}, max {max(us):.1f}); byte bound {bound:.1f} us = ({written / 1e6:.1f} MB written + '
              f'{gathered[0] / 1e6:.1f} MB gathered at order 0) / 5 TB/s; {gathered[order] / 1e6:.1f} MB of taps at this order; '
              f'{wall:.0f} us wall per VolumeDataset.batch with the draw and the descriptor upload; {100 * lit:.1f} % of the voxels annotated')
        if a.elastic or a.color_jitter or a.blur_or_noise:
            extra_launch(a, ds, params, raw, order, timed)
    if a.train_step:
        train_step(a, X, y, w)


def extra_launch(a, ds, params, raw, order, timed):
    """The pipeline of iunet_patch_batch_extra on the same patch descriptors, with drawn parameters of the transforms asked for
    ('mixed': blur and noise samples alternate)."""
    import ctypes
    B, S, ch, C = a.batch, a.patch, a.channels, a.classes
    extras = (loader.PatchExtraDesc * B)()
    use = 0
    for k, d in enumerate(extras):
        e = loader.draw_extra(ds.generator, a.elastic, a.color_jitter, a.blur_or_noise is not None)
        if a.blur_or_noise:
            kind = a.blur_or_noise if a.blur_or_noise != 'mixed' else ('blur', 'noise')[k % 2]
            e['blur_or_noise'] = {'kind': 'blur', 'sigma': 1.0} if kind == 'blur' else {'kind': 'noise', 'key': 12345 + k, 'sigma': 0.1}
        use |= loader._fill_patch_extra(d, e)
    xraw = torch.frombuffer(bytearray(bytes(extras)), dtype=torch.uint8).cuda()
    taps = torch.from_numpy(loader.gaussian_taps(ds.elastic_sigma)).cuda()
    ws = torch.empty(nv.answer(nv.lib().iunet_patch_extra_ws_bytes(B, ch, S, S, S)), dtype=torch.uint8, device='cuda')
    X = torch.empty((B, ch, S, S, S), dtype=torch.float16, device='cuda')
    y = torch.empty((B, C, S, S, S), dtype=torch.float16, device='cuda'); w = torch.empty_like(y)

    def launch():
        nv.call('iunet_patch_batch_extra', nv.ptr(raw), nv.ptr(xraw), use, B, ch, C, S, S, S, order, nv.ptr(ds._lut), nv.ptr(taps), int(taps.numel()),
                nv.ptr(ws), int(ws.numel()), nv.ptr(X), nv.ptr(y), nv.ptr(w), nv.stream())
    us = timed(launch)
    d = ws[:12 * B * S ** 3].view(torch.float32).double()
    rms = f'; RMS of a displacement component {float((d ** 2).mean().sqrt()):.3f} voxels, of the vector {float((d ** 2).mean().mul(3).sqrt()):.3f}' if a.elastic else ''
    name = ' + '.join(n for n, on in (('elastic', a.elastic), ('jitter', a.color_jitter), (a.blur_or_noise, a.blur_or_noise)) if on)
    print(f'order {order}, {name} (use {use}): {np.median(us):.1f} us per iunet_patch_batch_extra call (HIP events, median of {a.reps} x {a.iters}; min '
          f'{min(us):.1f}, max {max(us):.1f}); workspace {ws.numel() / 1e6:.1f} MB, {int(taps.numel())} elastic taps{rms}')


def train_step(a, X, y, w):
    """The dim = 3 training step the producer feeds (bf16, MCC + CE), on the batch it produced: median of 5 x 10 steps."""
    import warnings
    from interactive_unet.unet import UNet
    from interactive_unet.train_engine import TrainEngine
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        m = UNet(lr=1e-3, num_channels=a.channels, num_classes=a.classes, dim=3, act_dtype='bf16', pretrained=False).cuda()
    te = TrainEngine(m, lr=1e-3, loss_kind='mcc_ce')
    for _ in range(5): te.train_step(X, y, w)
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        t0 = time.time()
        for _ in range(10): te.train_step(X, y, w)
        torch.cuda.synchronize()
        ms.append((time.time() - t0) / 10 * 1e3)
    print(f'3-D training step (bf16, batch {a.batch} x {a.patch}^3): {np.median(ms):.2f} ms (median of 5 x 10 steps; min {min(ms):.2f}, max {max(ms):.2f})')


if __name__ == '__main__':
    main()
