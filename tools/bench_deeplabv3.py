"""DeepLabV3 against U-Net at the same shape: the 16-bit training step (MCC+CE, GPU time from HIP events, mean of n runs after warm-up) at
8 x 512^2 fp16 and at 2 x 128^3 bf16 (BASELINE config C3's shape), and one S^3 2.5-D block prediction (every axis' slices through the
2-D net) in each model's default prediction form (DeepLabV3 fp32, U-Net split precision) and in fp16.  Both training steps are sequenced
from Python (the U-Net's C handle off), so the comparison is of the launches, not of the sequencing.
    python tools/bench_deeplabv3.py [block]"""
import os, sys, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'interactive-unet_amd'))
import torch
from interactive_unet.unet import UNet
from interactive_unet import predict

BLK = int(sys.argv[1]) if len(sys.argv) > 1 else 128


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


def main():
    torch.manual_seed(0)
    rows = []
    for dim, N, sp, act in ((2, 8, (512, 512), 'fp16'), (3, 2, (128, 128, 128), 'bf16')):
        X = torch.rand((N, 1) + sp, device='cuda')
        lab = X[:, 0] > 0.5
        y = torch.stack([~lab, lab], 1).half()
        w = torch.ones_like(y)
        t = {}
        for arch in ('U-Net', 'DeepLabV3'):
            m = model(arch, dim, act_dtype=act)
            te = m.train_engine()
            te.use_handle = False
            t[arch] = timed(lambda: te.train_step(X, y, w, sync=False))
            del te, m
            torch.cuda.empty_cache()
        rows.append((f'train step {dim}-D {N} x {sp} {act}', t))
    blk = torch.rand((BLK,) * 3, device='cuda')
    for form in ('default', 'fp16'):
        t = {}
        for arch in ('U-Net', 'DeepLabV3'):
            kw = {} if form == 'default' else dict(infer_dtype='fp16')
            m = model(arch, 2, **kw).eval()
            out = torch.zeros((BLK,) * 3 + (2,), device='cuda')
            t[arch] = timed(lambda: predict.predict_block_device(m, blk, out, num_classes=2, batch_size=BLK), n=5, warm=2)
        rows.append((f'2.5-D block {BLK}^3, {form} form', t))
    for name, t in rows:
        print(f'{name:45s} U-Net {t["U-Net"]:9.2f} ms   DeepLabV3 {t["DeepLabV3"]:9.2f} ms   DeepLabV3 / U-Net {t["DeepLabV3"] / t["U-Net"]:.3f}')


if __name__ == '__main__':
    main()
