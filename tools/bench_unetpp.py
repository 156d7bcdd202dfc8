"""U-Net++ against U-Net at the same shape: the 16-bit training step (fp16, MCC+CE, both sequenced from Python) and one 2.5-D block
prediction (every axis' slices of an S^3 block through the 2-D net, each model in its default prediction form: U-Net++ fp32, U-Net
split precision; and both in fp16).  GPU time from HIP events, mean of n runs after warm-up.  Then the U-Net++ training step and
validation step sequenced from Python against the same step as one C call (TrainHandle over iunet_train_create_nested, NetGraph over
iunet_net_create_nested): GPU event time and host wall time per step.
    python tools/bench_unetpp.py [batch] [slice] [block]"""
import os, sys, time, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'interactive-unet_amd'))
import torch
from interactive_unet.unet import UNet
from interactive_unet import predict

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
S = int(sys.argv[2]) if len(sys.argv) > 2 else 512
BLK = int(sys.argv[3]) if len(sys.argv) > 3 else 128


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


def timed2(fn, n=20, warm=3):
    """(GPU event ms, host wall ms) per call: the wall clock runs from the first enqueue to the end of the last step on the device."""
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, (time.perf_counter() - t0) * 1e3 / n


def model(arch, dim=2, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return UNet(architecture=arch, num_classes=2, dim=dim, pretrained=False, **kw).cuda()


g = torch.Generator(device='cuda').manual_seed(0)
X = torch.randint(1, 255, (B, 1, S, S), dtype=torch.uint8, device='cuda', generator=g)
lab = X > 127
y = torch.cat([~lab, lab], 1).half()
w = torch.ones_like(y)
blk = torch.rand((BLK, BLK, BLK), device='cuda', generator=g)
out = torch.empty((BLK, BLK, BLK, 2), device='cuda')
res = {}
for arch in ('U-Net', 'U-Net++'):
    m = model(arch)
    te = m.train_engine()
    te.use_handle = False
    res[arch, 'train'] = timed(lambda: te.train_step(X, y, w, sync=False))
    for form, mm in (('default', model(arch)), ('fp16', model(arch, infer_dtype='fp16'))):
        mm.eval()
        res[arch, form] = timed(lambda: predict.predict_block_device(mm, blk, out, 2, BLK), n=3, warm=1)
    del te, m
for k in ('train', 'default', 'fp16'):
    a, b = res['U-Net', k], res['U-Net++', k]
    what = f'train step {B} x {S}^2 fp16' if k == 'train' else f'2.5-D block {BLK}^3, {k} prediction form'
    print(f'{what:48s}: U-Net {a:9.3f} ms, U-Net++ {b:9.3f} ms, ratio {b / a:.2f}', flush=True)

# U-Net++: the step sequenced from Python against the C-sequenced step (the handle serves every step after the first)
for tag, dim, N, sp, act in (('2-D fp16, batch 1 x 512^2', 2, 1, (512, 512), 'fp16'), ('2-D fp16, batch 8 x 512^2', 2, 8, (512, 512), 'fp16'),
                             ('3-D bf16, 2 x 64^3', 3, 2, (64, 64, 64), 'bf16')):
    Xs = torch.randint(1, 255, (N, 1) + sp, dtype=torch.uint8, device='cuda', generator=g)
    lb = Xs > 127
    ys = torch.cat([~lb, lb], 1).half()
    row = {}
    for how in ('python', 'handle'):
        te = model('U-Net++', dim, act_dtype=act).train_engine()
        te.use_handle = how == 'handle'
        row[how] = timed2(lambda: te.train_step(Xs, ys, None, sync=False))
        del te
    (pg, pw), (hg, hw) = row['python'], row['handle']
    print(f'U-Net++ train step {tag:28s}: Python-sequenced {pg:8.3f} ms GPU / {pw:8.3f} ms wall, C-sequenced {hg:8.3f} ms GPU / '
          f'{hw:8.3f} ms wall', flush=True)
    if dim == 2 and N == 8:
        te = model('U-Net++', dim, act_dtype=act).train_engine()
        te.train_step(Xs, ys, None)
        row = {}
        for how in ('python', 'handle'):
            if how == 'python':
                os.environ['IUNET_PY_EVAL'] = '1'
            else:
                os.environ.pop('IUNET_PY_EVAL', None)
            row[how] = timed2(lambda: te.eval_step(Xs, ys, None, sync=False))
        (pg, pw), (hg, hw) = row['python'], row['handle']
        print(f'U-Net++ validation step {tag:23s}: Python-sequenced {pg:8.3f} ms GPU / {pw:8.3f} ms wall, C-sequenced {hg:8.3f} ms GPU / '
              f'{hw:8.3f} ms wall', flush=True)
        del te
