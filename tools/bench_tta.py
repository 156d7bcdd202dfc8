"""Time the 3-D net's symmetry ensemble at the sizes predict_volumes would use: 128^3 blocks of a 256^3 volume.
  * iunet_sym_block on a 128^3 uint8 block, one code of each of the six permutations with f = 0 and with f = 7, against its byte bound:
    2 S^3 bytes (read + written) over 5 TB/s;
  * iunet_sym_accumulate on the block's fp32 [S, S, S, C] probabilities for the same codes, a middle member of an ensemble (index 1 of 3:
    q read, sum / mn / mx read and written), against 7 x 4 C S^3 bytes over 5 TB/s; and the mean-only call (q read, sum read and written);
  * predict.predict_volume_array of a --volume^3 volume at input_size --block, end to end (upload excluded: the volume is resident), for
    each --tta entry (none, flips, planar, full or codes joined by '+'), in the default prediction mode; the ratio to the `none` row, and
    how much of the excess over G forwards the two kernels account for (G x blocks x their middle-call times, row-preserving and
    transposing codes weighted as the set mixes them).
HIP events after warm-up, `--reps` times: median and spread.  `--pkg DIR` times another checkout's package (one without the tta keyword
is called without it: its `none` row is the A/B partner of this one's).
   python tools/bench_tta.py [--what kernels,e2e] [--tta none,flips,full] [--volume 256] [--block 128] [--classes 2] [--pkg DIR]"""
import argparse, json, os, sys, warnings
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HBM = 5e12        # bytes / s: the figure DESIGN.md uses for HBM passes
CODES = [8 * pi + f for pi in range(6) for f in (0, 7)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--what', default='kernels,e2e'); ap.add_argument('--tta', default='none,flips,full')
    ap.add_argument('--volume', type=int, default=256); ap.add_argument('--block', type=int, default=128)
    ap.add_argument('--classes', type=int, default=2); ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--reps', type=int, default=7); ap.add_argument('--pkg', default=ROOT); ap.add_argument('--json', default=None)
    a = ap.parse_args()
    pkg = os.path.abspath(a.pkg)
    sys.path.insert(0, os.path.join(pkg, 'interactive-unet_amd')); sys.path.insert(0, pkg)
    import numpy as np
    import torch
    from interactive_unet import predict, _native as nv
    assert torch.cuda.is_available(), 'the measurement needs the GPU'
    S, V, C = a.block, a.volume, a.classes
    what = a.what.split(',')
    result = {'pkg': pkg, 'block': S, 'volume': V, 'classes': C}

    def timed(fn, iters, reps, warm):
        for _ in range(warm): fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters): fn()
            e1.record(); torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / iters * 1e3)
        return out

    fmt = lambda us: f'{np.median(us):.1f} us (min {min(us):.1f}, max {max(us):.1f})'
    g = torch.Generator(device='cuda').manual_seed(0)
    kernel_us = {}
    if 'kernels' in what:
        vox = S ** 3
        blk = torch.randint(0, 256, (S, S, S), dtype=torch.uint8, device='cuda', generator=g)
        out = torch.empty_like(blk)
        # the accumulate's buffers rotate through `nset` sets, 512 MB together: twice the 256 MB Infinity Cache, so that back-to-back
        # launches meet HBM as a call between two forwards does (one set, 117 MB at 128^3 x 2, would be timed out of that cache)
        nset = max(1, -(-(512 << 20) // (4 * 4 * C * vox)))
        sets = [(torch.rand((S, S, S, C), dtype=torch.float32, device='cuda', generator=g),) + tuple(torch.zeros((S, S, S, C), device='cuda') for _ in range(3))
                for _ in range(nset)]
        turn = [0]

        def accumulate(sym, trio):
            q, s, mn, mx = sets[turn[0] % nset]
            turn[0] += 1
            nv.call('iunet_sym_accumulate', nv.ptr(q), S, S, S, C, sym, 1, 3, 1 / 3, nv.ptr(s), nv.ptr(mn) if trio else None, nv.ptr(mx) if trio else None,
                    None, nv.ptr(spread) if trio else None, nv.stream())
        spread = torch.empty((S, S, S), dtype=torch.float32, device='cuda')      # (written by an ensemble's last call only)
        b_blk, b_acc, b_mean = 2 * vox / HBM * 1e6, 7 * 4 * C * vox / HBM * 1e6, 3 * 4 * C * vox / HBM * 1e6
        print(f'block {S}^3, {C} classes; HIP events, median of {a.reps} x {a.iters} launches; byte bounds at 5 TB/s: sym_block {b_blk:.2f} us '
              f'({2 * vox / 1e6:.1f} MB), sym_accumulate {b_acc:.1f} us ({7 * 4 * C * vox / 1e6:.0f} MB), mean-only {b_mean:.1f} us; the accumulate rotates '
              f'through {nset} buffer sets ({nset * 16 * C * vox / 2 ** 20:.0f} MB)')
        for sym in CODES:
            ub = timed(lambda: nv.call('iunet_sym_block', nv.ptr(blk), S, S, S, sym, nv.ptr(out), nv.stream()), a.iters, a.reps, 10)
            ua = timed(lambda: accumulate(sym, True), a.iters, a.reps, 10)
            um = timed(lambda: accumulate(sym, False), a.iters, a.reps, 10)
            kernel_us[sym] = (float(np.median(ub)), float(np.median(ua)), float(np.median(um)))
            print(f'sym {sym:2d} (pi {sym >> 3}, f {sym & 7}): sym_block {fmt(ub)} -> {100 * b_blk / np.median(ub):.0f} % of its bound; '
                  f'sym_accumulate {fmt(ua)} -> {100 * b_acc / np.median(ua):.0f} %; mean-only {fmt(um)} -> {100 * b_mean / np.median(um):.0f} %')
        result['kernels_us'] = {str(k): v for k, v in kernel_us.items()}
    if 'e2e' in what:
        from interactive_unet.unet import UNet
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            model = UNet(num_classes=C, dim=3, pretrained=False)
        model.reset_parameters(seed=1)
        model = model.cuda().eval()
        eng = model.engine('eval')
        vol = torch.randint(1, 256, (V, V, V), dtype=torch.uint8, device='cuda', generator=g)
        nblk = len(predict.get_block_coordinates(np.array([V, V, V]), input_size=S, overlap=0.25)[0])
        has_tta = 'tta' in predict.predict_volume_array.__code__.co_varnames
        rows = {}
        for name in a.tta.split(','):
            spec = None if name == 'none' else (name if not name[0].isdigit() else [int(t) for t in name.split('+')])
            if spec is not None and not has_tta:
                print(f'tta {name}: this package has no tta keyword'); continue
            kw = dict(tta=spec) if spec is not None else {}
            acc = predict.VolumeAccumulator((V, V, V), C, S, 'cuda')

            def once():
                acc.reset()
                run = lambda: predict.predict_volume_array(model, vol, input_size=S, num_classes=C, accumulator=acc, **kw)
                return eng.run_checked(run) if hasattr(eng, 'run_checked') else run()
            ms = [u / 1e3 for u in timed(once, 1, a.reps, 2)]
            rows[name] = ms
            G = 1
            if spec is not None:
                from interactive_unet import tta
                G = len(tta.members(spec))
            line = f'predict_volume_array {V}^3 at input_size {S} ({nblk} blocks), tta {name} (G = {G}): {np.median(ms):.1f} ms (min {min(ms):.1f}, max {max(ms):.1f})'
            if 'none' in rows and spec is not None:
                base = float(np.median(rows['none']))
                excess = float(np.median(ms)) - G * base
                line += f'; {np.median(ms) / base:.2f} x the none row, excess over G x none {excess:+.1f} ms'
                if kernel_us:
                    from interactive_unet import tta
                    k_ms = sum(kernel_us[8 * (m >> 3)][0] + kernel_us[8 * (m >> 3)][2] for m in tta.members(spec)) * nblk / 1e3
                    line += f'; the two kernels: {k_ms:.1f} ms of the run (sym_block + mean-only accumulate per member and block)'
            print(line)
        form = eng.describe()['form'] if hasattr(eng, 'describe') else type(eng).__name__
        print(f'prediction mode: {form}')
        result['e2e_ms'] = rows
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(result, f)


if __name__ == '__main__':
    main()
