"""Placement of a kernel test's device operands inside larger, sentinel-filled allocations.

The networks never hand a kernel a tight, exactly sized buffer: an activation is a half of a concat buffer, a gradient a slot of
a multi-slot buffer, the sample stride is anything that keeps 16-byte alignment.  A kernel test that allocates through this module
gives every operand a PLACEMENT -- `lead` elements into an allocation, samples `ss` elements apart -- and afterwards checks that
  (a) the logical contents are what the reference says (`Operand.logical`),
  (b) every element outside the logical extents of the samples still holds the sentinel bits (`Operand.check_outside`),
  (c) an input's whole allocation is bit-identical to what it was before the call (`Operand.check_unchanged`).
The sentinel is a NaN of the element type (0x7FA5 in f16 and bf16, 0x7FA5A5A5 in fp32; 0xA5 for bytes), so a halo load that strays
into the gap between two samples shows in the result even when it meets a zero weight, and an output element nobody wrote is a NaN
in the comparison.  Nothing here provokes a fault: every access a correct or a stride-confused kernel makes stays inside the
allocation as long as it stays within one sample stride of the operand, which is what the bands at both ends are for.

No GPU is needed to import this module; the device is only touched when an Operand is created with device='cuda'."""
import ctypes

import torch

SENTINEL = {torch.float16: 0x7FA5, torch.bfloat16: 0x7FA5, torch.float32: 0x7FA5A5A5, torch.uint8: 0xA5}
INT_VIEW = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}
BAND = 8 * 256            # sentinel elements in front of the first and behind the last sample, whatever the placement

PLACEMENTS = ('tight', 'gap', 'upper', 'lower')


def placement(kind, per):
    """(ss, lead) of a placement for an operand of `per` = C * vox elements per sample.  Strides stay multiples of 8 elements
    (16 bytes in the 16-bit types): all the blocked layout and the networks guarantee."""
    if kind == 'tight':
        return per, 0
    if kind == 'gap':
        return per + 8 * 37, 8 * 5
    if kind == 'upper':       # the second half of a two-slot (concat) buffer
        return 2 * per, per
    if kind == 'lower':       # its mirror image
        return 2 * per, 0
    raise ValueError(f'unknown placement {kind!r}: {PLACEMENTS}')


def bits(t):
    """The integer view on which every comparison of this module is made (NaN payloads compare like any other bits)."""
    return t.contiguous().view(INT_VIEW[t.dtype])


def sentinel_filled(n, dtype, device='cpu'):
    iv = INT_VIEW[dtype]
    s = SENTINEL[dtype]
    if iv == torch.int16 and s >= 1 << 15:
        s -= 1 << 16
    return torch.full((n,), s, dtype=iv, device=device).view(dtype)


class Operand:
    """N samples of `per` elements each, placed in one allocation: [band | lead | sample 0 | ... ] with samples `ss` apart.
    data: a CPU tensor of N * per elements (an input), or None (an output or scratch: the logical extents hold the sentinel
    too, so an unwritten element is a NaN).  `t` is the device view that starts at sample 0: pass its pointer and `ss`."""

    def __init__(self, N, per, dtype, place='tight', data=None, device='cuda', name='operand', band=BAND):
        self.N, self.per, self.dtype, self.place, self.name, self.band = N, int(per), dtype, place, name, band
        self.ss, self.lead = placement(place, self.per)
        self.total = band + N * self.ss + band
        host = sentinel_filled(self.total, dtype)
        self.inside = torch.zeros(self.total, dtype=torch.bool)
        for n in range(N):
            a = self.start(n)
            self.inside[a:a + self.per] = True
            if data is not None:
                host[a:a + self.per] = data.reshape(N, self.per)[n].to(dtype)
        self.is_input = data is not None
        self.before = bits(host).clone()
        self.buf = host.to(device)
        self.t = self.buf[band + self.lead:]

    def start(self, n):
        return self.band + self.lead + n * self.ss

    def host(self):
        return self.buf.cpu()

    def logical(self):
        """The operand's contents, [N, per] on the CPU."""
        h = self.host()
        return torch.stack([h[self.start(n):self.start(n) + self.per] for n in range(self.N)])

    def _where(self, i):
        """Offset i of the allocation relative to the nearest sample."""
        n = min(range(self.N), key=lambda k: min(abs(i - self.start(k)), abs(i - (self.start(k) + self.per - 1))))
        rel = i - self.start(n)
        side = 'before the start' if rel < 0 else 'past the end'
        d = -rel if rel < 0 else rel - self.per + 1
        return f'{d} elements {side} of sample {n} (allocation offset {i}, ss {self.ss}, lead {self.lead}, per {self.per})'

    def check_outside(self):
        """(b): nothing outside the samples' logical extents was written."""
        now = bits(self.host())
        bad = (now != self.before) & ~self.inside
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            raise AssertionError(f'{self.name} [{self.place}]: {int(bad.sum())} sentinel elements overwritten, the first {self._where(i)}: '
                                 f'bits {int(now[i]) & 0xFFFFFFFF:#x}')

    def check_unchanged(self):
        """(c): an input is bit-identical to what it was before the call, gaps and bands included."""
        now = bits(self.host())
        bad = now != self.before
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            what = 'inside' if bool(self.inside[i]) else 'outside'
            raise AssertionError(f'{self.name} [{self.place}]: input modified ({int(bad.sum())} elements), the first {what} the samples, '
                                 f'{self._where(i)}')

    def check(self):
        if self.is_input:
            self.check_unchanged()
        else:
            self.check_outside()


def scratch(nelems, dtype=torch.float32, device='cuda', name='scratch'):
    """Scratch of exactly the size the library reports, sentinel-filled (a NaN: a row the entry point leaves unwritten shows in what
    is reduced from it), with a band behind and in front that check_outside() watches."""
    return Operand(1, nelems, dtype, 'tight', None, device, name)


def source_tables(operands):
    """The pointer table and the sample-stride table (`const void* const*`, `const long long*`) of the entry points that read several
    sources in one launch (iunet_sf_gemm, iunet_sf_wgrad), from one Operand per source: each at its own placement."""
    n = len(operands)
    return ((ctypes.c_void_p * n)(*[o.t.data_ptr() for o in operands]), (ctypes.c_longlong * n)(*[o.ss for o in operands]))


def pointer_table(operands):
    """A `const void* const*` table of small parameter vectors (one Operand each), e.g. the per-source prologue scales."""
    return (ctypes.c_void_p * len(operands))(*[o.t.data_ptr() for o in operands])


class StridedInput:
    """A caller's planar tensor [N, C, D, H, W] as a strided view of a larger one (row, plane, channel and sample pitch larger than
    the extents), the way the first conv reads it; the surroundings hold the sentinel and the whole thing is an input."""

    def __init__(self, x, pad=(1, 2, 3, 5), device='cuda', name='x'):
        N, C, D, H, W = x.shape
        pc, pd, ph, pw = pad
        big = sentinel_filled(N * (C + pc) * (D + pd) * (H + ph) * (W + pw) + 2 * 64, x.dtype)
        body = big[64:-64].view(N, C + pc, D + pd, H + ph, W + pw)
        body[:, :C, :D, :H, :W] = x
        self.name = name
        self.before = bits(big).clone()
        self.buf = big.to(device)
        self.t = self.buf[64:]
        self.strides = tuple(body.stride())

    def check(self):
        now = bits(self.buf.cpu())
        bad = now != self.before
        if bool(bad.any()):
            raise AssertionError(f'{self.name}: strided input modified, first at allocation offset {int(bad.nonzero()[0])}')


class StridedOutput:
    """The mirror image of StridedInput for an output [N, C, D, H, W] that a kernel writes through element strides: channels last
    (sC = 1), every pitch larger than its extent.  The body and its surroundings start as the sentinel; `logical()` is what was written
    (planar, on the CPU), `check()` that nothing outside it was."""

    def __init__(self, shape, dtype=torch.float32, pad=(1, 2, 3, 5), device='cuda', name='out'):
        N, C, D, H, W = shape
        pc, pd, ph, pw = pad
        self.shape, self.name, self.is_input = tuple(shape), name, False
        self.full = (N, D + pd, H + ph, W + pw, C + pc)
        big = sentinel_filled(N * (D + pd) * (H + ph) * (W + pw) * (C + pc) + 2 * 64, dtype)
        body = big[64:-64].view(self.full)
        sn, sd, sh, sw, sc = body.stride()
        self.strides = (sn, sc, sd, sh, sw)
        self.inside = torch.zeros(big.numel(), dtype=torch.bool)
        self.inside[64:-64].view(self.full)[:, :D, :H, :W, :C] = True
        self.before = bits(big).clone()
        self.buf = big.to(device)
        self.t = self.buf[64:]

    def logical(self):
        N, C, D, H, W = self.shape
        return self.buf.cpu()[64:-64].view(self.full)[:, :D, :H, :W, :C].permute(0, 4, 1, 2, 3).contiguous()

    def check(self):
        bad = (bits(self.buf.cpu()) != self.before) & ~self.inside
        if bool(bad.any()):
            raise AssertionError(f'{self.name}: {int(bad.sum())} sentinel elements of a strided output overwritten, first at allocation offset {int(bad.nonzero()[0])}')


# ---- the eval-mode BatchNorm fold every pack / prep kernel promises (csrc/common.h: bn_fold_scale / bn_fold_mul / bn_fold_bias), shared by
# the read-back tests of the fp32 form and of the other pack entry points
def sqrt_rn(t):
    """The correctly rounded fp32 square root (the device's __fsqrt_rn): the float64 root rounded once more, which is innocuous for a
    square root (53 >= 2 x 24 + 2 bits).  torch.sqrt on fp32 CPU tensors is NOT always correctly rounded (its vectorised path is one
    unit off for ~0.7 % of random arguments; tests/test_f32_matrix_cpu.py holds this function to numpy's fp32 root instead)."""
    return torch.sqrt(t.double()).float()


def fold_ref(w, bn, eps, transposed):
    """The eval-mode BatchNorm fold in separately, correctly rounded fp32 operations: a = gamma / sqrt(var + eps), w' = w a, bias = beta - mean a."""
    gamma, beta, mean, var = [t.float() for t in bn]
    a = gamma / sqrt_rn(var + torch.tensor(eps, dtype=torch.float32))
    shape = [1] * w.dim()
    shape[1 if transposed else 0] = -1
    return w * a.view(shape), beta - mean * a


# ---- the split forms of the prediction kernels (csrc/split16.hip, conv3_x2m.hip): channel-blocked planes inside a sentinel-filled allocation
SPLIT_PLACEMENTS = ('tight', 'gap', 'skip', 'up')


def blocked(x, cpp):
    """[N, C, ...] -> the channel-blocked planes [N][C / cpp][vox][cpp], flat per sample."""
    N, C = x.shape[:2]
    return x.reshape(N, C // cpp, cpp, -1).permute(0, 1, 3, 2).contiguous().reshape(N, -1)


def unblocked(flat, C, sp, cpp):
    """The inverse of blocked(): [N, C / cpp * vox * cpp] -> [N, C, *sp]."""
    N = flat.shape[0]
    return flat.reshape(N, C // cpp, -1, cpp).permute(0, 1, 3, 2).reshape((N, C) + tuple(sp))


class PlaneOperand:
    """N samples of `total` planes of [vox][cpp] elements each, `ss` elements apart, of which the operand owns the planes [p0, p0 + C / cpp)
    -- and, with lo >= 0, the planes [p0 + lo, p0 + lo + C / cpp) -- everything else, the bands at both ends included, holds the sentinel.
    Placements (`planes` = C / cpp; `pad` = 8 elements of a 16-bit type, 16 bytes: strides keep the 16-byte alignment the layout guarantees):
      tight  [own | lo] (or [own] alone), ss = total planes;          gap   the same, ss + 37 pad, 5 pad into the allocation;
      skip   the lower half of a concat buffer of 2 C channels, [skip | up | skip_lo | up_lo] (without lo planes: [skip | up]);
      up     its upper half: p0 = planes.
    `lo_at` overrides the distance of the lo planes at tight / gap (the hole in between holds the sentinel).  `t` is the device view that
    starts at plane p0 of sample 0: pass its pointer, `ss` and `lo`.  first / second: CPU tensors [N, C, ...] (an input) or None."""

    def __init__(self, N, C, vox, dtype, cpp, place, first=None, second=None, own_lo=True, lo_at=None, pair=True, device='cuda', name='operand',
                 band=BAND):
        planes, plane = C // cpp, vox * cpp
        pad = 8 if dtype != torch.uint8 else 16
        assert C % cpp == 0 and place in SPLIT_PLACEMENTS and (second is None or own_lo)
        if place in ('tight', 'gap'):
            p0, lo = 0, (lo_at or planes) if own_lo else -1
            total = lo + planes if own_lo else planes
        else:
            p0, lo = (0 if place == 'skip' else planes), (2 * planes if own_lo else -1)
            total = 4 * planes if pair else 2 * planes
        self.N, self.C, self.vox, self.dtype, self.cpp, self.place, self.name, self.band = N, C, vox, dtype, cpp, place, name, band
        self.planes, self.plane, self.p0, self.lo, self.total_planes = planes, plane, p0, lo, total
        self.ss = total * plane + (37 * pad if place == 'gap' else 0)
        self.lead = 5 * pad if place == 'gap' else 0
        self.per = planes * plane
        self.total = band + N * self.ss + band
        host = sentinel_filled(self.total, dtype)
        self.inside = torch.zeros(self.total, dtype=torch.bool)
        for k, data in enumerate((first, second) if own_lo else (first,)):
            rows = blocked(data, cpp).to(dtype) if data is not None else None
            for n in range(N):
                a = self.start(n, k)
                self.inside[a:a + self.per] = True
                if rows is not None:
                    host[a:a + self.per] = rows[n]
        self.is_input = first is not None
        self.before = bits(host).clone()
        self.buf = host.to(device)
        self.t = self.buf[band + self.lead + p0 * plane:]

    def start(self, n, second=0):
        return self.band + self.lead + n * self.ss + (self.p0 + (self.lo if second else 0)) * self.plane

    def host(self):
        return self.buf.cpu()

    def _read(self, second):
        h = self.host()
        return torch.stack([h[self.start(n, second):self.start(n, second) + self.per] for n in range(self.N)])

    def check_outside(self):
        now = bits(self.host())
        bad = (now != self.before) & ~self.inside
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            n, r = divmod(i - self.band - self.lead, self.ss)
            raise AssertionError(f'{self.name} [{self.place}]: {int(bad.sum())} sentinel elements overwritten, the first in plane {r // self.plane} '
                                 f'(element {r % self.plane}) of sample slot {n}; the operand owns planes {self.p0}..{self.p0 + self.planes - 1}'
                                 + (f' and {self.p0 + self.lo}..{self.p0 + self.lo + self.planes - 1}' if self.lo >= 0 else '') + f' of {self.total_planes}')

    def check_unchanged(self):
        now = bits(self.host())
        bad = now != self.before
        if bool(bad.any()):
            raise AssertionError(f'{self.name} [{self.place}]: input modified ({int(bad.sum())} elements), first at allocation offset {int(bad.nonzero()[0])}')

    def check(self):
        if self.is_input:
            self.check_unchanged()
        else:
            self.check_outside()


class SplitOperand(PlaneOperand):
    """A tensor of the fp16x2 form: C / 8 hi planes of [vox][8] fp16 and, with own_lo, its lo planes `lo` planes further on."""

    def __init__(self, N, C, vox, place='tight', hi=None, lo=None, own_lo=True, lo_at=None, device='cuda', name='split'):
        super().__init__(N, C, vox, torch.float16, 8, place, hi, lo, own_lo, lo_at, True, device, name)

    def logical(self):
        """(hi words, lo words or None), each [N, C / 8 * vox * 8] on the CPU."""
        return self._read(0), (self._read(1) if self.lo >= 0 else None)

    def values(self, sp):
        """hi and lo words as fp32 [N, C, *sp] (lo: zeros where the operand owns none)."""
        h, l = self.logical()
        h = unblocked(h.float(), self.C, sp, 8)
        return h, (unblocked(l.float(), self.C, sp, 8) if l is not None else torch.zeros_like(h))


class M8Operand(PlaneOperand):
    """The lo8 granule planes of a tensor of the x2m form: C / 16 planes of [vox][16] e4m3 bytes; skip / up: the halves of a concat buffer's
    granule planes (the upper half starts C / 16 planes in)."""

    def __init__(self, N, C, vox, place='tight', lo8=None, device='cuda', name='m8'):
        super().__init__(N, C, vox, torch.uint8, 16, place, lo8, None, False, None, False, device, name)

    def logical(self):
        return self._read(0)

    def codes(self, sp):
        """The e4m3 bytes [N, C, *sp]."""
        return unblocked(self.logical(), self.C, sp, 16)
