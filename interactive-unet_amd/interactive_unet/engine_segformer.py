"""Host-side plan of the native Segformer forward (Xie et al. 2021, smp's Segformer decoder on this project's encoder): folded eval-mode
BatchNorm, 16-bit (SegformerEngine, on engine.EncoderEngine's encoder) and fp32 (SegformerEngineF32, on engine_f32.EncoderEngineF32's).  Both keep
the `load_eval` / `infer(...)` interface predict.py drives.

Graph.  The decoder projects every encoder output X^l (mlp{l}), resizes it to the target grid T (the input grid / 4, level 2's grid),
concatenates the L maps deepest first and fuses them (1x1 conv, BatchNorm, ReLU).  All of that up to the BatchNorm is linear, so the engine
runs it as ONE gathered GEMM (csrc/segformer.hip): F = relu(s (sum_l M_l R_l(X^l) + beta - mean) + bn.bias) with M_l = W_f,l W_l folded and
packed once per load_eval, the B operand resampled straight out of the encoder tensors.  The 1x1 head gives the coarse logits on T; the
x4 upsampling (align_corners=True) writes iunet_head_fwd's output contract (logits / probs / class map, strides, divisor, accumulate).
No C-channel tensor finer than T and no L C-channel concat exists: the workspace table is `_Segformer._bufs`.
"""
import torch

from . import _native as nv
from .engine import BN_EPS, CoarseLogits, EncoderEngine, _vox
from .engine_f32 import EncoderEngineF32
from .topology import BN_KEYS

T_LEVEL = 2          # the target grid T is level 2's grid (stride 4)


def sources(ws, ch, dims, levels, P):
    """The gather GEMM's source table over the encoder outputs x{l}: (pointers, sample strides, channels, grids)."""
    xs = nv.ptr_array([P(ws[f'x{l}']).value for l in range(levels)])
    ss = nv.ll_array([ch[l] * _vox(dims[l]) for l in range(levels)])
    cin = nv.int_array(ch[:levels])
    grid = nv.int_array([e for l in range(levels) for e in dims[l]])
    return xs, ss, cin, grid


def pack_args(src, levels):
    """(ch array, fuse weight, mlp weight array, mlp bias array, kept sources) of iunet_sf_pack / iunet_sf_param_grads."""
    wf = src('fuse.conv.weight')
    w = [src(f'mlp{l}.weight') for l in range(levels)]
    b = [src(f'mlp{l}.bias') for l in range(levels)]
    return nv.ptr(wf), nv.ptr_array(w), nv.ptr_array(b), [wf] + w + b


class _Segformer(CoarseLogits):
    """What the two Segformer engines share: operator packing, workspace sizes, the decoder's launch."""
    coarse_level = T_LEVEL

    def _setup(self, decoder_channels):
        self.C = int(decoder_channels)
        if self.C % 32 or not (32 <= self.C <= 512) or not (3 <= self.levels <= 6):
            raise NotImplementedError(f'Segformer engine: decoder_channels {self.C} (a multiple of 32 in 32 .. 512), {self.levels} levels '
                                      f'(3 .. 6)')
        self.K = sum(self.ch)

    def _bufs(self, dims, N):
        """(element counts of the activation workspace, of the fp32 workspace): x{l} / a{l} / pin{l} of the encoder, feat (F on T);
        fp32: lc (coarse logits on T)."""
        act, ch = {}, self.ch
        for l in range(self.levels):
            v = _vox(dims[l])
            act[f'x{l}'] = N * ch[l] * v
            act[f'a{l}'] = N * ch[l] * v
            if l > 0:
                act[f'pin{l}'] = N * ch[l - 1] * v
        vt = _vox(dims[T_LEVEL])
        act['feat'] = N * self.C * vt
        return act, {'lc': N * self.ncls * vt}

    def _pack_decoder(self, src, dtype_code):
        """The collapsed decoder operator with fuse.bn folded: {sf: (operator [C][K], bias [C], kept sources), head}."""
        wf, w, b, keep = pack_args(src, self.levels)
        g = [src(f'fuse.bn.{k}') for k in BN_KEYS]
        dst = torch.empty(self.C * self.K, dtype=self._pack_dtype, device=self.device)
        bias = torch.empty(self.C, dtype=torch.float32, device=self.device)
        nv.call('iunet_sf_pack', dtype_code, self.levels, self.C, nv.int_array(self.ch), wf, w, b, nv.ptr(g[0]), nv.ptr(g[1]), nv.ptr(g[2]),
                nv.ptr(g[3]), BN_EPS, nv.ptr(dst), None, nv.ptr(bias), nv.stream())
        head = (src('head.weight').reshape(self.ncls, self.C).contiguous(), src('head.bias'))
        return {'sf': (dst, bias, keep + g), 'head': head}

    def _decode(self, ws, N):
        dims, C = ws['dims'], self.C
        dt = dims[T_LEVEL]
        xs, ss, cin, grid = sources(ws, self.ch, dims, self.levels, self._P)
        w, bias, _ = self.packed['sf']
        nv.call('iunet_sf_gemm', self.dt, self.dim, self.levels, xs, ss, cin, grid, None, None, nv.ptr(w), nv.ptr(bias), self._P(ws['feat']),
                C * _vox(dt), None, 1, N, dt[0], dt[1], dt[2], C, nv.stream())


class SegformerEngine(_Segformer, EncoderEngine):
    """The 16-bit (fp16 / bf16) Segformer forward with folded BatchNorm."""

    def __init__(self, dim=2, levels=4, base=32, cin=1, ncls=2, act_dtype=torch.float16, device='cuda', decoder_channels=256):
        EncoderEngine.__init__(self, dim, levels, base, cin, ncls, act_dtype, device)
        self._setup(decoder_channels)


class SegformerEngineF32(_Segformer, EncoderEngineF32):
    """The fp32 Segformer forward (planar fp32 activations, the f32-input matrix instruction): the default prediction form of a Segformer
    module, within the project's 1e-3 logit promise of the CPU fp32 path."""

    def __init__(self, dim=2, levels=4, base=32, cin=1, ncls=2, device='cuda', decoder_channels=256):
        EncoderEngineF32.__init__(self, dim, levels, base, cin, ncls, device)
        self._setup(decoder_channels)
