// What the decoders share when they move a tensor from one grid to another, each written once: segformer.hip,
// upernet.hip, manet.hip and deeplab.hip include it.  Tensors are NHWC8c (f16 / bf16) or planar fp32 [N][C][vox] with sample strides in
// elements.  Every sum is fp32 in a fixed order with one rounding to the stored type: no float atomics, a repeated launch is bit-equal.
// These functions are the bit-for-bit contract of four architectures: an edit here changes all of them together, and must change none.
#pragma once
#include "common.h"

namespace {

// ---- channel-group access: the channels one thread moves (one 16-byte group of NHWC8c, one channel of planar fp32), as fp32.  A
// relu(scale x + shift) prologue on a loaded value is norm_z<T, true>(scale[c], v, shift[c]) of common.h: iunet_bn_relu_fwd's bits.
template <typename T> struct ChanGroup { static constexpr int G = 8; };
template <> struct ChanGroup<float> { static constexpr int G = 1; };

// the G channels of group g at voxel v of a tensor with vox voxels per plane (s: the sample's base)
template <typename T>
__device__ __forceinline__ void group_load(const T* s, int g, long long v, long long vox, float (&out)[ChanGroup<T>::G]) {
  if constexpr (std::is_same<T, float>::value) {
    out[0] = s[(long long)g * vox + v];
  } else {
    const V8T<T> b = *(const V8T<T>*)(s + ((long long)g * vox + v) * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = to_f32<T>(b[j]);
  }
}
template <typename T>
__device__ __forceinline__ void group_store(T* s, int g, long long v, long long vox, const float (&val)[ChanGroup<T>::G]) {
  if constexpr (std::is_same<T, float>::value) {
    s[(long long)g * vox + v] = val[0];
  } else {
    V8T<T> o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = from_f32<T>(val[j]);
    *(V8T<T>*)(s + ((long long)g * vox + v) * 8) = o;
  }
}

// ---- the source index of linear resampling: target index t on an axis of nout voxels reads source voxels i0 and i1 of nin with
// weights (1 - l1, l1).  Three rules, NOT interchangeable: each is the bits of the architecture that uses it.
struct ResampleAx {
  int i0, i1;
  float l1;
};

// Segformer (sf_gemm_kernel's gather, the SfResample weight-gradient policy, iunet_sf_adjoint).  PyTorch's upsample_linear with
// align_corners=False and an output size: src = max(0, (t + 0.5) nin / nout - 0.5), i0 = floor(src), i1 = i0 + (i0 < nin - 1),
// l1 = src - i0, evaluated in fp32 as PyTorch's kernel does.  It stays fp32: the integer rule below gives other bits on odd grids, and
// its 64-bit divisions do not fit sf_gemm_kernel's gather, which has no register headroom.
__device__ __forceinline__ ResampleAx resample_axis_f32(int t, int nout, int nin) {
  const float scale = (float)nin / (float)nout;
  float src = scale * ((float)t + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  ResampleAx a;
  a.i0 = min((int)src, nin - 1);
  a.i1 = a.i0 + (a.i0 < nin - 1 ? 1 : 0);
  a.l1 = src - (float)a.i0;
  return a;
}

// UPerNet (iunet_pn_resize, iunet_pn_resize_adjoint).  The same align_corners=False rule evaluated on the integers
// num = nin (2 t + 1) - nout, den = 2 nout: i0 = num / den, l1 = (num mod den) / den with ONE rounding, so the weights carry no
// cancellation error of an fp32 src (which grows with the index) and the forward and its adjoint use bit-identical weights.
__device__ __forceinline__ ResampleAx resample_axis_exact(int t, int nout, int nin) {
  const long long den = 2ll * nout;
  long long num = (long long)nin * (2 * t + 1) - nout;
  num = num < 0 ? 0 : num;
  ResampleAx a;
  a.i0 = min((int)(num / den), nin - 1);
  const long long rem = num - a.i0 * den;
  a.l1 = (float)rem / (float)den;
  a.i1 = (rem != 0 && a.i0 < nin - 1) ? a.i0 + 1 : a.i0;      // (a zero weight reads its own voxel again: the identity is a copy)
  return a;
}

// DeepLab's logit upsampling (dl_up_logits, dl_up_adjoint_kernel), align_corners=True: src = t (nin - 1) / (nout - 1), i0 = floor(src),
// i1 = min(i0 + 1, nin - 1), l1 = src - i0; an axis of one target voxel reads source 0.
__device__ __forceinline__ ResampleAx resample_axis_corners(int t, int nout, int nin) {
  const float sc = nout > 1 ? (float)(nin - 1) / (float)(nout - 1) : 0.f;
  const float src = sc * (float)t;
  ResampleAx a;
  a.i0 = min((int)src, nin - 1);
  a.i1 = min(a.i0 + 1, nin - 1);
  a.l1 = src - (float)a.i0;
  return a;
}

using ResampleRule = ResampleAx (*)(int t, int nout, int nin);

// ---- the 2^ND taps of one target voxel: f(source voxel offset, weight) in (d, h, w) order, d outermost, the weight built as wd, then
// wd * wh, then (wd * wh) * ww.  The caller sums fmaf(weight, value, acc) in that order.
template <int ND, typename F>
__device__ __forceinline__ void resample_taps(const ResampleAx& ad, const ResampleAx& ah, const ResampleAx& aw, int Hs, int Ws, F&& f) {
#pragma unroll
  for (int kd = 0; kd < (ND == 3 ? 2 : 1); ++kd) {
    const int id = ND == 3 ? (kd ? ad.i1 : ad.i0) : 0;
    const float wd = ND == 3 ? (kd ? ad.l1 : 1.f - ad.l1) : 1.f;
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      const int ih = kh ? ah.i1 : ah.i0;
      const float wh = wd * (kh ? ah.l1 : 1.f - ah.l1);
#pragma unroll
      for (int kw = 0; kw < 2; ++kw) {
        const int iw = kw ? aw.i1 : aw.i0;
        f(((long long)id * Hs + ih) * Ws + iw, wh * (kw ? aw.l1 : 1.f - aw.l1));
      }
    }
  }
}

// ---- the adjoint as a gather: dx[n][c][q] = [dx +] sum over target voxels t of w(t, q) u[n][c][t], w the product of the per-axis weights
// (a border sample whose two taps land on one voxel gives it both).
// The target indices whose taps can reach source index q: src(t) in (q - 1, q + 1), widened by one index on each side (the clamp at 0
// included); every candidate is re-tested by its weight
__device__ __forceinline__ void resample_adj_range(int q, int nin, int nout, int& lo, int& hi) {
  const float inv = (float)nout / (float)nin;
  lo = (int)floorf(((float)q - 0.5f) * inv - 0.5f) - 1;
  hi = (int)ceilf(((float)q + 1.5f) * inv - 0.5f) + 1;
  if (q <= 1) lo = 0;
  lo = max(lo, 0);
  hi = min(hi, nout - 1);
}
// candidate target indices per source index on one axis (resample_adj_range's extent, clamped to the axis)
inline long long pn_adj_extent(int nin, int nout) {
  const long long e = (2ll * nout + nin - 1) / nin + 3;
  return e < nout ? e : nout;
}

// the weight of target index t on source index q under Rule
template <ResampleRule Rule>
__device__ __forceinline__ float resample_adj_w(int t, int q, int nout, int nin) {
  const ResampleAx a = Rule(t, nout, nin);
  return (a.i0 == q ? 1.f - a.l1 : 0.f) + (a.i1 == q ? a.l1 : 0.f);
}

// One thread per (source voxel q, 8 channels): the candidates in (d, h, w) order, zero weights skipped.
template <typename T, int ND, ResampleRule Rule>
__global__ __launch_bounds__(256) void resample_adjoint_kernel(const T* __restrict__ u, long long u_ss, int Dt, int Ht, int Wt, T* dx, long long dx_ss,
                                                               int Ds, int Hs, int Ws, int C, int N, int accumulate) {
  const long long vs = (long long)Ds * Hs * Ws, vT = (long long)Dt * Ht * Wt;
  const long long total = (long long)N * (C / 8) * vs;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long r = i % vs;
  const int pl = (int)((i / vs) % (C / 8)), n = (int)(i / (vs * (C / 8)));
  const int qw = (int)(r % Ws), qh = (int)((r / Ws) % Hs), qd = (int)(r / ((long long)Ws * Hs));
  int dlo = 0, dhi = 0, hlo, hhi, wlo, whi;
  if (ND == 3) resample_adj_range(qd, Ds, Dt, dlo, dhi);
  resample_adj_range(qh, Hs, Ht, hlo, hhi);
  resample_adj_range(qw, Ws, Wt, wlo, whi);
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  const T* us = u + (long long)n * u_ss + (long long)pl * vT * 8;
  for (int td = dlo; td <= dhi; ++td) {
    const float wd = ND == 3 ? resample_adj_w<Rule>(td, qd, Dt, Ds) : 1.f;
    if (wd == 0.f) continue;
    for (int th = hlo; th <= hhi; ++th) {
      const float wh = resample_adj_w<Rule>(th, qh, Ht, Hs);
      if (wh == 0.f) continue;
      for (int tw = wlo; tw <= whi; ++tw) {
        const float ww = resample_adj_w<Rule>(tw, qw, Wt, Ws);
        if (ww == 0.f) continue;
        const float wgt = wd * wh * ww;
        const V8T<T> v = *(const V8T<T>*)(us + (((long long)td * Ht + th) * Wt + tw) * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaf(wgt, to_f32<T>(v[j]), acc[j]);
      }
    }
  }
  if (accumulate) {
    float old[8];
    group_load<T>(dx + (long long)n * dx_ss, pl, r, vs, old);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += old[j];
  }
  group_store<T>(dx + (long long)n * dx_ss, pl, r, vs, acc);
}

// The same adjoint where few source voxels each gather from many target voxels (UPerNet's pyramid branches: a 1 .. 6-bin grid under the
// bottleneck's): one workgroup per (source voxel, 8 channels), its 256 threads walk the candidate range, then a fixed-order reduction (xor
// tree in the wave, the four waves in order).  Another summation order than the narrow form's, so a caller picks between them from the
// grids alone (iunet_pn_resize_adjoint) or never (iunet_sf_adjoint).
template <typename T, int ND, ResampleRule Rule>
__global__ __launch_bounds__(256) void resample_adjoint_wide_kernel(const T* __restrict__ u, long long u_ss, int Dt, int Ht, int Wt, T* dx,
                                                                    long long dx_ss, int Ds, int Hs, int Ws, int C, int N, int accumulate) {
  const long long vs = (long long)Ds * Hs * Ws, vT = (long long)Dt * Ht * Wt;
  const long long i = blockIdx.x;
  const long long r = i % vs;
  const int pl = (int)((i / vs) % (C / 8)), n = (int)(i / (vs * (C / 8)));
  const int qw = (int)(r % Ws), qh = (int)((r / Ws) % Hs), qd = (int)(r / ((long long)Ws * Hs));
  int dlo = 0, dhi = 0, hlo, hhi, wlo, whi;
  if (ND == 3) resample_adj_range(qd, Ds, Dt, dlo, dhi);
  resample_adj_range(qh, Hs, Ht, hlo, hhi);
  resample_adj_range(qw, Ws, Wt, wlo, whi);
  const int ew = whi - wlo + 1, eh = hhi - hlo + 1, cnt = (dhi - dlo + 1) * eh * ew;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  const T* us = u + (long long)n * u_ss + (long long)pl * vT * 8;
  for (int e = threadIdx.x; e < cnt; e += 256) {
    const int tw = wlo + e % ew, th = hlo + (e / ew) % eh, td = dlo + e / (ew * eh);
    const float wgt = (ND == 3 ? resample_adj_w<Rule>(td, qd, Dt, Ds) : 1.f) * resample_adj_w<Rule>(th, qh, Ht, Hs) *
                      resample_adj_w<Rule>(tw, qw, Wt, Ws);
    if (wgt == 0.f) continue;
    const V8T<T> v = *(const V8T<T>*)(us + (((long long)td * Ht + th) * Wt + tw) * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = fmaf(wgt, to_f32<T>(v[j]), acc[j]);
  }
  __shared__ float red[4][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float s = wave_sum(acc[j]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][j] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  T* o = dx + (long long)n * dx_ss + ((long long)pl * vs + r) * 8;
  V8T<T> old;
  if (accumulate) old = *(const V8T<T>*)o;
  V8T<T> res;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float s = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
    if (accumulate) s += to_f32<T>(old[j]);
    res[j] = from_f32<T>(s);
  }
  *(V8T<T>*)o = res;
}

}  // namespace
