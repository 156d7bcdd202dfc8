// Per-voxel terms of the fused softmax + loss kernels, shared by the 1x1-head kernels (train_pointwise.hip) and the upsampled-logit
// kernels of DeepLabV3 (deeplab.hip), and the fixed-order block reductions they store their partial sums with.
//
// Forward: per class the 8 sums loss_finalize_kernel reads (0 sw, 1 swy, 2 swp, 3 swyp, 4 swy*log(p+eps), 5 sw*ry, 6 sw*rp,
// 7 sw*ry*rp).  Backward: dl = dloss / dlogit, from the per-class coefficients dL/dp = w*(A + B*y) - CE * w*y/(p+eps) through the
// softmax, times the loss scale.  Targets / weights: [N][ncls][vox] contiguous, f16 (tdtype 1) or f32 (tdtype 0).
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ float load_t(const void* p, long long off, int dt) {
  return dt == 0 ? ((const float*)p)[off] : (float)((const f16*)p)[off];
}

__device__ __forceinline__ float block_sum_256(float v, float* red /* [4] */) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// Block reduction of NV per-thread values with ONE barrier: wave shuffles, then 4 wave
// partials through LDS (lds: [4][NV] floats), thread i < NV writes out[i].  Fixed order.
template <int NV>
__device__ __forceinline__ void block_reduce_store(const float (&vals)[NV], float* lds, float* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const float v = wave_sum(vals[i]);
    if (lane == 0) lds[wave * NV + i] = v;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NV; i += 256) out[i] = lds[i] + lds[NV + i] + lds[2 * NV + i] + lds[3 * NV + i];
}

// softmax of the logits l of voxel v of sample n, and its loss sums added to acc
template <int NCLS>
__device__ __forceinline__ void loss_sums(const float (&l)[NCLS], const void* target, const void* weight, int tdtype, int n,
                                          long long vox, long long v, float (&acc)[NCLS][8]) {
  float mx = l[0];
#pragma unroll
  for (int c = 1; c < NCLS; ++c) mx = fmaxf(mx, l[c]);
  float e[NCLS], s = 0.f;
#pragma unroll
  for (int c = 0; c < NCLS; ++c) { e[c] = __expf(l[c] - mx); s += e[c]; }
  const float inv = 1.f / s;
#pragma unroll
  for (int c = 0; c < NCLS; ++c) {
    const float pr = e[c] * inv;
    const long long to = ((long long)n * NCLS + c) * vox + v;
    const float y = load_t(target, to, tdtype);
    const float w = weight ? load_t(weight, to, tdtype) : 1.f;
    const float ry = rintf(y), rp = rintf(pr);
    acc[c][0] += w; acc[c][1] += w * y; acc[c][2] += w * pr; acc[c][3] += w * y * pr;
    acc[c][4] += w * y * __logf(pr + 1e-12f);
    acc[c][5] += w * ry; acc[c][6] += w * rp; acc[c][7] += w * ry * rp;
  }
}

// softmax of the logits l of voxel v of sample n -> dl = lscale * dloss / dl (coef [ncls][3] of loss_finalize_kernel), also added to accb:
// the per-voxel statements of head_loss_bwd_kernel (which keeps its own copy: inlined there, this form schedules its fp32 ops differently)
template <int NCLS>
__device__ __forceinline__ void loss_grad(const float (&l)[NCLS], const void* target, const void* weight, int tdtype, const float* coef,
                                          int n, long long vox, long long v, float lscale, float (&dl)[NCLS], float (&accb)[NCLS]) {
  float mx = l[0];
#pragma unroll
  for (int c = 1; c < NCLS; ++c) mx = fmaxf(mx, l[c]);
  float e[NCLS], s = 0.f;
#pragma unroll
  for (int c = 0; c < NCLS; ++c) { e[c] = __expf(l[c] - mx); s += e[c]; }
  const float inv = 1.f / s;
  float g[NCLS], dot = 0.f;
#pragma unroll
  for (int c = 0; c < NCLS; ++c) {
    const float pr = e[c] * inv;
    const long long to = ((long long)n * NCLS + c) * vox + v;
    const float y = load_t(target, to, tdtype);
    const float w = weight ? load_t(weight, to, tdtype) : 1.f;
    g[c] = w * (coef[c * 3] + coef[c * 3 + 1] * y) - coef[c * 3 + 2] * w * y / (pr + 1e-12f);
    e[c] = pr;
    dot += g[c] * pr;
  }
#pragma unroll
  for (int c = 0; c < NCLS; ++c) { dl[c] = e[c] * (g[c] - dot) * lscale; accb[c] += dl[c]; }   // softmax backward
}

}  // namespace
