// What the 2-D batch producer (augment.hip) and the 3-D patch producer (patch_augment.hip, section 18) share
// of their elastic, jitter, blur and noise pipelines, written once: the `use` bits, Philox, the word-to-uniform conversions, Box-Muller,
// the jitter of one value, the contrast mean, the LDS histogram, the elastic row pass and tile pass, and the entry points' common
// argument checks.  The definitions are tests/augment_ref.py and tests/patch_augment_ref.py: plain float32, every multiply and add
// rounded on its own -- every floating-point body below is under its own `fp contract(off)`, the pragma is lexical.
// Not here, because the two producers really differ: the finish kernels' blur (a 5 x 5 product table over bytes against three
// separable passes in a haloed tile), the 2-D integer map against the 3-D continuous displacement, the 2-D table T against the 3-D
// float image, and the block shapes of the two row kernels (256 x 1, 128 x 2).
#pragma once
#include <cstdio>
#include "common.h"

constexpr int AUG_ELASTIC = 1, AUG_JITTER = 2, AUG_BLUR = 4, AUG_NOISE = 8;      // the bits of `use` and of a descriptor's `flags`
constexpr int AUG_MAX_TAPS = 129;                // cap of the elastic Gaussian's K = int(8 sigma + 1) made odd: sigma up to 16; sizes the LDS arrays

// Philox4x32-10 at counter (c0, c1, c2, c3) under key (k0, k1): words 0 and 1 of the output.  32-bit integer arithmetic: exact.
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned& w0, unsigned& w1) {
  const unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned h0 = __umulhi(M0, c0), l0 = M0 * c0, h1 = __umulhi(M1, c2), l1 = M1 * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  w0 = c0; w1 = c1;
}

__device__ __forceinline__ int aug_reflect(int p, int n) {      // -1 -> 1, n -> n - 2: no edge repeat; needs |overhang| < n
  p = p < 0 ? -p : p;
  return p >= n ? 2 * n - 2 - p : p;
}
__device__ __forceinline__ float aug_clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// a Philox word's top 24 bits as a uniform: in [0, 1), and in (0, 1] for the logarithm's argument
__device__ __forceinline__ float aug_uniform(unsigned w) {
#pragma clang fp contract(off)
  return (float)(w >> 8) * 0x1p-24f;
}
__device__ __forceinline__ float aug_uniform_open(unsigned w) {
#pragma clang fp contract(off)
  return (float)((w >> 8) + 1u) * 0x1p-24f;
}

// Box-Muller's z from two Philox words, with the library's sqrtf / logf / cosf: their last-ulp differences from a correctly rounded
// pair are the one place an output may leave its definition, by one fp16 step
__device__ __forceinline__ float aug_gauss(unsigned w0, unsigned w1) {
#pragma clang fp contract(off)
  const float u1 = aug_uniform_open(w0), u2 = aug_uniform(w1);
  return sqrtf(-2.f * logf(u1)) * cosf(6.2831855f * u2);
}

// brightness and contrast of one value in drawn order, m: the contrast mean
__device__ __forceinline__ float aug_jitter(float x, float br, float co, bool contrast_first, float m) {
#pragma clang fp contract(off)
  if (contrast_first) return aug_clamp01(aug_clamp01(co * x + (1.f - co) * m) * br);
  const float t = aug_clamp01(x * br);
  return aug_clamp01(co * t + (1.f - co) * m);
}

// what enters the contrast step for a byte of value L = float32(v / 255): L itself, or its brightness step when brightness comes first
__device__ __forceinline__ float aug_entering(float L, float br, bool contrast_first) {
#pragma clang fp contract(off)
  return contrast_first ? L : aug_clamp01(L * br);
}

// The contrast mean of one jitter sample, by a block of 256 lanes, lane v = byte value v holding L = float32(v / 255): the exact one
// of the definition -- the products count[v] * entering[v] in float64 in parallel into `term` (LDS), summed by ONE lane in ascending v
// (a tree would round differently), divided by N, rounded to float32.  Lane 0 gets the mean, every other lane 0.
// Block-wide: one barrier.
__device__ __forceinline__ float aug_contrast_mean(const unsigned* counts, int v, float L, float br, bool contrast_first, long long N,
                                                   double* term) {
#pragma clang fp contract(off)
  term[v] = (double)counts[v] * (double)aug_entering(L, br, contrast_first);
  __syncthreads();
  float mean = 0.f;
  if (v == 0) {
    double acc = 0.0;
    for (int i = 0; i < 256; ++i) acc += term[i];
    mean = (float)(acc / (double)N);
  }
  return mean;
}

// A block's 256-bin histogram in LDS, lane `tid` of 256 owning bin `tid`: zeroed before the block counts into it with atomicAdd,
// then merged into the sample's 256 words with integer atomics (order-free).  Both calls are block-wide.
__device__ __forceinline__ void aug_hist_zero(unsigned* hist, int tid) {
  hist[tid] = 0;
  __syncthreads();
}
__device__ __forceinline__ void aug_hist_flush(const unsigned* hist, int tid, unsigned* sample_hist) {
  __syncthreads();
  const unsigned n = hist[tid];
  if (n) atomicAdd(&sample_hist[tid], n);
}

// Elastic, the pass along x of one row segment: LANES lanes share `line` (LDS, LANES + AUG_MAX_TAPS - 1 floats).  The noise 2u - 1
// of the segment's min(LANES, n - x0) positions from x0 plus r = K / 2 on each side (reflected in [0, n)) is generated once -- one Philox per
// value, counter (x, c1, c2, c3), not K per position -- and the lane's K taps are taken from there in ascending order.  Block-wide
// (one barrier inside; the caller places another before the line is filled again); `active`: the row exists.  Returns the sum for
// position x0 + lane, 0 where there is none.
template <int LANES>
__device__ __forceinline__ float aug_row_pass(float* line, int lane, bool active, int x0, int n, unsigned c1, unsigned c2, unsigned c3,
                                              unsigned k0, unsigned k1, const float* taps, int K) {
#pragma clang fp contract(off)
  const int r = K / 2, span = min(LANES, n - x0) + 2 * r;
  if (active)
    for (int t = lane; t < span; t += LANES) {
      unsigned w0, w1;
      philox4x32_10((unsigned)aug_reflect(x0 - r + t, n), c1, c2, c3, k0, k1, w0, w1);
      const float u = aug_uniform(w0);
      line[t] = 2.f * u - 1.f;
    }
  __syncthreads();
  float acc = 0.f;
  if (active && x0 + lane < n)
    for (int i = 0; i < K; ++i) acc += taps[i] * line[lane + i];
  return acc;
}

// Elastic, a pass along y or z (the axis: nA positions, sA elements apart) of one field: a block of 256 lanes takes a tile of 64
// positions along x by 32 along the axis; the tile plus r before and after (reflected) goes through `tile` (LDS) once, so a value is
// read from memory (32 + 2 r) / 32 times, not K times.  Lane (tx, ty) takes positions ty, ty + 4, ... of column tx; the taps run in
// ascending order.  src: the field's plane (the tile's position on the other axes included); what becomes of a sum is the caller's
// epilogue(q, oa, ox, acc), q = 0 .. 7 the lane's q-th position.  Block-wide: two barriers.
constexpr int AUG_TILE_X = 64, AUG_TILE_A = 32, AUG_TILE_LANES = 256;
constexpr int AUG_TILE_FLOATS = (AUG_TILE_A + AUG_MAX_TAPS - 1) * AUG_TILE_X;
template <typename Epilogue>
__device__ __forceinline__ void aug_tile_pass(float* tile, const float* src, int x0, int a0, int nX, int nA, long long sA, const float* taps,
                                              int K, Epilogue&& epilogue) {
#pragma clang fp contract(off)
  const int r = K / 2, rows = min(AUG_TILE_A, nA - a0) + 2 * r;
  const int tx = threadIdx.x & (AUG_TILE_X - 1), ty = threadIdx.x / AUG_TILE_X, ox = x0 + tx;
  for (int t = threadIdx.x; t < rows * AUG_TILE_X; t += AUG_TILE_LANES) {
    const int j = t / AUG_TILE_X, gx = x0 + (t & (AUG_TILE_X - 1));
    tile[t] = gx < nX ? src[aug_reflect(a0 - r + j, nA) * sA + gx] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < AUG_TILE_A / 4; ++q) {
    const int la = ty + 4 * q, oa = a0 + la;
    if (oa < nA && ox < nX) {
      float acc = 0.f;
      for (int i = 0; i < K; ++i) acc += taps[i] * tile[(la + i) * AUG_TILE_X + tx];
      epilogue(q, oa, ox, acc);
    }
  }
  __syncthreads();
}

inline long long aug_align256(long long v) { return (v + 255) & ~255LL; }      // the workspaces' parts start on 256 bytes

// The checks both extended entry points make before any launch.  who: the entry point's name; shape: its formatted output shape
// ("45 x 70 output"); side: the smallest extent; ws_fn: the function that answers the workspace's size; each: what the shape's numbers are ("side", "extent").
inline int aug_check_extra(const char* who, const char* shape, int use, const void* taps, int K, int side, long long ws_bytes,
                           long long ws_need, const char* ws_fn, const char* each) {
  IUNET_REQUIRE(use >= 0 && use <= (AUG_ELASTIC | AUG_JITTER | AUG_BLUR | AUG_NOISE), "%s: use %d (bits 1 elastic, 2 jitter, 4 blur, 8 noise)", who, use);
  IUNET_REQUIRE(ws_bytes >= ws_need, "%s: workspace of %lld bytes, %lld needed (%s)", who, ws_bytes, ws_need, ws_fn);
  if (use & AUG_ELASTIC) {
    IUNET_REQUIRE(taps, "%s: elastic without taps", who);
    IUNET_REQUIRE(K >= 1 && K <= AUG_MAX_TAPS && K % 2 == 1, "%s: %d elastic taps (odd, 1 .. %d)", who, K, AUG_MAX_TAPS);
    IUNET_REQUIRE(side > K / 2, "%s: a %s cannot reflect the elastic Gaussian's radius %d (every %s must exceed it)", who, shape, K / 2, each);
  }
  if (use & AUG_BLUR)
    IUNET_REQUIRE(side > 2, "%s: a %s cannot reflect the blur's radius 2 (every %s must exceed it)", who, shape, each);
  return IUNET_OK;
}
