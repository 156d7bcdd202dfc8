// The decoders' implicit GEMMs (linknet.hip, deeplab.hip, segformer.hip), each skeleton once.  The operator is A (rows = output channels),
// gathered activations are B (columns = output voxels), so a lane's 4 accumulator rows are 4 consecutive channels of one voxel.  What
// differs between the architectures -- where B comes from, where the A column is, where the result goes, what the epilogue adds -- is a
// GATHER POLICY: a small struct that is the kernel's second parameter and a template argument of the kernel, so every hook is inlined
// and no skeleton branches at run time on its caller.  The policy's name is part of the kernel's name in a profile.
//
// Forward policies (16-bit and fp32 forward):
//   static in_vox / out_vox(D, H, W)          voxels per channel plane of the input / output tensor, from the column grid
//   a_row0(cls, co0, Cout), lda               first operator row of the workgroup, operator row length
//   A_PADDED, a_col(tap, c, k)                the operator column of k = (tap, channel c); padded rows need no bound check past K
//   src(tap, cls, d, h, w, D, H, W, cb)       the tap's source voxel on the input grid or -1 (zero); cb = its first input channel
//   dst(cls, d, h, w, r, D, H, W)             the column's output voxel
//   pre(v, n, co, Cout)                       the fp32 accumulator of channel co plus what enters before statistics / bias
//   extra<T>(ex[4], n, co, vout, ov), post(v, ex)   what channels co .. co + 3 get after bias + ReLU (16-bit, NHWC8c), and how
//   post32(v, n, co, vout, ov)                the same for one channel of the fp32 form (planar)
// Weight-gradient policies (LDS-staged kernel):
//   lane(k_l, k_ok)                           what is invariant per thread for its 8 operator columns k_l .. k_l + 7
//   column<T, ACT>(lane, n, r, D, H, W)       the 8 gathered B values of column (n, r)
#pragma once
#include "common.h"

namespace {

constexpr int GG_WAVES = 4;          // waves per workgroup of the forward GEMMs
constexpr int GG_COG = 64;           // output channels per workgroup (4 row tiles of 16 per wave)
constexpr int GG_LD = 40;            // LDS row stride (elements) of the weight gradient's [64][32] operand images

template <typename T>
__device__ __forceinline__ V8T<T> gg_zero8() {
  V8T<T> z;
#pragma unroll
  for (int j = 0; j < 8; ++j) z[j] = from_f32<T>(0.f);
  return z;
}

struct GgFwd {
  const void* x; long long x_ss;     // NHWC8c T, or planar fp32 [C][vox]; sample strides in elements
  void* y; long long y_ss;
  const void* wpk;
  const float* in_scale; const float* in_shift;   // optional relu(scale x + shift) on the way in (16-bit, ACT)
  const float* bias;
  float* stats;                      // [gridDim.z * gridDim.x][Cout][2] or null (16-bit, epi 0)
  int N, D, H, W;                    // the column grid
  int Cin, Cout, K;                  // K = taps * Cin
  long long cols;                    // columns per class = N * D * H * W
  int epi;                           // 0 raw (+ stats), 1 + bias + ReLU (16-bit; the fp32 form is always 1)
};

// grid (blocks, Cout / 64 rounded up, classes); 256 threads; each wave walks column tiles of 16 voxels.  K runs tap-major,
// channel-minor, so each 8-wide k group is one 16-byte load of one plane at one voxel.
template <typename T, bool ACT, typename G>
__global__ __launch_bounds__(256) void gg_fwd_kernel(GgFwd p, G pol) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cls = blockIdx.z, co0 = blockIdx.y * GG_COG;
  const int ntile = min(4, (p.Cout - co0) / 16);
  const T* x = (const T*)p.x;
  const T* wpk = (const T*)p.wpk + pol.a_row0(cls, co0, p.Cout) * pol.lda;
  const long long vin = G::in_vox(p.D, p.H, p.W), vout = G::out_vox(p.D, p.H, p.W), vgrid = (long long)p.D * p.H * p.W;
  const long long ntiles = (p.cols + 15) / 16;
  const long long per_block = (ntiles + gridDim.x - 1) / gridDim.x;
  const long long t0 = (long long)blockIdx.x * per_block, t1 = min(ntiles, t0 + per_block);
  float ssum[4][4], ssq[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) { ssum[a][r] = 0.f; ssq[a][r] = 0.f; }
  const int q = lane >> 4, l15 = lane & 15;
  for (long long tile = t0 + wave; tile < t1; tile += GG_WAVES) {
    const long long col = tile * 16 + l15;
    const bool ok = col < p.cols;
    const long long cc = ok ? col : 0;
    const int n = (int)(cc / vgrid);
    const long long r = cc - (long long)n * vgrid;
    const int w = (int)(r % p.W), h = (int)((r / p.W) % p.H), d = (int)(r / ((long long)p.W * p.H));
    const T* xs = x + (long long)n * p.x_ss;
    f32x4 acc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < p.K; k0 += 32) {
      const int kg = k0 + q * 8;
      const bool kok = kg < p.K;
      const int tap = kok ? kg / p.Cin : 0, c0 = kg - tap * p.Cin;
      const int acol = pol.a_col(tap, c0, kg);
      V8T<T> b = gg_zero8<T>();
      if (ok && kok) {
        int cb;
        const long long sv = pol.src(tap, cls, d, h, w, p.D, p.H, p.W, cb);
        if (sv >= 0) {
          b = *(const V8T<T>*)(xs + ((long long)((cb + c0) >> 3) * vin + sv) * 8);
          if constexpr (ACT) b = bn_relu8<T>(b, p.in_scale, p.in_shift, cb + c0);
        }
      }
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        if (a < ntile) {
          V8T<T> av = gg_zero8<T>();
          if (G::A_PADDED || kok) av = *(const V8T<T>*)(wpk + (long long)(a * 16 + l15) * pol.lda + acol);
          acc[a] = mfma16<T>(av, b, acc[a]);
        }
      }
    }
    if (!ok) continue;
    const long long ov = G::dst(cls, d, h, w, r, p.D, p.H, p.W);
    T* ys = (T*)p.y + (long long)n * p.y_ss;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      if (a >= ntile) continue;
      const int co = co0 + a * 16 + q * 4;
      // (pre ahead of ONE epi branch per row tile, the conversion inside the branches: the other orders of these statements cost
      // LinkNet's or DeepLabV3's instantiations an occupancy step, 110 -> 114 or 106 -> 132 VGPRs)
      typename Vec4<T>::type o;
      float v[4];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) v[rr] = pol.pre(acc[a][rr], n, co + rr, p.Cout);
      if (p.epi == 0) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          o[rr] = from_f32<T>(v[rr]);
          ssum[a][rr] += v[rr];
          ssq[a][rr] += v[rr] * v[rr];
        }
      } else {
        float ex[4] = {0.f, 0.f, 0.f, 0.f};
        pol.template extra<T>(ex, n, co, vout, ov);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) o[rr] = from_f32<T>(pol.post(fmaxf(v[rr] + p.bias[co + rr], 0.f), ex[rr]));
      }
      *(typename Vec4<T>::type*)(ys + ((long long)(co >> 3) * vout + ov) * 8 + (co & 7)) = o;
    }
  }
  if (p.stats == nullptr) return;
  // BatchNorm partial sums: the 16 columns of a lane group, then the 4 waves in a fixed order -> one row per workgroup
  __shared__ float red[GG_WAVES][GG_COG][2];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      float s = ssum[a][rr], s2 = ssq[a][rr];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) { s += __shfl_xor(s, o); s2 += __shfl_xor(s2, o); }
      if (l15 == 0) { red[wave][a * 16 + q * 4 + rr][0] = s; red[wave][a * 16 + q * 4 + rr][1] = s2; }
    }
  __syncthreads();
  if (threadIdx.x < 2 * ntile * 16) {
    const int c = threadIdx.x >> 1, which = threadIdx.x & 1;
    const float v = (red[0][c][which] + red[1][c][which]) + (red[2][c][which] + red[3][c][which]);
    p.stats[((long long)(blockIdx.z * gridDim.x + blockIdx.x) * p.Cout + co0 + c) * 2 + which] = v;
  }
}

// Workgroups along x: about 4 column tiles per wave at least, at most ~2048 workgroups per launch (a statistics row per workgroup);
// ngroups = row groups x classes
inline int gg_fwd_blocks(long long cols, int ngroups) {
  const long long tiles = (cols + 15) / 16;
  long long b = (tiles + 4 * GG_WAVES - 1) / (4 * GG_WAVES);
  const long long cap = (2048 + ngroups - 1) / ngroups;
  if (b > cap) b = cap;
  if (b > 1024) b = 1024;
  return (int)(b < 1 ? 1 : b);
}

// ---- fp32 form: planar fp32 [N][C][vox], v_mfma_f32_16x16x4_f32: A[row l&15][k l>>4], B[k l>>4][col l&15]; always + bias + ReLU.
// grid (column tiles / 4 rounded up, Cout / 64 rounded up, classes): one column tile per wave
template <typename G>
__global__ __launch_bounds__(256) void gg_f32_kernel(GgFwd p, G pol) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, l15 = lane & 15;
  const int cls = blockIdx.z, co0 = blockIdx.y * GG_COG;
  const int ntile = min(4, (p.Cout - co0) / 16);
  const float* wpk = (const float*)p.wpk + pol.a_row0(cls, co0, p.Cout) * pol.lda;
  const long long vin = G::in_vox(p.D, p.H, p.W), vout = G::out_vox(p.D, p.H, p.W), vgrid = (long long)p.D * p.H * p.W;
  const long long tile = (long long)blockIdx.x * GG_WAVES + wave;
  const long long col = tile * 16 + l15;
  const bool ok = col < p.cols;
  const long long cc = ok ? col : 0;
  const int n = (int)(cc / vgrid);
  const long long r = cc - (long long)n * vgrid;
  const int w = (int)(r % p.W), h = (int)((r / p.W) % p.H), d = (int)(r / ((long long)p.W * p.H));
  const float* xs = (const float*)p.x + (long long)n * p.x_ss;
  f32x4 acc[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
  int tap = 0, c = q;                        // k = k0 + q, walked incrementally (k0 += 4)
  while (c >= p.Cin) { c -= p.Cin; ++tap; }
  for (int k0 = 0; k0 < p.K; k0 += 4) {
    float b = 0.f;
    const bool kok = k0 + q < p.K;
    if (ok && kok) {
      int cb;
      const long long sv = pol.src(tap, cls, d, h, w, p.D, p.H, p.W, cb);
      if (sv >= 0) b = xs[(long long)(cb + c) * vin + sv];
    }
    const int acol = G::A_PADDED || kok ? pol.a_col(tap, c, k0 + q) : 0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
      if (a < ntile)
        acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(G::A_PADDED || kok ? wpk[(long long)(a * 16 + l15) * pol.lda + acol] : 0.f, b, acc[a], 0, 0, 0);
    c += 4;
    while (c >= p.Cin) { c -= p.Cin; ++tap; }
  }
  if (!ok) return;
  const long long ov = G::dst(cls, d, h, w, r, p.D, p.H, p.W);
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    if (a >= ntile) continue;
    const int co = co0 + a * 16 + q * 4;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {                   // one element at a time: four epilogues in flight cost an occupancy step
      const float v = fmaxf(pol.pre(acc[a][rr], n, co + rr, p.Cout) + p.bias[co + rr], 0.f);
      ((float*)p.y)[(long long)n * p.y_ss + (long long)(co + rr) * vout + ov] = pol.post32(v, n, co + rr, vout, ov);
    }
  }
}

// ---- weight gradient, staged through LDS: slab[split][Cout][K] = sum over the split's columns of dy[col][co] * B[col][k'].
// A workgroup owns a 64 (co) x 64 (k') tile; per chunk of 32 columns its 256 threads load dy (8 channels of one column each, 16 bytes)
// and the gathered B (8 k' of one column each), write both into LDS transposed to [row][column], and each wave runs the 16 x 64 x 32
// product with both operands read from LDS as 16-byte rows.  grid (splits, Cout / 64 rounded up, K / 64 rounded up)
struct GgWg {
  const void* dy; long long dy_ss;
  float* slab;
  int D, H, W;                       // the column grid
  int Cout, K;
  long long cols, chunks_per_split;
};

template <typename T, bool ACT, typename G>
__global__ __launch_bounds__(256) void gg_wgrad_kernel(GgWg p, G pol) {
  __shared__ __attribute__((aligned(16))) T sA[64 * GG_LD];
  __shared__ __attribute__((aligned(16))) T sB[64 * GG_LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, l15 = lane & 15;
  const int co0 = blockIdx.y * 64, kb = blockIdx.z * 64;
  const long long vgrid = (long long)p.D * p.H * p.W;
  const long long nchunks = (p.cols + 31) / 32;
  const long long c_lo = (long long)blockIdx.x * p.chunks_per_split, c_hi = min(nchunks, c_lo + p.chunks_per_split);
  const T* dy = (const T*)p.dy;
  // this thread's loads: group g = 8 rows, column jc
  const int g = threadIdx.x >> 5, jc = threadIdx.x & 31;
  const int co_l = co0 + g * 8;                       // dy rows co_l .. +8
  const int k_l = kb + g * 8;                         // B rows k_l .. +8
  const bool co_ok = co_l < p.Cout, k_ok = k_l < p.K;
  const auto ln = pol.lane(k_l, k_ok);
  f32x4 acc[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long long ck = c_lo; ck < c_hi; ++ck) {
    const long long col = ck * 32 + jc;
    V8T<T> va = gg_zero8<T>(), vb = gg_zero8<T>();
    if (col < p.cols) {
      const int n = (int)(col / vgrid);
      const long long r = col - (long long)n * vgrid;
      if (co_ok) va = *(const V8T<T>*)(dy + (long long)n * p.dy_ss + ((long long)(co_l >> 3) * vgrid + r) * 8);
      if (k_ok) vb = pol.template column<T, ACT>(ln, n, r, p.D, p.H, p.W);
    }
    __syncthreads();                                   // the previous chunk's operands are consumed
#pragma unroll
    for (int j = 0; j < 8; ++j) { sA[(g * 8 + j) * GG_LD + jc] = va[j]; sB[(g * 8 + j) * GG_LD + jc] = vb[j]; }
    __syncthreads();
    const V8T<T> a = *(const V8T<T>*)(sA + (wave * 16 + l15) * GG_LD + q * 8);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const V8T<T> b = *(const V8T<T>*)(sB + (t * 16 + l15) * GG_LD + q * 8);
      acc[t] = mfma16<T>(a, b, acc[t]);
    }
  }
  // D[row = co][col = k']: lane holds rows co0 + wave*16 + q*4 + rr at column kb + t*16 + l15
  float* out = p.slab + (long long)blockIdx.x * p.Cout * p.K;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int kk = kb + t * 16 + l15;
    if (kk >= p.K) continue;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int co = co0 + wave * 16 + q * 4 + rr;
      if (co < p.Cout) out[(long long)co * p.K + kk] = acc[t][rr];
    }
  }
}

inline int gg_wgrad_splits(long long cols, long long per_split_floats) {
  const long long nchunks = (cols + 31) / 32;
  long long s = (nchunks + 15) / 16;                  // at least 16 chunks (512 columns) per split
  if (s > 64) s = 64;
  if (s < 1) s = 1;
  while (s > 1 && s * per_split_floats > (8ll << 20)) s >>= 1;
  return (int)s;
}

}  // namespace
