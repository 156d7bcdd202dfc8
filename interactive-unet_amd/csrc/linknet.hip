// LinkNet decoder blocks (Chaurasia & Culurciello 2017, smp's Linknet decoder on this project's encoder):
//   a1 = relu(bn1(conv1x1(D))), a2 = relu(bn2(convT_k4s2p1(a1))), D' = relu(bn3(conv1x1(a2))) + skip.
//
// Every product is one implicit GEMM on v_mfma_f32_16x16x32_{f16,bf16} (v_mfma_f32_16x16x4_f32 in the fp32 form) with the
// operator as A (rows = output channels) and the gathered activations as B (columns = output voxels), so a lane's 4 accumulator
// rows are 4 consecutive channels of one voxel: one 8-byte store into an NHWC8c plane.  Three gathers ("kinds"):
//   0  1x1 conv: K = Cin, the column's own voxel.
//   1  ConvTranspose k4 s2 p1: the output voxels split into 2^d parity classes; in class p an output voxel o = 2m + p has two
//      taps per axis (bit b: input m - b with kernel index 1 + 2b where p = 0, input m + b with kernel index 2 - 2b where p = 1),
//      K = 2^d Cin.  The operator is packed per class.
//   2  the data gradient of kind 1: the k4 s2 p1 strided conv over dy, dx[i] = sum_k dy[2i - 1 + k] W[.][.][k], K = 4^d Cout.
// K runs tap-major, channel-minor, so each 8-wide k group is one 16-byte load of one plane at one voxel.  The operator is packed
// [class][rows][Kpad] with Kpad = K rounded up to 32 (zeros), so A never needs a bound check.
#include "common.h"
#include "../../include/iunet.h"

namespace {

template <typename T> using V8T = typename Vec8<T>::type;
typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
template <typename T> struct Vec4;
template <> struct Vec4<f16> { typedef f16x4_t type; };
template <> struct Vec4<bf16> { typedef bf16x4_t type; };

constexpr int LK_WAVES = 4;          // waves per workgroup of the forward GEMM
constexpr int LK_COG = 64;           // output channels per workgroup (4 row tiles of 16 per wave)

inline int lk_taps(int nd, int kind) { return kind == 0 ? 1 : kind == 1 ? (1 << nd) : (1 << (2 * nd)); }
inline int lk_classes(int nd, int kind) { return kind == 1 ? (1 << nd) : 1; }
inline long long lk_kpad(long long K) { return (K + 31) / 32 * 32; }

struct Grid3 { int D, H, W; };

// Source voxel (on the input grid) of tap t for the output voxel (d, h, w) of class p; -1: outside (zero).
//   kind 0: the voxel itself; kind 1: (d, h, w) = m on the INPUT grid (D, H, W); kind 2: (d, h, w) on the output grid, input = 2x grid.
template <int ND, int KIND>
__device__ __forceinline__ long long lk_src(int t, int p, int d, int h, int w, int D, int H, int W) {
  if constexpr (KIND == 0) {
    return ((long long)d * H + h) * W + w;
  } else if constexpr (KIND == 1) {
    const int bw = t & 1, bh = (t >> 1) & 1, bd = (t >> 2) & 1;
    const int pw = p & 1, ph = (p >> 1) & 1, pd = (p >> 2) & 1;
    const int iw = w + (pw ? bw : -bw), ih = h + (ph ? bh : -bh), id = ND == 3 ? d + (pd ? bd : -bd) : 0;
    if (iw < 0 || iw >= W || ih < 0 || ih >= H || id < 0 || id >= D) return -1;
    return ((long long)id * H + ih) * W + iw;
  } else {
    const int kw = t & 3, kh = (t >> 2) & 3, kd = (t >> 4) & 3;
    const int W2 = 2 * W, H2 = 2 * H, D2 = ND == 3 ? 2 * D : 1;
    const int ow = 2 * w - 1 + kw, oh = 2 * h - 1 + kh, od = ND == 3 ? 2 * d - 1 + kd : 0;
    if (ow < 0 || ow >= W2 || oh < 0 || oh >= H2 || od < 0 || od >= D2) return -1;
    return ((long long)od * H2 + oh) * W2 + ow;
  }
}

// relu(scale * x + shift) rounded to T: the bits iunet_bn_relu_fwd stores
template <typename T>
__device__ __forceinline__ V8T<T> lk_act(V8T<T> v, const float* sc, const float* sh, int c0) {
  V8T<T> o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = from_f32<T>(fmaxf(fmaf(sc[c0 + j], to_f32<T>(v[j]), sh[c0 + j]), 0.f));
  return o;
}

struct LkFwd {
  const void* x; long long x_ss;
  void* y; long long y_ss;
  const void* wpk;
  const float* in_scale; const float* in_shift;
  const float* bias;
  const void* skip; long long skip_ss;
  float* stats;                   // [gridDim.z * gridDim.x][Cout][2] or null
  int N, D, H, W;                 // kind 0: the grid; kind 1: the input grid; kind 2: the output grid
  int Cin, Cout, K, Kpad;
  long long cols;                 // columns per class = N * D * H * W
  int epi;                        // 0 raw (+ stats), 1 + bias + ReLU (+ skip)
};

// grid (blocks, Cout / 64 rounded up, classes); 256 threads; each wave walks column tiles of 16 voxels
template <typename T, int ND, int KIND, bool ACT>
__global__ __launch_bounds__(256) void lk_fwd_kernel(LkFwd p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cls = blockIdx.z, co0 = blockIdx.y * LK_COG;
  const int ntile = min(4, (p.Cout - co0) / 16);
  const T* x = (const T*)p.x;
  const T* wpk = (const T*)p.wpk + ((long long)cls * p.Cout + co0) * p.Kpad;
  const int Din = KIND == 1 ? p.D : (KIND == 2 ? (ND == 3 ? 2 * p.D : 1) : p.D);
  const int Hin = KIND == 2 ? 2 * p.H : p.H, Win = KIND == 2 ? 2 * p.W : p.W;
  const long long vin = (long long)Din * Hin * Win;
  const int Dout = KIND == 1 ? (ND == 3 ? 2 * p.D : 1) : p.D, Hout = KIND == 1 ? 2 * p.H : p.H, Wout = KIND == 1 ? 2 * p.W : p.W;
  const long long vout = (long long)Dout * Hout * Wout, vgrid = (long long)p.D * p.H * p.W;
  const long long ntiles = (p.cols + 15) / 16;
  const long long per_block = (ntiles + gridDim.x - 1) / gridDim.x;
  const long long t0 = (long long)blockIdx.x * per_block, t1 = min(ntiles, t0 + per_block);
  float ssum[4][4], ssq[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) { ssum[a][r] = 0.f; ssq[a][r] = 0.f; }
  const int q = lane >> 4, l15 = lane & 15;
  for (long long tile = t0 + wave; tile < t1; tile += LK_WAVES) {
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
      V8T<T> b;
#pragma unroll
      for (int j = 0; j < 8; ++j) b[j] = from_f32<T>(0.f);
      if (ok && kg < p.K) {
        const int tap = kg / p.Cin, c0 = kg - tap * p.Cin;
        const long long sv = lk_src<ND, KIND>(tap, cls, d, h, w, p.D, p.H, p.W);
        if (sv >= 0) {
          b = *(const V8T<T>*)(xs + ((long long)(c0 >> 3) * vin + sv) * 8);
          if constexpr (ACT) b = lk_act<T>(b, p.in_scale, p.in_shift, c0);
        }
      }
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        if (a < ntile) {
          const V8T<T> av = *(const V8T<T>*)(wpk + (long long)(a * 16 + l15) * p.Kpad + kg);
          acc[a] = mfma16<T>(av, b, acc[a]);
        }
      }
    }
    if (!ok) continue;
    // output voxel of this column
    long long ov;
    if constexpr (KIND == 1) {
      const int od = ND == 3 ? 2 * d + ((cls >> 2) & 1) : 0, oh = 2 * h + ((cls >> 1) & 1), ow = 2 * w + (cls & 1);
      ov = ((long long)od * Hout + oh) * Wout + ow;
    } else {
      ov = r;
    }
    T* ys = (T*)p.y + (long long)n * p.y_ss;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      if (a >= ntile) continue;
      const int co = co0 + a * 16 + q * 4;
      typename Vec4<T>::type o;
      if (p.epi == 0) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          o[rr] = from_f32<T>(acc[a][rr]);
          ssum[a][rr] += acc[a][rr];
          ssq[a][rr] += acc[a][rr] * acc[a][rr];
        }
      } else {
        float sk[4] = {0.f, 0.f, 0.f, 0.f};
        if (p.skip != nullptr) {
          const typename Vec4<T>::type sv = *(const typename Vec4<T>::type*)((const T*)p.skip + (long long)n * p.skip_ss +
                                                                             ((long long)(co >> 3) * vout + ov) * 8 + (co & 7));
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) sk[rr] = to_f32<T>(sv[rr]);
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) o[rr] = from_f32<T>(fmaxf(acc[a][rr] + p.bias[co + rr], 0.f) + sk[rr]);
      }
      *(typename Vec4<T>::type*)(ys + ((long long)(co >> 3) * vout + ov) * 8 + (co & 7)) = o;
    }
  }
  if (p.stats == nullptr) return;
  // BatchNorm partial sums: the 16 columns of a lane group, then the 4 waves in a fixed order -> one row per workgroup
  __shared__ float red[LK_WAVES][LK_COG][2];
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

int lk_fwd_blocks(int nd, int kind, int N, int D, int H, int W, int Cout) {
  const long long cols = (long long)N * D * H * W;
  const long long tiles = (cols + 15) / 16;
  const int ncg = (Cout + LK_COG - 1) / LK_COG, ncls = lk_classes(nd, kind);
  // about 4 column tiles per wave at least, at most ~2048 workgroups per launch (a statistics row per workgroup and class)
  long long b = (tiles + 4 * LK_WAVES - 1) / (4 * LK_WAVES);
  const long long cap = (2048 + ncg * ncls - 1) / (ncg * ncls);
  if (b > cap) b = cap;
  if (b > 1024) b = 1024;
  return (int)(b < 1 ? 1 : b);
}

// ---- weight gradient: slab[class][split][Cout][K'] = sum over the split's columns of dy[col][co] * act(x)[k'][col]
struct LkWg {
  const void* x; long long x_ss;
  const void* dy; long long dy_ss;
  const float* in_scale; const float* in_shift;
  float* slab;
  int N, D, H, W;                 // kind 0: the grid; kind 1: the INPUT grid (dy on the 2x grid)
  int Cin, Cout, K;               // K = taps * Cin
  long long cols;
  int kgroups;                    // K / 64 rounded up
};

// grid (splits, (Cout / 16) * kgroups, classes); 256 threads: wave w takes the split's column steps w, w + 4, ..
template <typename T, int ND, int KIND, bool ACT>
__global__ __launch_bounds__(256) void lk_wgrad_kernel(LkWg p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, l15 = lane & 15;
  const int cls = blockIdx.z, mt = blockIdx.y / p.kgroups, kgp = blockIdx.y % p.kgroups;
  const int co = mt * 16 + l15;
  const int kb = kgp * 64;
  const int Dout = KIND == 1 ? (ND == 3 ? 2 * p.D : 1) : p.D, Hout = KIND == 1 ? 2 * p.H : p.H, Wout = KIND == 1 ? 2 * p.W : p.W;
  const long long vout = (long long)Dout * Hout * Wout, vin = (long long)p.D * p.H * p.W;
  const long long steps = (p.cols + 31) / 32;
  const long long per = (steps + gridDim.x - 1) / gridDim.x;
  const long long s0 = (long long)blockIdx.x * per, s1 = min(steps, s0 + per);
  const T* x = (const T*)p.x;
  const T* dy = (const T*)p.dy;
  // the B column of this lane: k' = kb + a * 16 + l15 -> tap, channel
  int tapk[4], chk[4];
  bool kok[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int kk = kb + a * 16 + l15;
    kok[a] = kk < p.K;
    tapk[a] = kok[a] ? kk / p.Cin : 0;
    chk[a] = kok[a] ? kk - tapk[a] * p.Cin : 0;
  }
  f32x4 acc[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long long st = s0 + wave; st < s1; st += LK_WAVES) {
    V8T<T> av;
    V8T<T> bv[4];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      av[j] = from_f32<T>(0.f);
#pragma unroll
      for (int a = 0; a < 4; ++a) bv[a][j] = from_f32<T>(0.f);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long long col = st * 32 + q * 8 + j;
      if (col >= p.cols) break;
      const int n = (int)(col / vin);
      const long long r = col - (long long)n * vin;
      const int w = (int)(r % p.W), h = (int)((r / p.W) % p.H), d = (int)(r / ((long long)p.W * p.H));
      long long ov = r;
      if constexpr (KIND == 1) {
        const int od = ND == 3 ? 2 * d + ((cls >> 2) & 1) : 0, oh = 2 * h + ((cls >> 1) & 1), ow = 2 * w + (cls & 1);
        ov = ((long long)od * Hout + oh) * Wout + ow;
      }
      av[j] = dy[(long long)n * p.dy_ss + ((long long)(co >> 3) * vout + ov) * 8 + (co & 7)];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        if (!kok[a]) continue;
        const long long sv = lk_src<ND, KIND>(tapk[a], cls, d, h, w, p.D, p.H, p.W);
        if (sv < 0) continue;
        const int c = chk[a];
        const T v = x[(long long)n * p.x_ss + ((long long)(c >> 3) * vin + sv) * 8 + (c & 7)];
        if constexpr (ACT) bv[a][j] = from_f32<T>(fmaxf(fmaf(p.in_scale[c], to_f32<T>(v), p.in_shift[c]), 0.f));
        else bv[a][j] = v;
      }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) acc[a] = mfma16<T>(av, bv[a], acc[a]);
  }
  // D[row = co][col = k']: lane holds rows mt*16 + q*4 + rr, column kb + a*16 + l15; the 4 waves meet in LDS in a fixed order
  __shared__ float red[LK_WAVES][16][64];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) red[wave][q * 4 + rr][a * 16 + l15] = acc[a][rr];
  __syncthreads();
  float* out = p.slab + ((long long)cls * gridDim.x + blockIdx.x) * p.Cout * p.K;
  for (int i = threadIdx.x; i < 16 * 64; i += 256) {
    const int row = i >> 6, c = i & 63;
    if (kb + c >= p.K) continue;
    const float v = (red[0][row][c] + red[1][row][c]) + (red[2][row][c] + red[3][row][c]);
    out[(long long)(mt * 16 + row) * p.K + kb + c] = v;
  }
}

int lk_wgrad_splits(int nd, int kind, int N, int D, int H, int W, int Cin, int Cout) {
  const long long cols = (long long)N * D * H * W;
  const int ncls = lk_classes(nd, kind);
  const long long K = (long long)lk_taps(nd, kind) * Cin;
  long long s = (cols + 2047) / 2048;
  if (s > 64) s = 64;
  if (s < 1) s = 1;
  while (s > 1 && (long long)ncls * s * Cout * K > (8ll << 20)) s >>= 1;
  return (int)s;
}

// dW = alpha * sum over splits (fixed order), scattered into the parameter's layout: kind 0 [Cout][Cin]; kind 1 [Cin][Cout][4^d]
template <int ND, int KIND>
__global__ __launch_bounds__(256) void lk_wgrad_reduce_kernel(const float* __restrict__ slab, int splits, int Cin, int Cout, float alpha,
                                                              float* __restrict__ dW) {
  const long long K = (long long)(KIND == 1 ? (1 << ND) : 1) * Cin;
  const long long per_cls = (long long)Cout * K;
  const long long total = per_cls * (KIND == 1 ? (1 << ND) : 1);
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int cls = (int)(i / per_cls);
  const long long e = i - cls * per_cls;
  float s = 0.f;
  for (int sp = 0; sp < splits; ++sp) s += slab[((long long)cls * splits + sp) * per_cls + e];
  const int co = (int)(e / K), kk = (int)(e - (long long)co * K);
  if constexpr (KIND == 0) {
    dW[(long long)co * Cin + kk] = alpha * s;
  } else {
    const int t = kk / Cin, ci = kk - t * Cin;
    const int bw = t & 1, bh = (t >> 1) & 1, bd = (t >> 2) & 1;
    const int pw = cls & 1, ph = (cls >> 1) & 1, pd = (cls >> 2) & 1;
    const int kw = pw ? 2 - 2 * bw : 1 + 2 * bw, kh = ph ? 2 - 2 * bh : 1 + 2 * bh, kd = pd ? 2 - 2 * bd : 1 + 2 * bd;
    const int kidx = ND == 3 ? (kd * 4 + kh) * 4 + kw : kh * 4 + kw;
    dW[((long long)ci * Cout + co) * (1 << (2 * ND)) + kidx] = alpha * s;
  }
}

// ---- operator packing
// kind 0: 1x1 forward, w [Cout][Cin] -> [Cout][Kpad(Cin)] (x BatchNorm scale); 1: 1x1 data gradient -> [Cin][Kpad(Cout)];
// 2: convT forward, w [Cin][Cout][4^d] -> [class][Cout][Kpad(2^d Cin)] (x scale); 3: convT data gradient -> [Cin][Kpad(4^d Cout)]
template <typename OT>
__global__ __launch_bounds__(256) void lk_pack_kernel(const float* __restrict__ w, const float* gamma, const float* beta, const float* mean,
                                                      const float* var, float eps, OT* __restrict__ dst, float* bias_out, int nd, int kind,
                                                      int Cout, int Cin, long long rows, long long K, long long Kpad, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long kk = i % Kpad, rowg = i / Kpad;
  const int row = (int)(rowg % rows), cls = (int)(rowg / rows);
  float v = 0.f;
  if (kk < K) {
    if (kind == 0) {
      v = w[(long long)row * Cin + kk];
    } else if (kind == 1) {
      v = w[kk * Cin + row];
    } else if (kind == 2) {
      const int t = (int)(kk / Cin), ci = (int)(kk - (long long)t * Cin);
      const int bw = t & 1, bh = (t >> 1) & 1, bd = (t >> 2) & 1;
      const int pw = cls & 1, ph = (cls >> 1) & 1, pd = (cls >> 2) & 1;
      const int kw = pw ? 2 - 2 * bw : 1 + 2 * bw, kh = ph ? 2 - 2 * bh : 1 + 2 * bh, kd = pd ? 2 - 2 * bd : 1 + 2 * bd;
      const int kidx = nd == 3 ? (kd * 4 + kh) * 4 + kw : kh * 4 + kw;
      v = w[((long long)ci * Cout + row) * (1 << (2 * nd)) + kidx];
    } else {
      const int t = (int)(kk / Cout), co = (int)(kk - (long long)t * Cout);
      v = w[((long long)row * Cout + co) * (1 << (2 * nd)) + t];
    }
    if (gamma != nullptr && (kind == 0 || kind == 2)) v *= gamma[row] / sqrtf(var[row] + eps);
  }
  dst[i] = (OT)v;
  if (bias_out != nullptr && gamma != nullptr && cls == 0 && kk == 0 && (kind == 0 || kind == 2)) {
    const float sc = gamma[row] / sqrtf(var[row] + eps);
    bias_out[row] = beta[row] - mean[row] * sc;
  }
}

// D = relu(scale * y + shift) + skip, the sum in fp32, one rounding
template <typename T>
__global__ __launch_bounds__(256) void lk_bn_relu_add_kernel(const T* __restrict__ y, long long y_ss, const T* __restrict__ skip, long long s_ss,
                                                             T* __restrict__ out, long long o_ss, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, long long vox) {
  const int pl = blockIdx.y, n = blockIdx.z;
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= vox) return;
  const long long off = ((long long)pl * vox + v) * 8;
  const V8T<T> a = *(const V8T<T>*)(y + n * y_ss + off);
  const V8T<T> b = *(const V8T<T>*)(skip + n * s_ss + off);
  V8T<T> o;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    o[j] = from_f32<T>(fmaxf(fmaf(scale[pl * 8 + j], to_f32<T>(a[j]), shift[pl * 8 + j]), 0.f) + to_f32<T>(b[j]));
  *(V8T<T>*)(out + n * o_ss + off) = o;
}

// ---- fp32 form: planar fp32 [N][C][vox] (sample strides in elements), v_mfma_f32_16x16x4_f32: A[row l&15][k l>>4], B[k l>>4][col l&15]
struct LkF32 {
  const float* x; long long x_ss;
  float* y; long long y_ss;
  const float* wpk; const float* bias;
  const float* skip; long long skip_ss;
  int D, H, W, Cin, Cout, K, Kpad;
  long long cols;
};

template <int ND, int KIND>
__global__ __launch_bounds__(256) void lk_f32_kernel(LkF32 p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, l15 = lane & 15;
  const int cls = blockIdx.z, co0 = blockIdx.y * LK_COG;
  const int ntile = min(4, (p.Cout - co0) / 16);
  const float* wpk = p.wpk + ((long long)cls * p.Cout + co0) * p.Kpad;
  const long long vin = (long long)p.D * p.H * p.W;
  const int Dout = KIND == 1 ? (ND == 3 ? 2 * p.D : 1) : p.D, Hout = KIND == 1 ? 2 * p.H : p.H, Wout = KIND == 1 ? 2 * p.W : p.W;
  const long long vout = (long long)Dout * Hout * Wout;
  const long long tile = (long long)blockIdx.x * LK_WAVES + wave;
  const long long col = tile * 16 + l15;
  const bool ok = col < p.cols;
  const long long cc = ok ? col : 0;
  const int n = (int)(cc / vin);
  const long long r = cc - (long long)n * vin;
  const int w = (int)(r % p.W), h = (int)((r / p.W) % p.H), d = (int)(r / ((long long)p.W * p.H));
  const float* xs = p.x + (long long)n * p.x_ss;
  f32x4 acc[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
  int tap = 0, c = q;                        // k = k0 + q, walked incrementally (k0 += 4)
  while (c >= p.Cin) { c -= p.Cin; ++tap; }
  for (int k0 = 0; k0 < p.K; k0 += 4) {
    float b = 0.f;
    if (ok && k0 + q < p.K) {
      const long long sv = lk_src<ND, KIND>(tap, cls, d, h, w, p.D, p.H, p.W);
      if (sv >= 0) b = xs[(long long)c * vin + sv];
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
      if (a < ntile) acc[a] = __builtin_amdgcn_mfma_f32_16x16x4f32(wpk[(long long)(a * 16 + l15) * p.Kpad + k0 + q], b, acc[a], 0, 0, 0);
    c += 4;
    while (c >= p.Cin) { c -= p.Cin; ++tap; }
  }
  if (!ok) return;
  long long ov = r;
  if constexpr (KIND == 1) {
    const int od = ND == 3 ? 2 * d + ((cls >> 2) & 1) : 0, oh = 2 * h + ((cls >> 1) & 1), ow = 2 * w + (cls & 1);
    ov = ((long long)od * Hout + oh) * Wout + ow;
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    if (a >= ntile) continue;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int co = co0 + a * 16 + q * 4 + rr;
      float v = fmaxf(acc[a][rr] + p.bias[co], 0.f);
      if (p.skip != nullptr) v += p.skip[(long long)n * p.skip_ss + (long long)co * vout + ov];
      p.y[(long long)n * p.y_ss + (long long)co * vout + ov] = v;
    }
  }
}

int lk_check(int nd, int kind, int N, int D, int H, int W, int Cin, int Cout) {
  IUNET_REQUIRE(nd == 2 || nd == 3, "linknet: nd must be 2 or 3, got %d", nd);
  IUNET_REQUIRE(kind >= 0 && kind <= 2, "linknet: kind must be 0, 1 or 2, got %d", kind);
  IUNET_REQUIRE_GRID("linknet", N, D, H, W);
  IUNET_REQUIRE(nd == 3 || D == 1, "linknet: 2-D tensors have D = 1");
  IUNET_REQUIRE(Cin > 0 && Cout > 0 && Cin % 16 == 0 && Cout % 16 == 0, "linknet: channel counts must be multiples of 16 (Cin %d, Cout %d)", Cin, Cout);
  return IUNET_OK;
}

}  // namespace

extern "C" {

long long iunet_lk_pack_elems(int nd, int kind, int Cout, int Cin) {
  if ((nd != 2 && nd != 3) || kind < 0 || kind > 3 || Cout <= 0 || Cin <= 0) return -1;
  const int taps = kind < 2 ? 1 : kind == 2 ? (1 << nd) : (1 << (2 * nd));
  const long long rows = kind == 1 || kind == 3 ? Cin : Cout;
  const long long K = (long long)taps * (kind == 1 || kind == 3 ? Cout : Cin);
  return (kind == 2 ? (1 << nd) : 1) * rows * lk_kpad(K);
}

int iunet_lk_pack(int dtype, int nd, int kind, const void* w, const void* gamma, const void* beta, const void* mean, const void* var,
                  float eps, void* dst, void* bias_out, int Cout, int Cin, void* stream) {
  IUNET_REQUIRE(dtype >= 0 && dtype <= 2, "lk_pack: dtype must be 0 (f16), 1 (bf16) or 2 (f32), got %d", dtype);
  const long long total = iunet_lk_pack_elems(nd, kind, Cout, Cin);
  IUNET_REQUIRE(total > 0, "lk_pack: bad arguments nd %d, kind %d, Cout %d, Cin %d", nd, kind, Cout, Cin);
  IUNET_REQUIRE(w && dst, "lk_pack: null pointer");
  IUNET_REQUIRE(!gamma || (beta && mean && var), "lk_pack: a BatchNorm fold needs gamma, beta, mean and var");
  const int taps = kind < 2 ? 1 : kind == 2 ? (1 << nd) : (1 << (2 * nd));
  const long long rows = kind == 1 || kind == 3 ? Cin : Cout;
  const long long K = (long long)taps * (kind == 1 || kind == 3 ? Cout : Cin);
  const dim3 grid((unsigned)((total + 255) / 256));
#define LKP(OT) hipLaunchKernelGGL(lk_pack_kernel<OT>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)w, (const float*)gamma, \
                                   (const float*)beta, (const float*)mean, (const float*)var, eps, (OT*)dst, (float*)bias_out, nd, kind, Cout, \
                                   Cin, rows, K, lk_kpad(K), total)
  if (dtype == 0) LKP(f16); else if (dtype == 1) LKP(bf16); else LKP(float);
#undef LKP
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_lk_stats_parts(int nd, int kind, int N, int D, int H, int W, int Cout) {
  if (lk_check(nd, kind, N, D, H, W, 16, Cout) != IUNET_OK) return IUNET_ERR_ARG;
  return lk_fwd_blocks(nd, kind, N, D, H, W, Cout) * lk_classes(nd, kind);
}

int iunet_lk_conv_fwd(int dtype, int nd, int kind, const void* x, long long x_ss, void* y, long long y_ss, const void* wpk,
                      const void* in_scale, const void* in_shift, const void* bias, const void* skip, long long skip_ss, void* stats, int epi,
                      int N, int D, int H, int W, int Cin, int Cout, void* stream) {
  IUNET_REQUIRE(dtype == 0 || dtype == 1, "lk_conv_fwd: dtype must be 0 (f16) or 1 (bf16), got %d", dtype);
  const int rc = lk_check(nd, kind, N, D, H, W, Cin, Cout);
  if (rc != IUNET_OK) return rc;
  IUNET_REQUIRE(x && y && wpk, "lk_conv_fwd: null pointer");
  IUNET_REQUIRE(epi == 0 || epi == 1, "lk_conv_fwd: epi must be 0 (raw) or 1 (+bias, ReLU), got %d", epi);
  IUNET_REQUIRE(epi == 0 || bias, "lk_conv_fwd: epi 1 needs a bias");
  IUNET_REQUIRE(epi == 1 || !skip, "lk_conv_fwd: a skip is added in the eval epilogue (epi 1) only");
  IUNET_REQUIRE(epi == 0 || !stats, "lk_conv_fwd: statistics are taken of the raw output (epi 0) only");
  IUNET_REQUIRE(!in_scale == !in_shift, "lk_conv_fwd: the input activation needs both scale and shift");
  IUNET_REQUIRE(kind != 2 || !in_scale, "lk_conv_fwd: the data gradient (kind 2) takes no input activation");
  LkFwd p;
  p.x = x; p.x_ss = x_ss; p.y = y; p.y_ss = y_ss; p.wpk = wpk;
  p.in_scale = (const float*)in_scale; p.in_shift = (const float*)in_shift; p.bias = (const float*)bias;
  p.skip = skip; p.skip_ss = skip_ss; p.stats = (float*)stats;
  p.N = N; p.D = D; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
  p.K = lk_taps(nd, kind) * Cin; p.Kpad = (int)lk_kpad(p.K);
  p.cols = (long long)N * D * H * W; p.epi = epi;
  const dim3 grid(lk_fwd_blocks(nd, kind, N, D, H, W, Cout), (Cout + LK_COG - 1) / LK_COG, lk_classes(nd, kind));
  const bool act = in_scale != nullptr;
#define LKF(TT, NDV, KV, AV) hipLaunchKernelGGL((lk_fwd_kernel<TT, NDV, KV, AV>), grid, dim3(256), 0, (hipStream_t)stream, p)
#define LKF_K(TT, NDV)                                                          \
  do {                                                                          \
    if (kind == 0) { if (act) LKF(TT, NDV, 0, true); else LKF(TT, NDV, 0, false); } \
    else if (kind == 1) { if (act) LKF(TT, NDV, 1, true); else LKF(TT, NDV, 1, false); } \
    else LKF(TT, NDV, 2, false);                                                \
  } while (0)
  if (dtype == 0) { if (nd == 3) LKF_K(f16, 3); else LKF_K(f16, 2); }
  else { if (nd == 3) LKF_K(bf16, 3); else LKF_K(bf16, 2); }
#undef LKF_K
#undef LKF
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

long long iunet_lk_wgrad_slab_floats(int nd, int kind, int N, int D, int H, int W, int Cin, int Cout) {
  if (lk_check(nd, kind, N, D, H, W, Cin, Cout) != IUNET_OK || kind == 2) return -1;
  return (long long)lk_classes(nd, kind) * lk_wgrad_splits(nd, kind, N, D, H, W, Cin, Cout) * Cout * lk_taps(nd, kind) * Cin;
}

int iunet_lk_wgrad(int dtype, int nd, int kind, const void* x, long long x_ss, const void* dy, long long dy_ss, const void* x_scale,
                   const void* x_shift, void* slab, void* dW, float alpha, int N, int D, int H, int W, int Cin, int Cout, void* stream) {
  IUNET_REQUIRE(dtype == 0 || dtype == 1, "lk_wgrad: dtype must be 0 (f16) or 1 (bf16), got %d", dtype);
  const int rc = lk_check(nd, kind, N, D, H, W, Cin, Cout);
  if (rc != IUNET_OK) return rc;
  IUNET_REQUIRE(kind == 0 || kind == 1, "lk_wgrad: kind must be 0 (1x1 conv) or 1 (k4 s2 p1 transposed conv), got %d", kind);
  IUNET_REQUIRE(x && dy && slab && dW, "lk_wgrad: null pointer");
  IUNET_REQUIRE(!x_scale == !x_shift, "lk_wgrad: the input activation needs both scale and shift");
  LkWg p;
  p.x = x; p.x_ss = x_ss; p.dy = dy; p.dy_ss = dy_ss;
  p.in_scale = (const float*)x_scale; p.in_shift = (const float*)x_shift; p.slab = (float*)slab;
  p.N = N; p.D = D; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout;
  p.K = lk_taps(nd, kind) * Cin; p.cols = (long long)N * D * H * W; p.kgroups = (p.K + 63) / 64;
  const int splits = lk_wgrad_splits(nd, kind, N, D, H, W, Cin, Cout), ncls = lk_classes(nd, kind);
  const dim3 grid(splits, (Cout / 16) * p.kgroups, ncls);
  const bool act = x_scale != nullptr;
#define LKW(TT, NDV, KV, AV) hipLaunchKernelGGL((lk_wgrad_kernel<TT, NDV, KV, AV>), grid, dim3(256), 0, (hipStream_t)stream, p)
#define LKW_K(TT, NDV)                                                          \
  do {                                                                          \
    if (kind == 0) { if (act) LKW(TT, NDV, 0, true); else LKW(TT, NDV, 0, false); } \
    else { if (act) LKW(TT, NDV, 1, true); else LKW(TT, NDV, 1, false); }      \
  } while (0)
  if (dtype == 0) { if (nd == 3) LKW_K(f16, 3); else LKW_K(f16, 2); }
  else { if (nd == 3) LKW_K(bf16, 3); else LKW_K(bf16, 2); }
#undef LKW_K
#undef LKW
  IUNET_CHECK_HIP(hipGetLastError());
  const long long total = (long long)ncls * Cout * p.K;
  const dim3 rg((unsigned)((total + 255) / 256));
#define LKR(NDV, KV) hipLaunchKernelGGL((lk_wgrad_reduce_kernel<NDV, KV>), rg, dim3(256), 0, (hipStream_t)stream, (const float*)slab, splits, Cin, Cout, alpha, (float*)dW)
  if (nd == 3) { if (kind == 0) LKR(3, 0); else LKR(3, 1); } else { if (kind == 0) LKR(2, 0); else LKR(2, 1); }
#undef LKR
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_lk_bn_relu_add(int dtype, const void* y, long long y_ss, const void* skip, long long skip_ss, void* out, long long out_ss,
                         const void* scale, const void* shift, int C, int N, long long vox, void* stream) {
  IUNET_REQUIRE(dtype == 0 || dtype == 1, "lk_bn_relu_add: dtype must be 0 (f16) or 1 (bf16), got %d", dtype);
  IUNET_REQUIRE(y && skip && out && scale && shift, "lk_bn_relu_add: null pointer");
  IUNET_REQUIRE(C > 0 && C % 8 == 0 && N > 0 && vox > 0, "lk_bn_relu_add: C %d (multiple of 8), N %d, %lld voxels", C, N, vox);
  const dim3 grid((unsigned)((vox + 255) / 256), C / 8, N);
  if (dtype == 0) hipLaunchKernelGGL(lk_bn_relu_add_kernel<f16>, grid, dim3(256), 0, (hipStream_t)stream, (const f16*)y, y_ss, (const f16*)skip, skip_ss, (f16*)out, out_ss, (const float*)scale, (const float*)shift, vox);
  else hipLaunchKernelGGL(lk_bn_relu_add_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)y, y_ss, (const bf16*)skip, skip_ss, (bf16*)out, out_ss, (const float*)scale, (const float*)shift, vox);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_lk_f32_conv_fwd(int nd, int kind, const void* x, long long x_ss, void* y, long long y_ss, const void* wpk, const void* bias,
                          const void* skip, long long skip_ss, int N, int D, int H, int W, int Cin, int Cout, void* stream) {
  const int rc = lk_check(nd, kind, N, D, H, W, Cin, Cout);
  if (rc != IUNET_OK) return rc;
  IUNET_REQUIRE(kind == 0 || kind == 1, "lk_f32_conv_fwd: kind must be 0 (1x1 conv) or 1 (k4 s2 p1 transposed conv), got %d", kind);
  IUNET_REQUIRE(x && y && wpk && bias, "lk_f32_conv_fwd: null pointer");
  LkF32 p;
  p.x = (const float*)x; p.x_ss = x_ss; p.y = (float*)y; p.y_ss = y_ss; p.wpk = (const float*)wpk; p.bias = (const float*)bias;
  p.skip = (const float*)skip; p.skip_ss = skip_ss;
  p.D = D; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.K = lk_taps(nd, kind) * Cin; p.Kpad = (int)lk_kpad(p.K);
  p.cols = (long long)N * D * H * W;
  const long long tiles = (p.cols + 15) / 16;
  const dim3 grid((unsigned)((tiles + LK_WAVES - 1) / LK_WAVES), (Cout + LK_COG - 1) / LK_COG, lk_classes(nd, kind));
#define LK32(NDV, KV) hipLaunchKernelGGL((lk_f32_kernel<NDV, KV>), grid, dim3(256), 0, (hipStream_t)stream, p)
  if (nd == 3) { if (kind == 0) LK32(3, 0); else LK32(3, 1); } else { if (kind == 0) LK32(2, 0); else LK32(2, 1); }
#undef LK32
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

}  // extern "C"
