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
// The forward GEMMs are gather_gemm.h's skeletons under the LkGather<ND, KIND> policy.
#include "common.h"
#include "gather_gemm.h"

namespace {

constexpr int LK_WAVES = 4;          // waves per workgroup of the weight gradient

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

// Output voxel of the column (d, h, w) (flat: r) of class cls: kind 1 scatters the classes over the 2x grid
template <int ND, int KIND>
__device__ __forceinline__ long long lk_dst(int cls, int d, int h, int w, long long r, int H, int W) {
  if constexpr (KIND == 1) {
    const int od = ND == 3 ? 2 * d + ((cls >> 2) & 1) : 0, oh = 2 * h + ((cls >> 1) & 1), ow = 2 * w + (cls & 1);
    return ((long long)od * (2 * H) + oh) * (2 * W) + ow;
  } else {
    return r;
  }
}

// gather_gemm.h policy of the three kinds.  (D, H, W) is the column grid: kind 0 the grid; kind 1 the input grid (the output is 2x);
// kind 2 the output grid (the input is 2x).  The operator is [class][Cout][lda = Kpad]; the eval epilogue adds the skip.
struct LkData {
  int lda;
  const void* skip; long long skip_ss;   // NHWC8c T (planar fp32 in the fp32 form) or null
};
template <int ND, int KIND>
struct LkGather : LkData {
  static constexpr bool A_PADDED = true;
  static __device__ __forceinline__ long long in_vox(int D, int H, int W) {
    return KIND == 2 ? (long long)(ND == 3 ? 2 * D : 1) * (2 * H) * (2 * W) : (long long)D * H * W;
  }
  static __device__ __forceinline__ long long out_vox(int D, int H, int W) {
    return KIND == 1 ? (long long)(ND == 3 ? 2 * D : 1) * (2 * H) * (2 * W) : (long long)D * H * W;
  }
  __device__ __forceinline__ long long a_row0(int cls, int co0, int Cout) const { return (long long)cls * Cout + co0; }
  __device__ __forceinline__ int a_col(int, int, int k) const { return k; }
  __device__ __forceinline__ long long src(int tap, int cls, int d, int h, int w, int D, int H, int W, int& cb) const {
    cb = 0;
    return lk_src<ND, KIND>(tap, cls, d, h, w, D, H, W);
  }
  static __device__ __forceinline__ long long dst(int cls, int d, int h, int w, long long r, int, int H, int W) {
    return lk_dst<ND, KIND>(cls, d, h, w, r, H, W);
  }
  __device__ __forceinline__ float pre(float v, int, int, int) const { return v; }
  template <typename T>
  __device__ __forceinline__ void extra(float (&sk)[4], int n, int co, long long vout, long long ov) const {
    if (skip == nullptr) return;
    const typename Vec4<T>::type sv = *(const typename Vec4<T>::type*)((const T*)skip + (long long)n * skip_ss +
                                                                       ((long long)(co >> 3) * vout + ov) * 8 + (co & 7));
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) sk[rr] = to_f32<T>(sv[rr]);
  }
  __device__ __forceinline__ float post(float v, float sk) const { return v + sk; }
  __device__ __forceinline__ float post32(float v, int n, int co, long long vout, long long ov) const {
    return skip != nullptr ? v + ((const float*)skip)[(long long)n * skip_ss + (long long)co * vout + ov] : v;
  }
};

int lk_fwd_blocks(int nd, int kind, int N, int D, int H, int W, int Cout) {
  return gg_fwd_blocks((long long)N * D * H * W, (Cout + GG_COG - 1) / GG_COG * lk_classes(nd, kind));
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
  const long long vout = LkGather<ND, KIND>::out_vox(p.D, p.H, p.W), vin = (long long)p.D * p.H * p.W;
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
      const long long ov = lk_dst<ND, KIND>(cls, d, h, w, r, p.H, p.W);
      av[j] = dy[(long long)n * p.dy_ss + ((long long)(co >> 3) * vout + ov) * 8 + (co & 7)];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        if (!kok[a]) continue;
        const long long sv = lk_src<ND, KIND>(tapk[a], cls, d, h, w, p.D, p.H, p.W);
        if (sv < 0) continue;
        const int c = chk[a];
        const T v = x[(long long)n * p.x_ss + ((long long)(c >> 3) * vin + sv) * 8 + (c & 7)];
        bv[a][j] = ACT ? bn_relu1<T>(v, p.in_scale, p.in_shift, c) : v;
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
    if (gamma != nullptr && (kind == 0 || kind == 2)) v = bn_fold_mul(v, bn_fold_scale(gamma, var, eps, row));
  }
  dst[i] = (OT)v;
  if (bias_out != nullptr && gamma != nullptr && cls == 0 && kk == 0 && (kind == 0 || kind == 2))
    bias_out[row] = bn_fold_bias(beta, mean, bn_fold_scale(gamma, var, eps, row), row);
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
  GgFwd p;
  p.x = x; p.x_ss = x_ss; p.y = y; p.y_ss = y_ss; p.wpk = wpk;
  p.in_scale = (const float*)in_scale; p.in_shift = (const float*)in_shift; p.bias = (const float*)bias; p.stats = (float*)stats;
  p.N = N; p.D = D; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.K = lk_taps(nd, kind) * Cin;
  p.cols = (long long)N * D * H * W; p.epi = epi;
  const LkData g{(int)lk_kpad(p.K), skip, skip_ss};
  const dim3 grid(lk_fwd_blocks(nd, kind, N, D, H, W, Cout), (Cout + GG_COG - 1) / GG_COG, lk_classes(nd, kind));
  iunet_dispatch(dtype, nd, in_scale != nullptr, [&](auto t, auto ndc, auto act) {
    auto launch = [&](auto pol) {
      hipLaunchKernelGGL((gg_fwd_kernel<decltype(t), act.value, decltype(pol)>), grid, dim3(256), 0, (hipStream_t)stream, p, pol);
    };
    if (kind == 0) launch(LkGather<ndc.value, 0>{g});
    else if (kind == 1) launch(LkGather<ndc.value, 1>{g});
    else if constexpr (!act.value) launch(LkGather<ndc.value, 2>{g});        // (checked above: kind 2 takes no input activation)
  });
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
  iunet_dispatch(dtype, nd, x_scale != nullptr, [&](auto t, auto ndc, auto act) {
    if (kind == 0) hipLaunchKernelGGL((lk_wgrad_kernel<decltype(t), ndc.value, 0, act.value>), grid, dim3(256), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((lk_wgrad_kernel<decltype(t), ndc.value, 1, act.value>), grid, dim3(256), 0, (hipStream_t)stream, p);
  });
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
  GgFwd p = {};
  p.x = x; p.x_ss = x_ss; p.y = y; p.y_ss = y_ss; p.wpk = wpk; p.bias = (const float*)bias;
  p.N = N; p.D = D; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.K = lk_taps(nd, kind) * Cin;
  p.cols = (long long)N * D * H * W; p.epi = 1;
  const LkData g{(int)lk_kpad(p.K), skip, skip_ss};
  const long long tiles = (p.cols + 15) / 16;
  const dim3 grid((unsigned)((tiles + GG_WAVES - 1) / GG_WAVES), (Cout + GG_COG - 1) / GG_COG, lk_classes(nd, kind));
#define LK32(NDV, KV) hipLaunchKernelGGL((gg_f32_kernel<LkGather<NDV, KV>>), grid, dim3(256), 0, (hipStream_t)stream, p, LkGather<NDV, KV>{g})
  if (nd == 3) { if (kind == 0) LK32(3, 0); else LK32(3, 1); } else { if (kind == 0) LK32(2, 0); else LK32(2, 1); }
#undef LK32
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

}  // extern "C"
