// DeepLabV3 decoder (Chen et al. 2017, smp's DeepLabV3Decoder on this project's encoder), on the encoder's coarsest grid:
//   ASPP: b0 = relu(bn(conv1x1(X))), b_k = relu(bn(conv3^d dilation r_k (X))) (k = 1..3), bp = relu(bn(conv1x1(mean(X)))) broadcast;
//   P = relu(bn(conv1x1_{5C -> C}(concat[b0, b1, b2, b3, bp]))), A = dropout(P), F = relu(bn(conv3^d(A))), logits_c = head(F);
//   logits = upsample x s (bilinear / trilinear, align_corners=True), softmax.
//
// Products are implicit GEMMs on v_mfma_f32_16x16x32_{f16,bf16} (v_mfma_f32_16x16x4_f32 in the fp32 form) as in linknet.hip: the operator
// is A (rows = output channels), gathered activations are B (columns = output voxels).  The gather is a list of TAPS built at launch:
// tap t reads input channels [cb_t, cb_t + Cin) at the voxel offset (dd, dh, dw)_t and meets operator columns [col_t, col_t + Cin).  A
// dilated 3^d conv of rate r keeps the taps whose offset (k - 1) r satisfies |(k - 1) r| < E on every axis of extent E (the others only
// ever read zero padding); rate 0 denotes a 1x1 conv.  K runs over the kept taps only, so at 16^3 a rate-24 conv is a 1x1 GEMM.  A data
// gradient is the same gather with the flipped operator, and the ASPP's data gradient is ONE launch over four branches' taps (channel
// bases = the four slots of the branch-gradient buffer, operator columns = the four branches' packed operators side by side).
// Operators are packed per weight with all ksz^d taps ([rows][ksz^d * Cin], tap-major, channel-minor); no padding is read: a lane whose
// k is past the kept K loads zeros for both operands.
//
// Per-sample bias: the pooling branch is constant over space, so W_proj[:, 4C:5C] bp[n] enters the projection as a per-sample bias
// [N][Cout] added to the fp32 accumulator (the projection reads only the four spatial slots, K = 4C).  The same epilogue adds the pooling
// branch's adjoint dmean[n][c] / vox to the ASPP data gradient: one fp32 sum, one rounding.
//
// All reductions are fixed-order (per-workgroup slabs, then ordered sums): no float atomics, two identical calls are bit-identical.
//
// The GEMMs are gather_gemm.h's skeletons under the DlFwdGather / DlWgGather policies (segformer.hip calls the forward for M^T dZ).
#include "common.h"
#include "gather_gemm.h"
#include "head_out.h"
#include "loss_terms.h"
#include "resample.h"

namespace {

constexpr int DL_MAXT = 96;          // taps per launch (the 3-D ASPP data gradient: 1 + 3 x 27)
constexpr int DL_MAXBR = 4;          // branches per launch

struct DlTaps {
  int n;
  int cb[DL_MAXT], col[DL_MAXT];
  short od[DL_MAXT], oh[DL_MAXT], ow[DL_MAXT];
};

// Appends the kept taps of one conv (rate 0: 1x1) over the grid D x H x W.  The 3^d kernel index of a tap is (kd * 3 + kh) * 3 + kw (2-D:
// kh * 3 + kw), its operator columns start at colbase + kidx * Cin.  Returns false if the table overflows.
bool dl_add_taps(DlTaps& t, int nd, int rate, int D, int H, int W, int cbase, int colbase, int Cin) {
  if (rate == 0) {
    if (t.n >= DL_MAXT) return false;
    t.cb[t.n] = cbase; t.col[t.n] = colbase; t.od[t.n] = t.oh[t.n] = t.ow[t.n] = 0; ++t.n;
    return true;
  }
  for (int kd = 0; kd < (nd == 3 ? 3 : 1); ++kd)
    for (int kh = 0; kh < 3; ++kh)
      for (int kw = 0; kw < 3; ++kw) {
        const long long od = nd == 3 ? (long long)(kd - 1) * rate : 0, oh = (long long)(kh - 1) * rate, ow = (long long)(kw - 1) * rate;
        if (od <= -D || od >= D || oh <= -H || oh >= H || ow <= -W || ow >= W) continue;
        if (t.n >= DL_MAXT) return false;
        const int kidx = nd == 3 ? (kd * 3 + kh) * 3 + kw : kh * 3 + kw;
        t.cb[t.n] = cbase; t.col[t.n] = colbase + kidx * Cin;
        t.od[t.n] = (short)od; t.oh[t.n] = (short)oh; t.ow[t.n] = (short)ow;
        ++t.n;
      }
  return true;
}

// Source voxel of tap t for the column (d, h, w), -1: outside (zero)
__device__ __forceinline__ long long dl_tap_src(const DlTaps& t, int tap, int d, int h, int w, int D, int H, int W) {
  const int sd = d + t.od[tap], sh = h + t.oh[tap], sw = w + t.ow[tap];
  if (sd < 0 || sd >= D || sh < 0 || sh >= H || sw < 0 || sw >= W) return -1;
  return ((long long)sd * H + sh) * W + sw;
}

// gather_gemm.h forward policy: one class, input and output on the column grid, operator [Cout][lda = Kw] without padding, a per-sample
// bias [N][Cout] (x psb_scale) or null added to the accumulator
struct DlFwdGather {
  int lda;
  const float* psb; float psb_scale;
  DlTaps taps;
  static constexpr bool A_PADDED = false;
  static __device__ __forceinline__ long long in_vox(int D, int H, int W) { return (long long)D * H * W; }
  static __device__ __forceinline__ long long out_vox(int D, int H, int W) { return (long long)D * H * W; }
  __device__ __forceinline__ long long a_row0(int, int co0, int) const { return co0; }
  __device__ __forceinline__ int a_col(int tap, int c, int) const { return taps.col[tap] + c; }
  __device__ __forceinline__ long long src(int tap, int, int d, int h, int w, int D, int H, int W, int& cb) const {
    cb = taps.cb[tap];
    return dl_tap_src(taps, tap, d, h, w, D, H, W);
  }
  static __device__ __forceinline__ long long dst(int, int, int, int, long long r, int, int, int) { return r; }
  __device__ __forceinline__ float pre(float v, int n, int co, int Cout) const {
    return psb != nullptr ? v + psb[(long long)n * Cout + co] * psb_scale : v;
  }
  template <typename T>
  __device__ __forceinline__ void extra(float (&)[4], int, int, long long, long long) const {}
  __device__ __forceinline__ float post(float v, float) const { return v; }
  __device__ __forceinline__ float post32(float v, int, int, long long, long long) const { return v; }
};

int dl_fwd_blocks(int N, int D, int H, int W, int Cout) { return gg_fwd_blocks((long long)N * D * H * W, (Cout + GG_COG - 1) / GG_COG); }

// gather_gemm.h weight-gradient policy: B[k' = (tap, ci)] = act(x)[cb_tap + ci] at the tap-shifted voxel
struct DlWgGather {
  const void* x; long long x_ss;
  const float* in_scale; const float* in_shift;
  int Cin;
  DlTaps taps;
  struct Lane { int tap, ch; };
  __device__ __forceinline__ Lane lane(int k_l, bool k_ok) const {      // one tap: Cin is a multiple of 8
    const int tap = k_ok ? k_l / Cin : 0;
    return Lane{tap, taps.cb[tap] + k_l - tap * Cin};
  }
  template <typename T, bool ACT>
  __device__ __forceinline__ V8T<T> column(const Lane& l, int n, long long r, int D, int H, int W) const {
    const int w = (int)(r % W), h = (int)((r / W) % H), d = (int)(r / ((long long)W * H));
    const long long sv = dl_tap_src(taps, l.tap, d, h, w, D, H, W);
    if (sv < 0) return gg_zero8<T>();
    const V8T<T> v = *(const V8T<T>*)((const T*)x + (long long)n * x_ss + ((long long)(l.ch >> 3) * ((long long)D * H * W) + sv) * 8);
    return ACT ? bn_relu8<T>(v, in_scale, in_shift, l.ch) : v;
  }
};


// dW[co][ci_off + ci][kidx] = alpha * sum over splits (fixed order) of the kept taps' columns; a pruned tap's gradient is zero
__global__ __launch_bounds__(256) void dl_wgrad_reduce_kernel(const float* __restrict__ slab, int splits, int Cin, int Cout, int K, int kvol,
                                                              float alpha,
                                                              float* __restrict__ dW, int Cin_tot, int ci_off, DlTaps taps) {
  const long long total = (long long)Cout * Cin * kvol;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int kidx = (int)(i % kvol), ci = (int)((i / kvol) % Cin), co = (int)(i / ((long long)kvol * Cin));
  int t = -1;
  for (int u = 0; u < taps.n; ++u)
    if (taps.col[u] == kidx * Cin) { t = u; break; }
  float s = 0.f;
  if (t >= 0) {
    const long long e = (long long)co * K + (long long)t * Cin + ci;
    for (int sp = 0; sp < splits; ++sp) s += slab[(long long)sp * Cout * K + e];
  }
  dW[((long long)co * Cin_tot + ci_off + ci) * kvol + kidx] = alpha * s;
}

// ---- operator packing: w [Cout][Cin_tot][ksz^d] fp32 (channels ci_off .. ci_off + Cin of it).
// mode 0 (forward): dst[co][k_off + kidx * Cin + ci] = w[co][ci_off + ci][kidx] (x the BatchNorm fold where gamma is given, bias_out = beta -
// mean * scale); mode 1 (data gradient): dst[ci][k_off + kidx * Cout + co] = w[co][ci_off + ci][kvol - 1 - kidx] (the flipped kernel).
template <typename OT>
__global__ __launch_bounds__(256) void dl_pack_kernel(const float* __restrict__ w, const float* gamma, const float* beta, const float* mean,
                                                      const float* var, float eps, OT* __restrict__ dst, float* bias_out, int mode, int kvol,
                                                      int Cout, int Cin, int Cin_tot, int ci_off, int k_off, int ld) {
  const long long total = (long long)Cout * Cin * kvol;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int kidx = (int)(i % kvol), ci = (int)((i / kvol) % Cin), co = (int)(i / ((long long)kvol * Cin));
  float v = w[((long long)co * Cin_tot + ci_off + ci) * kvol + kidx];
  if (mode == 0) {
    if (gamma != nullptr) v = bn_fold_mul(v, bn_fold_scale(gamma, var, eps, co));
    dst[(long long)co * ld + k_off + (long long)kidx * Cin + ci] = (OT)v;
    if (bias_out != nullptr && gamma != nullptr && ci == 0 && kidx == 0) bias_out[co] = bn_fold_bias(beta, mean, bn_fold_scale(gamma, var, eps, co), co);
  } else {
    dst[(long long)ci * ld + k_off + (long long)(kvol - 1 - kidx) * Cout + co] = (OT)v;
  }
}

// ---- pooling branch
// out[n][c] = scale * sum over the grid of x[n][c]: NHWC8c T (one workgroup per (plane, n), 8 channels per thread) or planar fp32
template <typename T>
__global__ __launch_bounds__(256) void dl_chansum_kernel(const T* __restrict__ x, long long x_ss, float* __restrict__ out, float scale, int C,
                                                         long long vox) {
  const int pl = blockIdx.x, n = blockIdx.y;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  const T* xs = x + (long long)n * x_ss + (long long)pl * vox * 8;
  for (long long v = threadIdx.x; v < vox; v += 256) {
    const V8T<T> a = *(const V8T<T>*)(xs + v * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += to_f32<T>(a[j]);
  }
  __shared__ float red[4 * 8];
  __shared__ float tot[8];
  block_reduce_store<8>(acc, red, tot);
  __syncthreads();
  if (threadIdx.x < 8) out[(long long)n * C + pl * 8 + threadIdx.x] = tot[threadIdx.x] * scale;
}

__global__ __launch_bounds__(256) void dl_chansum_f32_kernel(const float* __restrict__ x, long long x_ss, float* __restrict__ out, float scale,
                                                             int C, long long vox) {
  const int c = blockIdx.x, n = blockIdx.y;
  const float* xs = x + (long long)n * x_ss + (long long)c * vox;
  float acc = 0.f;
  for (long long v = threadIdx.x; v < vox; v += 256) acc += xs[v];
  __shared__ float red[4];
  const float s = block_sum_256(acc, red);
  if (threadIdx.x == 0) out[(long long)n * C + c] = s * scale;
}

// ypool[n][co] = sum_ci Wpool[co][ci] mean[n][ci]; stats[n][co] = (y, y^2) rows for iunet_bn_finalize (count N)
__global__ __launch_bounds__(256) void dl_pool_gemv_kernel(const float* __restrict__ mean, const float* __restrict__ wp, float* __restrict__ ypool,
                                                           float* stats, int N, int Cb, int C) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N * C) return;
  const int n = i / C, co = i - n * C;
  float s = 0.f;
  for (int ci = 0; ci < Cb; ++ci) s = fmaf(wp[(long long)co * Cb + ci], mean[(long long)n * Cb + ci], s);
  ypool[i] = s;
  if (stats != nullptr) { stats[(long long)i * 2] = s; stats[(long long)i * 2 + 1] = s * s; }
}

// bp[n][j] = relu(scale[j] ypool[n][j] + shift[j]) (scale / shift: the batch statistics' (training) or folded from the running statistics
// (eval, scale == null)); psb[n][c] = fold_c * sum_j Wproj[c][4C + j] bp[n][j], fold_c = the projection's eval BatchNorm scale or 1
__global__ __launch_bounds__(256) void dl_pool_bp_kernel(const float* __restrict__ ypool, const float* scale, const float* shift, const float* gamma,
                                                         const float* beta, const float* rmean, const float* rvar, float eps, float* __restrict__ bp,
                                                         int N, int C) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N * C) return;
  const int j = i % C;
  float sc, sh;
  if (scale != nullptr) { sc = scale[j]; sh = shift[j]; }
  else { sc = bn_fold_scale(gamma, rvar, eps, j); sh = bn_fold_bias(beta, rmean, sc, j); }
  bp[i] = fmaxf(fmaf(sc, ypool[i], sh), 0.f);
}

__global__ __launch_bounds__(256) void dl_pool_psb_kernel(const float* __restrict__ bp, const float* __restrict__ wproj, const float* pgamma,
                                                          const float* pvar, float eps, float* __restrict__ psb, int N, int C) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N * C) return;
  const int n = i / C, c = i - n * C;
  float s = 0.f;
  for (int j = 0; j < C; ++j) s = fmaf(wproj[(long long)c * 5 * C + 4 * C + j], bp[(long long)n * C + j], s);
  if (pgamma != nullptr) s = bn_fold_mul(s, bn_fold_scale(pgamma, pvar, eps, c));
  psb[i] = s;
}

// backward, from dpsb[n][c] = sum over the grid of the projection's raw-output gradient:
//   dWproj[c][4C + j] = sum_n dpsb[n][c] bp[n][j]; dbp[n][j] = sum_c Wproj[c][4C + j] dpsb[n][c]
__global__ __launch_bounds__(256) void dl_pool_bwd1_kernel(const float* __restrict__ dpsb, const float* __restrict__ bp, const float* __restrict__ wproj,
                                                           float* __restrict__ dwproj, float* __restrict__ dbp, int N, int C) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < (long long)C * C) {
    const int c = (int)(i / C), j = (int)(i - (long long)c * C);
    float s = 0.f;
    for (int n = 0; n < N; ++n) s = fmaf(dpsb[(long long)n * C + c], bp[(long long)n * C + j], s);
    dwproj[(long long)c * 5 * C + 4 * C + j] = s;
  }
  if (i < (long long)N * C) {
    const int n = (int)(i / C), j = (int)(i - (long long)n * C);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s = fmaf(wproj[(long long)c * 5 * C + 4 * C + j], dpsb[(long long)n * C + c], s);
    dbp[i] = s;
  }
}

// BatchNorm (batch statistics over N) + ReLU backward of the pooling branch, one thread per channel: dy[n][j], dgamma, dbeta
__global__ __launch_bounds__(256) void dl_pool_bwd2_kernel(const float* __restrict__ dbp, const float* __restrict__ bp, const float* __restrict__ ypool,
                                                           const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dy, int N, int C) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= C) return;
  float sb = 0.f, sg = 0.f;
  for (int n = 0; n < N; ++n) {
    const long long i = (long long)n * C + j;
    const float d = bp[i] > 0.f ? dbp[i] : 0.f;
    sb += d;
    sg += d * (ypool[i] - mean[j]) * invstd[j];
  }
  dgamma[j] = sg;
  dbeta[j] = sb;
  const float k = gamma[j] * invstd[j], inv_n = 1.f / (float)N;
  for (int n = 0; n < N; ++n) {
    const long long i = (long long)n * C + j;
    const float d = bp[i] > 0.f ? dbp[i] : 0.f;
    const float xh = (ypool[i] - mean[j]) * invstd[j];
    dy[i] = k * (d - sb * inv_n - xh * sg * inv_n);
  }
}

// dWpool[j][ci] = sum_n dy[n][j] mean[n][ci]; dmean[n][ci] = sum_j Wpool[j][ci] dy[n][j]
__global__ __launch_bounds__(256) void dl_pool_bwd3_kernel(const float* __restrict__ dy, const float* __restrict__ mean, const float* __restrict__ wpool,
                                                           float* __restrict__ dwpool, float* __restrict__ dmean, int N, int Cb, int C) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < (long long)C * Cb) {
    const int j = (int)(i / Cb), ci = (int)(i - (long long)j * Cb);
    float s = 0.f;
    for (int n = 0; n < N; ++n) s = fmaf(dy[(long long)n * C + j], mean[(long long)n * Cb + ci], s);
    dwpool[i] = s;
  }
  if (i < (long long)N * Cb) {
    const int n = (int)(i / Cb), ci = (int)(i - (long long)n * Cb);
    float s = 0.f;
    for (int j = 0; j < C; ++j) s = fmaf(wpool[(long long)j * Cb + ci], dy[(long long)n * C + j], s);
    dmean[i] = s;
  }
}

// ---- projection BatchNorm + ReLU + dropout.  mode 0 (forward): out = T(T(relu(scale y + shift)) * keep), keep = mask / (1 - p) (1 without a
// mask); mode 1 (backward of the dropout): out = T(y * keep).  mask: uint8 [N][C][vox] (torch's NC* order).
template <typename T>
__global__ __launch_bounds__(256) void dl_dropout_kernel(const T* __restrict__ y, long long y_ss, T* __restrict__ out, long long o_ss,
                                                         const float* scale, const float* shift, const unsigned char* mask, float inv_keep,
                                                         int mode, int C, long long vox) {
  const int pl = blockIdx.y, n = blockIdx.z;
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= vox) return;
  const long long off = ((long long)pl * vox + v) * 8;
  const V8T<T> a = *(const V8T<T>*)(y + n * y_ss + off);
  V8T<T> o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = pl * 8 + j;
    float z = mode == 0 ? norm_z<T, true>(scale[c], to_f32<T>(a[j]), shift[c]) : to_f32<T>(a[j]);
    if (mask != nullptr) z = mask[((long long)n * C + c) * vox + v] ? z * inv_keep : 0.f;
    o[j] = from_f32<T>(z);
  }
  *(V8T<T>*)(out + n * o_ss + off) = o;
}

// ---- logit upsampling, align_corners=True: resample_axis_corners of resample.h
// the fine logits of voxel (d, h, w) of sample n from coarse fp32 [N][NCLS][Dc][Hc][Wc]
template <int NCLS, int ND>
__device__ __forceinline__ void dl_up_logits(const float* lc, int n, int d, int h, int w, int Dc, int Hc, int Wc, int Df, int Hf, int Wf,
                                             float (&l)[NCLS]) {
  ResampleAx ad = {0, 0, 0.f};
  if constexpr (ND == 3) ad = resample_axis_corners(d, Df, Dc);
  const ResampleAx ah = resample_axis_corners(h, Hf, Hc), aw = resample_axis_corners(w, Wf, Wc);
  const int d0 = ad.i0, d1 = ad.i1, h0 = ah.i0, h1 = ah.i1, w0 = aw.i0, w1 = aw.i1;
  const float fd = ad.l1, fh = ah.l1, fw = aw.l1;
  const long long vc = (long long)Dc * Hc * Wc;
#pragma unroll
  for (int c = 0; c < NCLS; ++c) {
    const float* p = lc + ((long long)n * NCLS + c) * vc;
    auto plane = [&](int dd) {
      const float* q = p + (long long)dd * Hc * Wc;
      return (1.f - fh) * ((1.f - fw) * q[(long long)h0 * Wc + w0] + fw * q[(long long)h0 * Wc + w1]) +
             fh * ((1.f - fw) * q[(long long)h1 * Wc + w0] + fw * q[(long long)h1 * Wc + w1]);
    };
    if constexpr (ND == 3) l[c] = (1.f - fd) * plane(d0) + fd * plane(d1);
    else l[c] = plane(0);
  }
}

struct DlUp {
  const float* lc; int Dc, Hc, Wc, s;
  HeadOut o;
  int N, D, H, W;
};

// prediction: iunet_head_fwd's output contract on the upsampled logits
template <int NCLS, int ND>
__global__ __launch_bounds__(256) void dl_up_head_kernel(DlUp p) {
  const long long vox = (long long)p.D * p.H * p.W;
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= vox) return;
  const int n = blockIdx.y;
  const int gx = (int)(v % p.W), gy = (int)((v / p.W) % p.H), gz = (int)(v / ((long long)p.W * p.H));
  float l[NCLS];
  dl_up_logits<NCLS, ND>(p.lc, n, gz, gy, gx, p.Dc, p.Hc, p.Wc, p.D, p.H, p.W, l);
  head_store<NCLS, false>(p.o, l, n, vox, v, gz, gy, gx);
}

#define DL_UPL_ITER 8
struct DlUpLoss {
  const float* lc; int Dc, Hc, Wc;
  const void* target; const void* weight; int tdtype;
  float* slab;                      // fwd: [parts][ncls][8]
  const float* coef; const float* lscale;
  float* dfine;                     // bwd: [N][ncls][vox] fp32
  int D, H, W;
};

template <int NCLS, int ND>
__global__ __launch_bounds__(256) void dl_up_loss_fwd_kernel(DlUpLoss p) {
  const int n = blockIdx.y;
  const long long vox = (long long)p.D * p.H * p.W;
  float acc[NCLS][8];
#pragma unroll
  for (int c = 0; c < NCLS; ++c)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[c][k] = 0.f;
  for (int it = 0; it < DL_UPL_ITER; ++it) {
    const long long v = ((long long)blockIdx.x * DL_UPL_ITER + it) * 256 + threadIdx.x;
    if (v >= vox) break;
    const int gx = (int)(v % p.W), gy = (int)((v / p.W) % p.H), gz = (int)(v / ((long long)p.W * p.H));
    float l[NCLS];
    dl_up_logits<NCLS, ND>(p.lc, n, gz, gy, gx, p.Dc, p.Hc, p.Wc, p.D, p.H, p.W, l);
    loss_sums<NCLS>(l, p.target, p.weight, p.tdtype, n, vox, v, acc);
  }
  __shared__ float red[4 * NCLS * 8];
  const long long part = (long long)n * gridDim.x + blockIdx.x;
  float vals[NCLS * 8];
#pragma unroll
  for (int c = 0; c < NCLS; ++c)
#pragma unroll
    for (int k = 0; k < 8; ++k) vals[c * 8 + k] = acc[c][k];
  block_reduce_store<NCLS * 8>(vals, red, p.slab + part * NCLS * 8);
}

template <int NCLS, int ND>
__global__ __launch_bounds__(256) void dl_up_loss_bwd_kernel(DlUpLoss p) {
  const int n = blockIdx.y;
  const long long vox = (long long)p.D * p.H * p.W;
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  if (v >= vox) return;
  const int gx = (int)(v % p.W), gy = (int)((v / p.W) % p.H), gz = (int)(v / ((long long)p.W * p.H));
  float l[NCLS], dl[NCLS], sum_dl[NCLS];
#pragma unroll
  for (int c = 0; c < NCLS; ++c) sum_dl[c] = 0.f;
  dl_up_logits<NCLS, ND>(p.lc, n, gz, gy, gx, p.Dc, p.Hc, p.Wc, p.D, p.H, p.W, l);
  loss_grad<NCLS>(l, p.target, p.weight, p.tdtype, p.coef, n, vox, v, *p.lscale, dl, sum_dl);
#pragma unroll
  for (int c = 0; c < NCLS; ++c) p.dfine[((long long)n * NCLS + c) * vox + v] = dl[c];
}

// the interpolation's adjoint along one axis, as a gather: in [outer][Ef][inner] -> out [outer][Ec][inner],
// out[i] = sum over the fine o that read i of its weight x in[o] (o ascending: a fixed order)
__global__ __launch_bounds__(256) void dl_up_adjoint_kernel(const float* __restrict__ in, float* __restrict__ out, long long outer, int Ec, int Ef,
                                                            long long inner) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= outer * Ec * inner) return;
  const long long in_i = i % inner, ci = (i / inner) % Ec, ou = i / (inner * Ec);
  const int c = (int)ci;
  // fine indices whose source lies in (c - 1, c + 1): o in [(c - 1) / sc, (c + 1) / sc], widened by 2 for rounding; every o is re-tested
  const float sc = Ef > 1 ? (float)(Ec - 1) / (float)(Ef - 1) : 0.f;
  int lo = 0, hi = Ef - 1;
  if (sc > 0.f) {
    lo = max(0, (int)floorf((float)(c - 1) / sc) - 2);
    hi = min(Ef - 1, (int)ceilf((float)(c + 1) / sc) + 2);
  }
  float s = 0.f;
  for (int o = lo; o <= hi; ++o) {
    const float wgt = resample_adj_w<resample_axis_corners>(o, c, Ef, Ec);
    if (wgt != 0.f) s = fmaf(wgt, in[(ou * Ef + o) * inner + in_i], s);
  }
  out[i] = s;
}

// ---- head backward on the coarse grid: dF = W^T dl (T, NHWC8c); dW[k][c] = sum dl[k] F[c], db[k] = sum dl[k] via per-workgroup rows
template <typename T>
__global__ __launch_bounds__(256) void dl_head_dx_kernel(const float* __restrict__ dl, const float* __restrict__ w, int ncls, T* __restrict__ dx,
                                                         long long dx_ss, int C, long long vox) {
  const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
  const int n = blockIdx.y;
  if (v >= vox) return;
  float g[10];
  for (int k = 0; k < ncls; ++k) g[k] = dl[((long long)n * ncls + k) * vox + v];
  T* o = dx + (long long)n * dx_ss + v * 8;
  for (int pl = 0; pl < C / 8; ++pl) {
    V8T<T> r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float a = 0.f;
      for (int k = 0; k < ncls; ++k) a = fmaf(g[k], w[k * C + pl * 8 + j], a);
      r[j] = from_f32<T>(a);
    }
    *(V8T<T>*)(o + (long long)pl * vox * 8) = r;
  }
}

constexpr int DL_HB_PER = 2048;      // voxels per workgroup of the head's weight gradient
// grid (parts, planes + 1, N): plane pl < C/8 -> rows [ncls][8] of dW, plane C/8 -> [ncls] of db;  slab [N][parts][C/8 + 1][ncls][8]
template <typename T>
__global__ __launch_bounds__(256) void dl_head_dw_kernel(const float* __restrict__ dl, int ncls, const T* __restrict__ x, long long x_ss, int C,
                                                         long long vox, float* __restrict__ slab) {
  const int part = blockIdx.x, pl = blockIdx.y, n = blockIdx.z, planes = C / 8;
  float acc[80];
#pragma unroll
  for (int i = 0; i < 80; ++i) acc[i] = 0.f;
  const long long v0 = (long long)part * DL_HB_PER, v1 = min(vox, v0 + DL_HB_PER);
  for (long long v = v0 + threadIdx.x; v < v1; v += 256) {
    float xv[8];
    if (pl < planes) {
      const V8T<T> a = *(const V8T<T>*)(x + (long long)n * x_ss + ((long long)pl * vox + v) * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) xv[j] = to_f32<T>(a[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) xv[j] = j == 0 ? 1.f : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) {
      if (k >= ncls) break;
      const float g = dl[((long long)n * ncls + k) * vox + v];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[k * 8 + j] = fmaf(g, xv[j], acc[k * 8 + j]);
    }
  }
  __shared__ float red[4 * 80];
  float* out = slab + (((long long)n * gridDim.x + part) * (planes + 1) + pl) * 80;
  block_reduce_store<80>(acc, red, out);
}

__global__ __launch_bounds__(256) void dl_head_dw_reduce_kernel(const float* __restrict__ slab, int rows, int ncls, int C, float* __restrict__ dw,
                                                                float* __restrict__ db) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int planes = C / 8;
  if (i >= (planes + 1) * 80) return;
  const int pl = i / 80, e = i - pl * 80, k = e / 8, j = e - k * 8;
  if (k >= ncls) return;
  if (pl == planes && j != 0) return;
  float s = 0.f;
  for (int r = 0; r < rows; ++r) s += slab[((long long)r * (planes + 1) + pl) * 80 + e];
  if (pl < planes) dw[k * C + pl * 8 + j] = s;
  else db[k] = s;
}

int dl_check_grid(int nd, int N, int D, int H, int W) {
  IUNET_REQUIRE(nd == 2 || nd == 3, "deeplab: nd must be 2 or 3, got %d", nd);
  IUNET_REQUIRE_GRID("deeplab", N, D, H, W);
  IUNET_REQUIRE(nd == 3 || D == 1, "deeplab: 2-D tensors have D = 1");
  return IUNET_OK;
}

int dl_build(DlTaps& t, int nd, int nbr, const int* rates, const int* cbase, const int* colbase, int D, int H, int W, int Cin) {
  IUNET_REQUIRE(nbr >= 1 && nbr <= DL_MAXBR, "deeplab: 1 .. %d branches per launch, got %d", DL_MAXBR, nbr);
  IUNET_REQUIRE(rates && cbase && colbase, "deeplab: null branch table");
  t.n = 0;
  for (int b = 0; b < nbr; ++b) {
    IUNET_REQUIRE(rates[b] >= 0, "deeplab: rate must be >= 0 (0: 1x1), got %d", rates[b]);
    IUNET_REQUIRE(cbase[b] >= 0 && cbase[b] % 8 == 0 && colbase[b] >= 0 && colbase[b] % 8 == 0, "deeplab: channel / column bases must be multiples of 8");
    IUNET_REQUIRE(dl_add_taps(t, nd, rates[b], D, H, W, cbase[b], colbase[b], Cin), "deeplab: more than %d taps", DL_MAXT);
  }
  return IUNET_OK;
}

}  // namespace

extern "C" {

int iunet_dl_num_taps(int nd, int rate, int D, int H, int W) {
  if ((nd != 2 && nd != 3) || rate < 0 || D <= 0 || H <= 0 || W <= 0) return -1;
  DlTaps t;
  t.n = 0;
  dl_add_taps(t, nd, rate, D, H, W, 0, 0, 8);
  return t.n;
}

int iunet_dl_pack(int dtype, int nd, int mode, int ksz, const void* w, const void* gamma, const void* beta, const void* mean, const void* var,
                  float eps, void* dst, void* bias_out, int Cout, int Cin, int Cin_tot, int ci_off, int k_off, int ld, void* stream) {
  IUNET_REQUIRE(dtype >= 0 && dtype <= 2, "dl_pack: dtype must be 0 (f16), 1 (bf16) or 2 (f32), got %d", dtype);
  IUNET_REQUIRE(nd == 2 || nd == 3, "dl_pack: nd must be 2 or 3, got %d", nd);
  IUNET_REQUIRE(mode == 0 || mode == 1, "dl_pack: mode must be 0 (forward) or 1 (data gradient), got %d", mode);
  IUNET_REQUIRE(ksz == 1 || ksz == 3, "dl_pack: ksz must be 1 or 3, got %d", ksz);
  IUNET_REQUIRE(w && dst, "dl_pack: null pointer");
  IUNET_REQUIRE(Cout > 0 && Cin > 0 && ci_off >= 0 && ci_off + Cin <= Cin_tot, "dl_pack: bad channels Cout %d, Cin %d of %d at %d", Cout, Cin, Cin_tot, ci_off);
  const int kvol = ksz == 1 ? 1 : (nd == 3 ? 27 : 9);
  const long long span = (long long)kvol * (mode == 0 ? Cin : Cout);
  IUNET_REQUIRE(k_off >= 0 && k_off + span <= ld, "dl_pack: columns %d + %lld exceed the row length %d", k_off, span, ld);
  IUNET_REQUIRE(!gamma || (beta && mean && var && mode == 0), "dl_pack: a BatchNorm fold (forward only) needs gamma, beta, mean and var");
  const long long total = (long long)Cout * Cin * kvol;
  const dim3 grid((unsigned)((total + 255) / 256));
#define DLP(OT) hipLaunchKernelGGL(dl_pack_kernel<OT>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)w, (const float*)gamma, \
                                   (const float*)beta, (const float*)mean, (const float*)var, eps, (OT*)dst, (float*)bias_out, mode, kvol, Cout, Cin, \
                                   Cin_tot, ci_off, k_off, ld)
  if (dtype == 0) DLP(f16); else if (dtype == 1) DLP(bf16); else DLP(float);
#undef DLP
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_dl_stats_parts(int N, int D, int H, int W, int Cout) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cout <= 0) return -1;
  return dl_fwd_blocks(N, D, H, W, Cout);
}

int iunet_dl_conv_fwd(int dtype, int nd, const void* x, long long x_ss, void* y, long long y_ss, const void* wpk, int Kw, int nbr,
                      const int* rates, const int* cbase, const int* colbase, const void* in_scale, const void* in_shift, const void* bias,
                      const void* psb, float psb_scale, void* stats, int epi, int N, int D, int H, int W, int Cin, int Cout, void* stream) {
  IUNET_REQUIRE(dtype == 0 || dtype == 1, "dl_conv_fwd: dtype must be 0 (f16) or 1 (bf16), got %d", dtype);
  const int rc = dl_check_grid(nd, N, D, H, W);
  if (rc != IUNET_OK) return rc;
  IUNET_REQUIRE(Cin > 0 && Cout > 0 && Cin % 8 == 0 && Cout % 16 == 0, "dl_conv_fwd: Cin %d (multiple of 8), Cout %d (multiple of 16)", Cin, Cout);
  IUNET_REQUIRE(x && y && wpk, "dl_conv_fwd: null pointer");
  IUNET_REQUIRE(epi == 0 || epi == 1, "dl_conv_fwd: epi must be 0 (raw) or 1 (+bias, ReLU), got %d", epi);
  IUNET_REQUIRE(epi == 0 || bias, "dl_conv_fwd: epi 1 needs a bias");
  IUNET_REQUIRE(epi == 0 || !stats, "dl_conv_fwd: statistics are taken of the raw output (epi 0) only");
  IUNET_REQUIRE(!in_scale == !in_shift, "dl_conv_fwd: the input activation needs both scale and shift");
  GgFwd p;
  DlFwdGather g;
  const int rb = dl_build(g.taps, nd, nbr, rates, cbase, colbase, D, H, W, Cin);
  if (rb != IUNET_OK) return rb;
  for (int t = 0; t < g.taps.n; ++t)
    IUNET_REQUIRE(g.taps.col[t] + Cin <= Kw, "dl_conv_fwd: tap %d reads operator columns past the row length %d", t, Kw);
  IUNET_REQUIRE(Kw % 8 == 0, "dl_conv_fwd: the operator row length must be a multiple of 8, got %d", Kw);
  p.x = x; p.x_ss = x_ss; p.y = y; p.y_ss = y_ss; p.wpk = wpk;
  p.in_scale = (const float*)in_scale; p.in_shift = (const float*)in_shift; p.bias = (const float*)bias; p.stats = (float*)stats;
  p.N = N; p.D = D; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.K = g.taps.n * Cin;
  p.cols = (long long)N * D * H * W; p.epi = epi;
  g.lda = Kw; g.psb = (const float*)psb; g.psb_scale = psb_scale;
  const dim3 grid(dl_fwd_blocks(N, D, H, W, Cout), (Cout + GG_COG - 1) / GG_COG);
  iunet_dispatch(dtype, nd, in_scale != nullptr, [&](auto t, auto, auto act) {
    hipLaunchKernelGGL((gg_fwd_kernel<decltype(t), act.value, DlFwdGather>), grid, dim3(256), 0, (hipStream_t)stream, p, g);
  });
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

long long iunet_dl_wgrad_slab_floats(int nd, int rate, int N, int D, int H, int W, int Cin, int Cout) {
  const int nt = iunet_dl_num_taps(nd, rate, D, H, W);
  if (nt <= 0 || N <= 0 || Cin <= 0 || Cout <= 0) return -1;
  const long long per = (long long)Cout * nt * Cin;
  return gg_wgrad_splits((long long)N * D * H * W, per) * per;
}

int iunet_dl_wgrad(int dtype, int nd, int rate, const void* x, long long x_ss, int cbase, const void* dy, long long dy_ss, const void* x_scale,
                   const void* x_shift, void* slab, void* dW, int Cin_tot, int ci_off, float alpha, int N, int D, int H, int W, int Cin, int Cout,
                   void* stream) {
  IUNET_REQUIRE(dtype == 0 || dtype == 1, "dl_wgrad: dtype must be 0 (f16) or 1 (bf16), got %d", dtype);
  const int rc = dl_check_grid(nd, N, D, H, W);
  if (rc != IUNET_OK) return rc;
  IUNET_REQUIRE(Cin > 0 && Cout > 0 && Cin % 8 == 0 && Cout % 8 == 0, "dl_wgrad: Cin %d, Cout %d (multiples of 8)", Cin, Cout);
  IUNET_REQUIRE(rate >= 0 && cbase >= 0 && cbase % 8 == 0, "dl_wgrad: rate %d (>= 0), channel base %d (a multiple of 8)", rate, cbase);
  IUNET_REQUIRE(ci_off >= 0 && ci_off + Cin <= Cin_tot, "dl_wgrad: channels %d at %d of %d", Cin, ci_off, Cin_tot);
  IUNET_REQUIRE(x && dy && slab && dW, "dl_wgrad: null pointer");
  IUNET_REQUIRE(!x_scale == !x_shift, "dl_wgrad: the input activation needs both scale and shift");
  GgWg p;
  DlWgGather g;
  const int colbase = 0;
  const int rb = dl_build(g.taps, nd, 1, &rate, &cbase, &colbase, D, H, W, Cin);
  if (rb != IUNET_OK) return rb;
  g.x = x; g.x_ss = x_ss; g.in_scale = (const float*)x_scale; g.in_shift = (const float*)x_shift; g.Cin = Cin;
  p.dy = dy; p.dy_ss = dy_ss; p.slab = (float*)slab;
  p.D = D; p.H = H; p.W = W; p.Cout = Cout; p.K = g.taps.n * Cin;
  p.cols = (long long)N * D * H * W;
  const int splits = gg_wgrad_splits(p.cols, (long long)Cout * p.K);
  const long long nchunks = (p.cols + 31) / 32;
  p.chunks_per_split = (nchunks + splits - 1) / splits;
  const dim3 grid(splits, (Cout + 63) / 64, (p.K + 63) / 64);
  iunet_dispatch(dtype, nd, x_scale != nullptr, [&](auto t, auto, auto act) {
    hipLaunchKernelGGL((gg_wgrad_kernel<decltype(t), act.value, DlWgGather>), grid, dim3(256), 0, (hipStream_t)stream, p, g);
  });
  IUNET_CHECK_HIP(hipGetLastError());
  const int kvol = rate == 0 ? 1 : (nd == 3 ? 27 : 9);
  const long long total = (long long)Cout * Cin * kvol;
  hipLaunchKernelGGL(dl_wgrad_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)slab, splits,
                     Cin, Cout, p.K, kvol, alpha, (float*)dW, Cin_tot, ci_off, g.taps);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_dl_f32_conv_fwd(int nd, int rate, const void* x, long long x_ss, void* y, long long y_ss, const void* wpk, int Kw, const void* bias,
                          const void* psb, int N, int D, int H, int W, int Cin, int Cout, void* stream) {
  const int rc = dl_check_grid(nd, N, D, H, W);
  if (rc != IUNET_OK) return rc;
  IUNET_REQUIRE(Cin > 0 && Cout > 0 && Cin % 8 == 0 && Cout % 16 == 0, "dl_f32_conv_fwd: Cin %d (multiple of 8), Cout %d (multiple of 16)", Cin, Cout);
  IUNET_REQUIRE(x && y && wpk && bias, "dl_f32_conv_fwd: null pointer");
  GgFwd p = {};
  DlFwdGather g;
  const int zero = 0;
  const int rb = dl_build(g.taps, nd, 1, &rate, &zero, &zero, D, H, W, Cin);
  if (rb != IUNET_OK) return rb;
  for (int t = 0; t < g.taps.n; ++t)
    IUNET_REQUIRE(g.taps.col[t] + Cin <= Kw, "dl_f32_conv_fwd: tap %d reads operator columns past the row length %d", t, Kw);
  p.x = x; p.x_ss = x_ss; p.y = y; p.y_ss = y_ss; p.wpk = wpk; p.bias = (const float*)bias;
  p.N = N; p.D = D; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.K = g.taps.n * Cin;
  p.cols = (long long)N * D * H * W; p.epi = 1;
  g.lda = Kw; g.psb = (const float*)psb; g.psb_scale = 1.f;
  const long long tiles = (p.cols + 15) / 16;
  const dim3 grid((unsigned)((tiles + GG_WAVES - 1) / GG_WAVES), (Cout + GG_COG - 1) / GG_COG);
  hipLaunchKernelGGL(gg_f32_kernel<DlFwdGather>, grid, dim3(256), 0, (hipStream_t)stream, p, g);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_dl_chansum(int dtype, const void* x, long long x_ss, void* out, float scale, int C, int N, long long vox, void* stream) {
  IUNET_REQUIRE(dtype >= 0 && dtype <= 2, "dl_chansum: dtype must be 0 (f16), 1 (bf16) or 2 (planar f32), got %d", dtype);
  IUNET_REQUIRE(x && out, "dl_chansum: null pointer");
  IUNET_REQUIRE(C > 0 && C % 8 == 0 && N > 0 && vox > 0, "dl_chansum: C %d (multiple of 8), N %d, %lld voxels", C, N, vox);
  if (dtype == 2) {
    hipLaunchKernelGGL(dl_chansum_f32_kernel, dim3(C, N), dim3(256), 0, (hipStream_t)stream, (const float*)x, x_ss, (float*)out, scale, C, vox);
  } else if (dtype == 0) {
    hipLaunchKernelGGL(dl_chansum_kernel<f16>, dim3(C / 8, N), dim3(256), 0, (hipStream_t)stream, (const f16*)x, x_ss, (float*)out, scale, C, vox);
  } else {
    hipLaunchKernelGGL(dl_chansum_kernel<bf16>, dim3(C / 8, N), dim3(256), 0, (hipStream_t)stream, (const bf16*)x, x_ss, (float*)out, scale, C, vox);
  }
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_dl_pool_gemv(const void* mean, const void* wpool, void* ypool, void* stats, int N, int Cb, int C, void* stream) {
  IUNET_REQUIRE(mean && wpool && ypool, "dl_pool_gemv: null pointer");
  IUNET_REQUIRE(N > 0 && Cb > 0 && C > 0, "dl_pool_gemv: N %d, Cb %d, C %d", N, Cb, C);
  hipLaunchKernelGGL(dl_pool_gemv_kernel, dim3((N * C + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)mean, (const float*)wpool,
                     (float*)ypool, (float*)stats, N, Cb, C);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_dl_pool_psb(const void* ypool, const void* scale, const void* shift, const void* gamma, const void* beta, const void* rmean,
                      const void* rvar, float eps, void* bp, const void* wproj, const void* pgamma, const void* pvar, void* psb, int N, int C,
                      void* stream) {
  IUNET_REQUIRE(ypool && bp && wproj && psb, "dl_pool_psb: null pointer");
  IUNET_REQUIRE(!scale == !shift, "dl_pool_psb: scale and shift go together");
  IUNET_REQUIRE(scale || (gamma && beta && rmean && rvar), "dl_pool_psb: eval mode needs gamma, beta and the running statistics");
  IUNET_REQUIRE(!pgamma == !pvar, "dl_pool_psb: the projection's fold needs its gamma and running variance");
  IUNET_REQUIRE(N > 0 && C > 0, "dl_pool_psb: N %d, C %d", N, C);
  const dim3 g((N * C + 255) / 256);
  hipLaunchKernelGGL(dl_pool_bp_kernel, g, dim3(256), 0, (hipStream_t)stream, (const float*)ypool, (const float*)scale, (const float*)shift,
                     (const float*)gamma, (const float*)beta, (const float*)rmean, (const float*)rvar, eps, (float*)bp, N, C);
  hipLaunchKernelGGL(dl_pool_psb_kernel, g, dim3(256), 0, (hipStream_t)stream, (const float*)bp, (const float*)wproj, (const float*)pgamma,
                     (const float*)pvar, eps, (float*)psb, N, C);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_dl_pool_bwd(const void* dpsb, const void* bp, const void* ypool, const void* mean, const void* invstd, const void* gamma,
                      const void* wproj, const void* wpool, const void* xmean, void* dwproj, void* dgamma, void* dbeta, void* dwpool,
                      void* dxmean, void* scratch, int N, int Cb, int C, void* stream) {
  IUNET_REQUIRE(dpsb && bp && ypool && mean && invstd && gamma && wproj && wpool && xmean && dwproj && dgamma && dbeta && dwpool && dxmean && scratch,
                "dl_pool_bwd: null pointer");
  IUNET_REQUIRE(N > 1 && Cb > 0 && C > 0, "dl_pool_bwd: N %d (batch statistics need 2 or more), Cb %d, C %d", N, Cb, C);
  float* dbp = (float*)scratch;
  float* dy = dbp + (long long)N * C;
  const long long n1 = (long long)C * C > (long long)N * C ? (long long)C * C : (long long)N * C;
  hipLaunchKernelGGL(dl_pool_bwd1_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)dpsb,
                     (const float*)bp, (const float*)wproj, (float*)dwproj, dbp, N, C);
  hipLaunchKernelGGL(dl_pool_bwd2_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)dbp, (const float*)bp,
                     (const float*)ypool, (const float*)mean, (const float*)invstd, (const float*)gamma, (float*)dgamma, (float*)dbeta, dy, N, C);
  const long long n3 = (long long)C * Cb > (long long)N * Cb ? (long long)C * Cb : (long long)N * Cb;
  hipLaunchKernelGGL(dl_pool_bwd3_kernel, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)dy,
                     (const float*)xmean, (const float*)wpool, (float*)dwpool, (float*)dxmean, N, Cb, C);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_dl_dropout(int dtype, int mode, const void* y, long long y_ss, void* out, long long out_ss, const void* scale, const void* shift,
                     const void* mask, float p, int C, int N, long long vox, void* stream) {
  IUNET_REQUIRE(dtype == 0 || dtype == 1, "dl_dropout: dtype must be 0 (f16) or 1 (bf16), got %d", dtype);
  IUNET_REQUIRE(mode == 0 || mode == 1, "dl_dropout: mode must be 0 (forward) or 1 (backward), got %d", mode);
  IUNET_REQUIRE(y && out, "dl_dropout: null pointer");
  IUNET_REQUIRE(mode == 1 || (scale && shift), "dl_dropout: the forward needs the BatchNorm scale and shift");
  IUNET_REQUIRE(p >= 0.f && p < 1.f, "dl_dropout: p must be in [0, 1), got %g", (double)p);
  IUNET_REQUIRE(C > 0 && C % 8 == 0 && N > 0 && vox > 0, "dl_dropout: C %d (multiple of 8), N %d, %lld voxels", C, N, vox);
  const dim3 grid((unsigned)((vox + 255) / 256), C / 8, N);
  const float ik = 1.f / (1.f - p);
  if (dtype == 0)
    hipLaunchKernelGGL(dl_dropout_kernel<f16>, grid, dim3(256), 0, (hipStream_t)stream, (const f16*)y, y_ss, (f16*)out, out_ss, (const float*)scale,
                       (const float*)shift, (const unsigned char*)mask, ik, mode, C, vox);
  else
    hipLaunchKernelGGL(dl_dropout_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)y, y_ss, (bf16*)out, out_ss, (const float*)scale,
                       (const float*)shift, (const unsigned char*)mask, ik, mode, C, vox);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

#define DL_NCLS_SWITCH(MAC, NDV) \
  switch (ncls) { case 2: MAC(2, NDV); break; case 3: MAC(3, NDV); break; case 4: MAC(4, NDV); break; case 5: MAC(5, NDV); break; \
                  case 6: MAC(6, NDV); break; case 7: MAC(7, NDV); break; case 8: MAC(8, NDV); break; case 9: MAC(9, NDV); break; \
                  default: MAC(10, NDV); break; }

static int dl_up_check(const char* what, int nd, const void* lc, int ncls, int N, int Dc, int Hc, int Wc, int s) {
  IUNET_REQUIRE(nd == 2 || nd == 3, "%s: nd must be 2 or 3, got %d", what, nd);
  IUNET_REQUIRE(lc, "%s: null pointer", what);
  IUNET_REQUIRE(ncls >= 2 && ncls <= 10, "%s: num_classes must be 2..10, got %d", what, ncls);
  IUNET_REQUIRE(N > 0 && Dc > 0 && Hc > 0 && Wc > 0 && (nd == 3 || Dc == 1), "%s: bad coarse grid N %d, %d x %d x %d", what, N, Dc, Hc, Wc);
  IUNET_REQUIRE(s >= 1 && s <= 64, "%s: scale factor must be 1..64, got %d", what, s);
  return IUNET_OK;
}

int iunet_dl_up_head(int nd, const void* lc, int ncls, int Dc, int Hc, int Wc, int s, void* logits, void* probs, void* cls,
                     const long long* out_strides, float divisor, int accumulate, int N, void* stream) {
  const int rc = dl_up_check("dl_up_head", nd, lc, ncls, N, Dc, Hc, Wc, s);
  if (rc != IUNET_OK) return rc;
  DlUp p;
  if (const int rc2 = head_out_fill(p.o, "dl_up_head", logits, probs, cls, out_strides, divisor, accumulate)) return rc2;
  p.lc = (const float*)lc; p.Dc = Dc; p.Hc = Hc; p.Wc = Wc; p.s = s; p.N = N;
  p.D = nd == 3 ? Dc * s : 1; p.H = Hc * s; p.W = Wc * s;
  const long long vox = (long long)p.D * p.H * p.W;
  const dim3 grid((unsigned)((vox + 255) / 256), N);
#define DLU(NC, NDV) hipLaunchKernelGGL((dl_up_head_kernel<NC, NDV>), grid, dim3(256), 0, (hipStream_t)stream, p)
  if (nd == 3) { DL_NCLS_SWITCH(DLU, 3) } else { DL_NCLS_SWITCH(DLU, 2) }
#undef DLU
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_dl_up_loss_num_parts(int N, long long vox) {
  if (N <= 0 || vox <= 0) return -1;
  return N * (int)((vox + 256 * DL_UPL_ITER - 1) / (256 * DL_UPL_ITER));
}

int iunet_dl_up_loss_fwd(int nd, const void* lc, int ncls, int Dc, int Hc, int Wc, int s, const void* target, const void* weight, int tdtype,
                         int kind, void* slab, void* out4, void* coef, int N, void* stream) {
  const int rc = dl_up_check("dl_up_loss_fwd", nd, lc, ncls, N, Dc, Hc, Wc, s);
  if (rc != IUNET_OK) return rc;
  IUNET_REQUIRE(target && slab && out4 && coef, "dl_up_loss_fwd: null pointer");
  IUNET_REQUIRE(kind >= 0 && kind <= 6, "dl_up_loss_fwd: unknown loss kind %d", kind);
  IUNET_REQUIRE(tdtype == 0 || tdtype == 1, "dl_up_loss_fwd: target dtype must be 0 (f32) or 1 (f16)");
  DlUpLoss p;
  p.lc = (const float*)lc; p.Dc = Dc; p.Hc = Hc; p.Wc = Wc;
  p.target = target; p.weight = weight; p.tdtype = tdtype; p.slab = (float*)slab;
  p.coef = nullptr; p.lscale = nullptr; p.dfine = nullptr;
  p.D = nd == 3 ? Dc * s : 1; p.H = Hc * s; p.W = Wc * s;
  const long long vox = (long long)p.D * p.H * p.W;
  const int nparts = iunet_dl_up_loss_num_parts(N, vox);
  const dim3 grid((unsigned)(nparts / N), N);
#define DLL(NC, NDV) hipLaunchKernelGGL((dl_up_loss_fwd_kernel<NC, NDV>), grid, dim3(256), 0, (hipStream_t)stream, p)
  if (nd == 3) { DL_NCLS_SWITCH(DLL, 3) } else { DL_NCLS_SWITCH(DLL, 2) }
#undef DLL
  IUNET_CHECK_HIP(hipGetLastError());
  return iunet_loss_finalize_launch((const float*)slab, nparts, ncls, kind, weight != nullptr, (double)N * (double)vox, (float*)out4,
                                    (float*)coef, (hipStream_t)stream);
}

int iunet_dl_up_loss_bwd(int nd, const void* lc, int ncls, int Dc, int Hc, int Wc, int s, const void* target, const void* weight, int tdtype,
                         const void* coef, const void* lscale, void* dfine, void* tmp, void* dcoarse, int N, void* stream) {
  const int rc = dl_up_check("dl_up_loss_bwd", nd, lc, ncls, N, Dc, Hc, Wc, s);
  if (rc != IUNET_OK) return rc;
  IUNET_REQUIRE(target && coef && lscale && dfine && tmp && dcoarse, "dl_up_loss_bwd: null pointer");
  IUNET_REQUIRE(tdtype == 0 || tdtype == 1, "dl_up_loss_bwd: target dtype must be 0 (f32) or 1 (f16)");
  DlUpLoss p;
  p.lc = (const float*)lc; p.Dc = Dc; p.Hc = Hc; p.Wc = Wc;
  p.target = target; p.weight = weight; p.tdtype = tdtype; p.slab = nullptr;
  p.coef = (const float*)coef; p.lscale = (const float*)lscale; p.dfine = (float*)dfine;
  const int Df = nd == 3 ? Dc * s : 1, Hf = Hc * s, Wf = Wc * s;
  p.D = Df; p.H = Hf; p.W = Wf;
  const long long vox = (long long)Df * Hf * Wf;
  const dim3 grid((unsigned)((vox + 255) / 256), N);
#define DLB(NC, NDV) hipLaunchKernelGGL((dl_up_loss_bwd_kernel<NC, NDV>), grid, dim3(256), 0, (hipStream_t)stream, p)
  if (nd == 3) { DL_NCLS_SWITCH(DLB, 3) } else { DL_NCLS_SWITCH(DLB, 2) }
#undef DLB
  IUNET_CHECK_HIP(hipGetLastError());
  // the adjoint, axis by axis: W (dfine -> tmp), H (tmp -> dfine, 2-D: -> dcoarse), D (dfine -> dcoarse)
  const long long rows = (long long)N * ncls;
  auto adj = [&](const float* in, float* out, long long outer, int Ec, int Ef, long long inner) {
    const long long tot = outer * Ec * inner;
    hipLaunchKernelGGL(dl_up_adjoint_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, out, outer, Ec, Ef, inner);
  };
  adj((const float*)dfine, (float*)tmp, rows * Df * Hf, Wc, Wf, 1);
  adj((const float*)tmp, nd == 3 ? (float*)dfine : (float*)dcoarse, rows * Df, Hc, Hf, Wc);
  if (nd == 3) adj((const float*)dfine, (float*)dcoarse, rows, Dc, Df, (long long)Hc * Wc);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_dl_head_bwd_parts(int N, long long vox) {
  if (N <= 0 || vox <= 0) return -1;
  return N * (int)((vox + DL_HB_PER - 1) / DL_HB_PER);
}

int iunet_dl_head_bwd(int dtype, const void* x, long long x_ss, int C, const void* w, const void* dl, int ncls, void* dx, long long dx_ss, void* slab,
                      void* dw, void* db, int N, long long vox, void* stream) {
  IUNET_REQUIRE(dtype == 0 || dtype == 1, "dl_head_bwd: dtype must be 0 (f16) or 1 (bf16), got %d", dtype);
  IUNET_REQUIRE(x && w && dl && dx && slab && dw && db, "dl_head_bwd: null pointer");
  IUNET_REQUIRE(ncls >= 2 && ncls <= 10, "dl_head_bwd: num_classes must be 2..10, got %d", ncls);
  IUNET_REQUIRE(C > 0 && C % 8 == 0 && N > 0 && vox > 0, "dl_head_bwd: C %d (multiple of 8), N %d, %lld voxels", C, N, vox);
  const int parts = (int)((vox + DL_HB_PER - 1) / DL_HB_PER);
  const dim3 g1((unsigned)((vox + 255) / 256), N), g2(parts, C / 8 + 1, N);
  if (dtype == 0) {
    hipLaunchKernelGGL(dl_head_dx_kernel<f16>, g1, dim3(256), 0, (hipStream_t)stream, (const float*)dl, (const float*)w, ncls, (f16*)dx, dx_ss, C, vox);
    hipLaunchKernelGGL(dl_head_dw_kernel<f16>, g2, dim3(256), 0, (hipStream_t)stream, (const float*)dl, ncls, (const f16*)x, x_ss, C, vox, (float*)slab);
  } else {
    hipLaunchKernelGGL(dl_head_dx_kernel<bf16>, g1, dim3(256), 0, (hipStream_t)stream, (const float*)dl, (const float*)w, ncls, (bf16*)dx, dx_ss, C, vox);
    hipLaunchKernelGGL(dl_head_dw_kernel<bf16>, g2, dim3(256), 0, (hipStream_t)stream, (const float*)dl, ncls, (const bf16*)x, x_ss, C, vox, (float*)slab);
  }
  hipLaunchKernelGGL(dl_head_dw_reduce_kernel, dim3(((C / 8 + 1) * 80 + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)slab,
                     N * parts, ncls, C, (float*)dw, (float*)db);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

}  // extern "C"
