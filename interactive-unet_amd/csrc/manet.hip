// MA-Net decoder kernels (Fan et al. 2020): what the network adds to the convs this library already has.
//   ma_attn_fwd_kernel      position attention on the coarsest grid, flash style on the 16-bit MFMA: Y = X + softmax_j(Kc Q^T) V + bv
//   ma_attn_rows_kernel     its backward, the launch that owns row blocks i:    delta_i = sum_j P_ij dP_ij, dKc
//   ma_attn_cols_kernel     its backward, the launch that owns column blocks j: dV, dQ
//   ma_f32_attn_fwd_kernel  the forward on planar fp32 with the f32-input MFMA (an fp32 fma chain: exact fp32 products)
//   ma_gate_kernel / _bwd   the two squeeze-and-excitation branches of a decoder block in one launch: g[n][c] = g_hl + g_ll
//   ma_up_gate_kernel       u = nearest_up2(relu(scale y + shift)) g[n][c] into a channel slot, with its backward (ma_up_gate_dg_kernel and
//                           ma_dg_sum_kernel: dg, ma_up_gate_bwd_kernel: dh) and ma_add_mean_kernel (the mean's share of a gradient)
// Tensors are NHWC8c (dtype 0 f16 / 1 bf16) or planar fp32 [N][C][vox] (dtype 2) with sample strides in elements.  A token is a voxel of
// the coarsest grid: element (t, c) of a 16-bit tensor over T tokens sits at ((c / 8) T + t) 8 + c % 8.
//
// Attention, S[i][j] = sum_k (Kc[i][k] + bk[k]) (Q[j][k] + bq[k]) over K = 64, A = the row softmax, O = A V.  All three 16-bit kernels share
// one shape: a wave OWNS 16 tokens and WALKS the others 32 at a time.
//   first products   G^T[w][o] = sum_k Wk[w][k] Ok[o][k]: both operands are 16-byte loads of 8 consecutive channels of one token (the biases
//                    are added, and the sum rounded to the activation type, on load).  The result has the owned token on the lane and 4 + 4
//                    walked tokens in its registers: the softmax statistics of an owned row need no LDS, and
//   second products  Out^T[c][o] = sum_w M[w][c] R^T[w][o] take R^T (P or dS, rounded to the activation type) straight from those registers
//                    as the B operand; its k order is then w = 4 (lane / 16) + e, 16 + 4 (lane / 16) + e - 4 for element e of a lane, so
//                    the A operand M^T[c][w] is read in that order from an LDS image [channel][walked token] that the workgroup's four waves
//                    fill (a transpose by 2-byte LDS stores: NHWC8c has channels, not tokens, contiguous).
// The forward splits O's channels over the grid, 128 per workgroup, and recomputes S there (64 of the 64 + 128 contraction depth of a step):
// 32 accumulator registers per lane whatever Cb, and Cb / 128 times the workgroups on a grid of at most a few thousand tokens.
// The backward recomputes: P from Q, Kc and lse; delta from P and dP (delta_i = sum_c dY[i][c] O'[i][c] = sum_j P_ij dP_ij, so O' is never
// stored): the row launch walks j twice, first for delta (written for the column launch), then for dKc.
// Every sum is fp32 in a fixed order (MFMA chains, xor trees, serial loops): no float atomics, a repeated launch is bit-equal.
#include "common.h"
#include "resample.h"

namespace {

constexpr int MA_K = 64;          // query / key width
constexpr int MA_OWN = 64;        // owned tokens per workgroup: 16 per wave
constexpr int MA_WALK = 32;       // walked tokens per step
constexpr int MA_CH = 128;        // channels of the second product per workgroup
constexpr int MA_LD = 36;         // LDS row of the [channel][walked token] image: 32 tokens + 4 (72 bytes: 8-byte aligned reads)
constexpr int MA_MAX_T = 65536;

template <typename T> __device__ __forceinline__ V8T<T> ma_zero8() {
  V8T<T> z;
#pragma unroll
  for (int j = 0; j < 8; ++j) z[j] = from_f32<T>(0.f);
  return z;
}

// 8 channels (group kg) of token t of a [tokens][*] tensor, + bias, rounded to T
template <typename T>
__device__ __forceinline__ V8T<T> ma_load8(const T* s, int tokens, int t, int kg, const float* bias) {
  V8T<T> v = *(const V8T<T>*)(s + ((long long)kg * tokens + t) * 8);
  if (bias != nullptr) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = from_f32<T>(to_f32<T>(v[j]) + bias[kg * 8 + j]);
  }
  return v;
}

// The [channel][walked token] LDS image of MA_WALK tokens x NC channels (from channel c0) of a [tokens][*] tensor: loaded to registers a step
// ahead (load), written transposed after the barrier that ends the previous step's reads (write).  Tokens past the end are zeros.
template <typename T, int NC>
struct MaStage {
  static constexpr int R = NC * MA_WALK / 8 / 256;       // 16-byte items per thread
  V8T<T> v[R];
  __device__ __forceinline__ void load(const T* s, int tokens, int w0, int c0, const float* bias) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int item = threadIdx.x + 256 * r, t = item & (MA_WALK - 1), g = item / MA_WALK, tok = w0 + t;
      v[r] = tok < tokens ? ma_load8<T>(s, tokens, tok, c0 / 8 + g, bias) : ma_zero8<T>();
    }
  }
  __device__ __forceinline__ void write(T* lds) const {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int item = threadIdx.x + 256 * r, t = item & (MA_WALK - 1), g = item / MA_WALK;
#pragma unroll
      for (int e = 0; e < 8; ++e) lds[(g * 8 + e) * MA_LD + t] = v[r][e];
    }
  }
};

// the A fragment M^T[channel row][walked token] of one step, in the k order of a register-held B operand
template <typename T>
__device__ __forceinline__ V8T<T> ma_lds_frag(const T* lds, int row, int fq) {
  typedef typename Vec4<T>::type V4;
  const V4 lo = *(const V4*)(lds + row * MA_LD + 4 * fq);
  const V4 hi = *(const V4*)(lds + row * MA_LD + 16 + 4 * fq);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// two accumulator tiles (walked tokens 4 fq + r and 16 + 4 fq + r) as the B operand of the second product
template <typename T>
__device__ __forceinline__ V8T<T> ma_pack(const f32x4& a, const f32x4& b) {
  V8T<T> o;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    o[r] = from_f32<T>(a[r]);
    o[4 + r] = from_f32<T>(b[r]);
  }
  return o;
}

// max / sum over the four lane groups that share an owned token (lanes l, l ^ 16, l ^ 32, l ^ 48): a fixed tree
__device__ __forceinline__ float ma_group_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float ma_group_sum(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

struct MaAttn {
  const void* q; long long q_ss; const float* bq;
  const void* k; long long k_ss; const float* bk;
  const void* v; long long v_ss;
  const void* x; long long x_ss; const float* bv;
  void* y; long long y_ss;
  float* lse;
  int Cb, T, N;
};

template <typename T>
__global__ __launch_bounds__(256) void ma_attn_fwd_kernel(MaAttn p) {
  __shared__ __attribute__((aligned(16))) T vt[MA_CH * MA_LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
  const int n = blockIdx.z, c0 = blockIdx.y * MA_CH, Tn = p.T;
  const int i = blockIdx.x * MA_OWN + wave * 16 + fr, ic = min(i, Tn - 1);
  const T* q = (const T*)p.q + (long long)n * p.q_ss;
  const T* k = (const T*)p.k + (long long)n * p.k_ss;
  const T* v = (const T*)p.v + (long long)n * p.v_ss;
  V8T<T> kb[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) kb[s] = ma_load8<T>(k, Tn, ic, 4 * s + fq, p.bk);
  f32x4 acc[MA_CH / 16];
#pragma unroll
  for (int ct = 0; ct < MA_CH / 16; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;
  MaStage<T, MA_CH> stg;
  stg.load(v, Tn, 0, c0, nullptr);
  for (int w0 = 0; w0 < Tn; w0 += MA_WALK) {
    __syncthreads();                                   // the previous step's fragment reads
    stg.write(vt);
    __syncthreads();
    if (w0 + MA_WALK < Tn) stg.load(v, Tn, w0 + MA_WALK, c0, nullptr);
    f32x4 st[2];                                       // S^T[j = w0 + 16 t2 + 4 fq + r][i]
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      st[t2] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int jc = min(w0 + 16 * t2 + fr, Tn - 1);
#pragma unroll
      for (int s = 0; s < 2; ++s) st[t2] = mfma16<T>(ma_load8<T>(q, Tn, jc, 4 * s + fq, p.bq), kb[s], st[t2]);
    }
    float mb = -INFINITY;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (w0 + 16 * t2 + 4 * fq + r >= Tn) st[t2][r] = -INFINITY;
        mb = fmaxf(mb, st[t2][r]);
      }
    const float m_new = fmaxf(m_run, ma_group_max(mb));    // finite: token w0 < T is in every step
    const float alpha = __expf(m_run - m_new);
    float ps = 0.f;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        st[t2][r] = __expf(st[t2][r] - m_new);
        ps += st[t2][r];
      }
    l_run = l_run * alpha + ma_group_sum(ps);
    m_run = m_new;
    const V8T<T> pb = ma_pack<T>(st[0], st[1]);
#pragma unroll
    for (int ct = 0; ct < MA_CH / 16; ++ct) {
      acc[ct] *= alpha;
      acc[ct] = mfma16<T>(ma_lds_frag<T>(vt, 16 * ct + fr, fq), pb, acc[ct]);
    }
  }
  if (i >= Tn) return;
  // acc[ct][r] = O^T[c0 + 16 ct + 4 fq + r][i] l_run: four consecutive channels of one group
  typedef typename Vec4<T>::type V4;
  const float inv = 1.f / l_run;
  const T* x = (const T*)p.x + (long long)n * p.x_ss;
  T* y = (T*)p.y + (long long)n * p.y_ss;
#pragma unroll
  for (int ct = 0; ct < MA_CH / 16; ++ct) {
    const int c = c0 + 16 * ct + 4 * fq;
    const long long at = ((long long)(c >> 3) * Tn + i) * 8 + (c & 7);
    const V4 xv = *(const V4*)(x + at);
    V4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = from_f32<T>(to_f32<T>(xv[r]) + (acc[ct][r] * inv + p.bv[c + r]));
    *(V4*)(y + at) = o;
  }
  if (blockIdx.y == 0 && fq == 0) p.lse[(long long)n * Tn + i] = m_run + __logf(l_run);
}

// ---- the same contract on planar fp32 [C][T]: the f32-input MFMA 16x16x4 (lane l: A[row l & 15][k = l >> 4], B[k = l >> 4][col l & 15]), P
// kept in fp32.  The second product takes k-step r from accumulator register r (walked token 4 (l >> 4) + r), so nothing goes through LDS.
__global__ __launch_bounds__(256) void ma_f32_attn_fwd_kernel(MaAttn p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
  const int n = blockIdx.z, c0 = blockIdx.y * MA_CH, Tn = p.T;
  const int i = blockIdx.x * MA_OWN + wave * 16 + fr, ic = min(i, Tn - 1);
  const float* q = (const float*)p.q + (long long)n * p.q_ss;
  const float* k = (const float*)p.k + (long long)n * p.k_ss;
  const float* v = (const float*)p.v + (long long)n * p.v_ss;
  float kb[MA_K / 4];
#pragma unroll
  for (int s = 0; s < MA_K / 4; ++s) kb[s] = k[(long long)(4 * s + fq) * Tn + ic] + p.bk[4 * s + fq];
  f32x4 acc[MA_CH / 16];
#pragma unroll
  for (int ct = 0; ct < MA_CH / 16; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;
  for (int w0 = 0; w0 < Tn; w0 += 16) {
    const int jc = min(w0 + fr, Tn - 1);
    f32x4 st = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < MA_K / 4; ++s)
      st = __builtin_amdgcn_mfma_f32_16x16x4f32(q[(long long)(4 * s + fq) * Tn + jc] + p.bq[4 * s + fq], kb[s], st, 0, 0, 0);
    float mb = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (w0 + 4 * fq + r >= Tn) st[r] = -INFINITY;
      mb = fmaxf(mb, st[r]);
    }
    const float m_new = fmaxf(m_run, ma_group_max(mb));
    const float alpha = expf(m_run - m_new);
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      st[r] = expf(st[r] - m_new);
      ps += st[r];
    }
    l_run = l_run * alpha + ma_group_sum(ps);
    m_run = m_new;
#pragma unroll
    for (int ct = 0; ct < MA_CH / 16; ++ct) {
      acc[ct] *= alpha;
      const float* vr = v + (long long)(c0 + 16 * ct + fr) * Tn;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = w0 + 4 * fq + r;
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(j < Tn ? vr[j] : 0.f, st[r], acc[ct], 0, 0, 0);
      }
    }
  }
  if (i >= Tn) return;
  const float inv = 1.f / l_run;
  const float* x = (const float*)p.x + (long long)n * p.x_ss;
  float* y = (float*)p.y + (long long)n * p.y_ss;
#pragma unroll
  for (int ct = 0; ct < MA_CH / 16; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = c0 + 16 * ct + 4 * fq + r;
      y[(long long)c * Tn + i] = x[(long long)c * Tn + i] + (acc[ct][r] * inv + p.bv[c]);
    }
  if (blockIdx.y == 0 && fq == 0) p.lse[(long long)n * Tn + i] = m_run + logf(l_run);
}

// ---- backward.  dY: the gradient of Y; dX = dY is the residual's share (the caller adds it where it gathers X's gradient).
struct MaAttnBwd {
  const void* q; long long q_ss; const float* bq;
  const void* k; long long k_ss; const float* bk;
  const void* v; long long v_ss;
  const void* dy; long long dy_ss;
  const float* lse;
  float* delta;                                   // [N][T]: written by the row launch, read by the column launch
  void* dq; long long dq_ss;
  void* dk; long long dk_ss;
  void* dv; long long dv_ss;
  int Cb, T, N;
};

// P^T and dP^T of one step of the row launch: tiles [j = w0 + 16 t2 + 4 fq + r][i]
// dyf: the owned row's dY fragments (channels 32 cs + 8 fq .. + 8), loaded once per wave -- they do not depend on the walked step
template <typename T, int NCS>
__device__ __forceinline__ void ma_rows_tiles(const MaAttnBwd& p, const T* q, const T* v, const V8T<T> (&dyf)[NCS], const V8T<T> (&kb)[2], int w0,
                                              float lse_i, int fr, int fq, f32x4 (&pt)[2], f32x4 (&dpt)[2]) {
  const int Tn = p.T;
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2) {
    const int jc = min(w0 + 16 * t2 + fr, Tn - 1);
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) s = mfma16<T>(ma_load8<T>(q, Tn, jc, 4 * ks + fq, p.bq), kb[ks], s);
    f32x4 d = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int cs = 0; cs < NCS; ++cs) d = mfma16<T>(ma_load8<T>(v, Tn, jc, 4 * cs + fq, nullptr), dyf[cs], d);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool in = w0 + 16 * t2 + 4 * fq + r < Tn;
      pt[t2][r] = in ? __expf(s[r] - lse_i) : 0.f;
      dpt[t2][r] = in ? d[r] : 0.f;
    }
  }
}

template <typename T, int NCS>          // NCS = Cb / 32
__global__ __launch_bounds__(256) void ma_attn_rows_kernel(MaAttnBwd p) {
  __shared__ __attribute__((aligned(16))) T qt[MA_K * MA_LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
  const int n = blockIdx.z, Tn = p.T;
  const int i = blockIdx.x * MA_OWN + wave * 16 + fr, ic = min(i, Tn - 1);
  const T* q = (const T*)p.q + (long long)n * p.q_ss;
  const T* k = (const T*)p.k + (long long)n * p.k_ss;
  const T* v = (const T*)p.v + (long long)n * p.v_ss;
  const T* dy = (const T*)p.dy + (long long)n * p.dy_ss;
  V8T<T> kb[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) kb[s] = ma_load8<T>(k, Tn, ic, 4 * s + fq, p.bk);
  const float lse_i = p.lse[(long long)n * Tn + ic];
  V8T<T> dyf[NCS];
#pragma unroll
  for (int cs = 0; cs < NCS; ++cs) dyf[cs] = ma_load8<T>(dy, Tn, ic, 4 * cs + fq, nullptr);
  f32x4 pt[2], dpt[2];
  // pass 1: delta_i = sum_j P_ij dP_ij (per lane in j order, then the tree over the four lane groups)
  float dl = 0.f;
  for (int w0 = 0; w0 < Tn; w0 += MA_WALK) {
    ma_rows_tiles<T, NCS>(p, q, v, dyf, kb, w0, lse_i, fr, fq, pt, dpt);
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
      for (int r = 0; r < 4; ++r) dl = fmaf(pt[t2][r], dpt[t2][r], dl);
  }
  dl = ma_group_sum(dl);
  if (i < Tn && fq == 0) p.delta[(long long)n * Tn + i] = dl;
  // pass 2: dKc^T[k][i] = sum_j Q'^T[k][j] dS^T[j][i], dS = P (dP - delta)
  f32x4 acc[MA_K / 16];
#pragma unroll
  for (int kt = 0; kt < MA_K / 16; ++kt) acc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
  MaStage<T, MA_K> stg;
  stg.load(q, Tn, 0, 0, p.bq);
  for (int w0 = 0; w0 < Tn; w0 += MA_WALK) {
    __syncthreads();
    stg.write(qt);
    __syncthreads();
    if (w0 + MA_WALK < Tn) stg.load(q, Tn, w0 + MA_WALK, 0, p.bq);
    ma_rows_tiles<T, NCS>(p, q, v, dyf, kb, w0, lse_i, fr, fq, pt, dpt);
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
      for (int r = 0; r < 4; ++r) pt[t2][r] *= dpt[t2][r] - dl;
    const V8T<T> ds = ma_pack<T>(pt[0], pt[1]);
#pragma unroll
    for (int kt = 0; kt < MA_K / 16; ++kt) acc[kt] = mfma16<T>(ma_lds_frag<T>(qt, 16 * kt + fr, fq), ds, acc[kt]);
  }
  if (i >= Tn) return;
  typedef typename Vec4<T>::type V4;
  T* dk = (T*)p.dk + (long long)n * p.dk_ss;
#pragma unroll
  for (int kt = 0; kt < MA_K / 16; ++kt) {
    const int c = 16 * kt + 4 * fq;
    V4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = from_f32<T>(acc[kt][r]);
    *(V4*)(dk + ((long long)(c >> 3) * Tn + i) * 8 + (c & 7)) = o;
  }
}

// The column launch: a wave owns 16 tokens j and walks the rows i.  blockIdx.y < Cb / 128: dV's channels [128 y, 128 y + 128) (M = dY, R = P);
// blockIdx.y == Cb / 128: dQ (M = Kc', R = dS).  Tiles are [i = w0 + 16 t2 + 4 fq + r][j].
template <typename T>
__global__ __launch_bounds__(256) void ma_attn_cols_kernel(MaAttnBwd p) {
  __shared__ __attribute__((aligned(16))) T mt[MA_CH * MA_LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15, fq = lane >> 4;
  const int n = blockIdx.z, Tn = p.T;
  const bool for_q = (int)blockIdx.y == p.Cb / MA_CH;
  const int c0 = for_q ? 0 : blockIdx.y * MA_CH;
  const int j = blockIdx.x * MA_OWN + wave * 16 + fr, jc = min(j, Tn - 1);
  const T* q = (const T*)p.q + (long long)n * p.q_ss;
  const T* k = (const T*)p.k + (long long)n * p.k_ss;
  const T* v = (const T*)p.v + (long long)n * p.v_ss;
  const T* dy = (const T*)p.dy + (long long)n * p.dy_ss;
  const float* lse = p.lse + (long long)n * Tn;
  const float* delta = p.delta + (long long)n * Tn;
  V8T<T> qb[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) qb[s] = ma_load8<T>(q, Tn, jc, 4 * s + fq, p.bq);
  f32x4 acc[MA_CH / 16];
#pragma unroll
  for (int ct = 0; ct < MA_CH / 16; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  MaStage<T, MA_CH> stg;                                // dQ uses the first 64 rows of the image (Kc'), the other rows hold zeros
  auto load = [&](int w0) {
    if (for_q) {
#pragma unroll
      for (int r = 0; r < MaStage<T, MA_CH>::R; ++r) {
        const int item = threadIdx.x + 256 * r, t = item & (MA_WALK - 1), g = item / MA_WALK, tok = w0 + t;
        stg.v[r] = (tok < Tn && g < MA_K / 8) ? ma_load8<T>(k, Tn, tok, g, p.bk) : ma_zero8<T>();
      }
    } else {
      stg.load(dy, Tn, w0, c0, nullptr);
    }
  };
  load(0);
  for (int w0 = 0; w0 < Tn; w0 += MA_WALK) {
    __syncthreads();
    stg.write(mt);
    __syncthreads();
    if (w0 + MA_WALK < Tn) load(w0 + MA_WALK);
    f32x4 rt[2];
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      const int ic = min(w0 + 16 * t2 + fr, Tn - 1);
      f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) s = mfma16<T>(ma_load8<T>(k, Tn, ic, 4 * ks + fq, p.bk), qb[ks], s);
      f32x4 d = f32x4{0.f, 0.f, 0.f, 0.f};
      if (for_q)
        for (int cs = 0; cs < p.Cb / 32; ++cs)
          d = mfma16<T>(ma_load8<T>(dy, Tn, ic, 4 * cs + fq, nullptr), ma_load8<T>(v, Tn, jc, 4 * cs + fq, nullptr), d);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ir = w0 + 16 * t2 + 4 * fq + r;
        const bool in = ir < Tn;
        const float pv = in ? __expf(s[r] - lse[min(ir, Tn - 1)]) : 0.f;
        rt[t2][r] = for_q ? pv * (d[r] - delta[min(ir, Tn - 1)]) : pv;
      }
    }
    const V8T<T> rb = ma_pack<T>(rt[0], rt[1]);
    if (for_q) {
#pragma unroll
      for (int ct = 0; ct < MA_K / 16; ++ct) acc[ct] = mfma16<T>(ma_lds_frag<T>(mt, 16 * ct + fr, fq), rb, acc[ct]);
    } else {
#pragma unroll
      for (int ct = 0; ct < MA_CH / 16; ++ct) acc[ct] = mfma16<T>(ma_lds_frag<T>(mt, 16 * ct + fr, fq), rb, acc[ct]);
    }
  }
  if (j >= Tn) return;
  typedef typename Vec4<T>::type V4;
  T* out = for_q ? (T*)p.dq + (long long)n * p.dq_ss : (T*)p.dv + (long long)n * p.dv_ss;
#pragma unroll
  for (int ct = 0; ct < MA_CH / 16; ++ct) {
    if (for_q && ct >= MA_K / 16) break;
    const int c = c0 + 16 * ct + 4 * fq;
    V4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = from_f32<T>(acc[ct][r]);
    *(V4*)(out + ((long long)(c >> 3) * Tn + j) * 8 + (c & 7)) = o;
  }
}

// ---- squeeze-and-excitation gates.  s = 0: the branch on h (mean_h), s = 1: on the skip (mean_skip).
//   z_s = relu(W1_s mean_s + b1_s)  [m];  sig_s = sigmoid(W2_s z_s + b2_s)  [C];  g = sig_0 + sig_1
// hid: [N][2][m] (z), sig: [N][2][C].  One workgroup per sample; every dot product is a lane-strided sum and the wave's xor tree.
struct MaGate {
  const float* mean[2];
  const float* w1[2]; const float* b1[2]; const float* w2[2]; const float* b2[2];
  float* g; float* hid; float* sig;
  int C, m, N;
};

__global__ __launch_bounds__(256) void ma_gate_kernel(MaGate p) {
  const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* hid = p.hid + (long long)n * 2 * p.m;
  for (int u = wave; u < 2 * p.m; u += 4) {
    const int s = u / p.m, uu = u % p.m;
    float a = 0.f;
    for (int c = lane; c < p.C; c += 64) a = fmaf(p.w1[s][(long long)uu * p.C + c], p.mean[s][(long long)n * p.C + c], a);
    a = wave_sum(a);
    if (lane == 0) hid[u] = fmaxf(a + p.b1[s][uu], 0.f);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < p.C; c += 256) {
    float gs = 0.f;
    for (int s = 0; s < 2; ++s) {
      float a = p.b2[s][c];
      for (int u = 0; u < p.m; ++u) a = fmaf(p.w2[s][(long long)c * p.m + u], hid[s * p.m + u], a);
      const float sg = 1.f / (1.f + expf(-a));
      p.sig[((long long)n * 2 + s) * p.C + c] = sg;
      gs += sg;
    }
    p.g[(long long)n * p.C + c] = gs;
  }
}

struct MaGateBwd {
  const float* dg;
  const float* mean[2];
  const float* w1[2]; const float* w2[2];
  const float* hid; const float* sig;
  float* dhid;                                    // [N][2][m]: the gradient of the hidden pre-activations (workspace)
  float* dw1[2]; float* db1[2]; float* dw2[2]; float* db2[2];
  float* dmean[2];
  int C, m, N;
};

// One workgroup: da2[n][s][c] = dg sig (1 - sig) is recomputed where it is used; the sums over the batch run in sample order.
__global__ __launch_bounds__(256) void ma_gate_bwd_kernel(MaGateBwd p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, C = p.C, m = p.m;
  auto da2 = [&](int n, int s, int c) {
    const float sg = p.sig[((long long)n * 2 + s) * C + c];
    return p.dg[(long long)n * C + c] * sg * (1.f - sg);
  };
  for (int e = wave; e < p.N * 2 * m; e += 4) {            // dhid[n][s][u] = [z > 0] sum_c W2[c][u] da2[n][s][c]
    const int u = e % m, s = (e / m) % 2, n = e / (2 * m);
    float a = 0.f;
    for (int c = lane; c < C; c += 64) a = fmaf(p.w2[s][(long long)c * m + u], da2(n, s, c), a);
    a = wave_sum(a);
    if (lane == 0) p.dhid[e] = p.hid[e] > 0.f ? a : 0.f;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 2 * C * m; e += 256) {      // the two weight matrices of both branches
    const int s = e / (C * m), c = (e % (C * m)) / m, u = e % m;
    float a2 = 0.f, a1 = 0.f;
    for (int n = 0; n < p.N; ++n) {
      a2 = fmaf(da2(n, s, c), p.hid[((long long)n * 2 + s) * m + u], a2);
      a1 = fmaf(p.dhid[((long long)n * 2 + s) * m + u], p.mean[s][(long long)n * C + c], a1);
    }
    p.dw2[s][(long long)c * m + u] = a2;
    p.dw1[s][(long long)u * C + c] = a1;
  }
  for (int e = threadIdx.x; e < 2 * C; e += 256) {
    const int s = e / C, c = e % C;
    float a = 0.f;
    for (int n = 0; n < p.N; ++n) a += da2(n, s, c);
    p.db2[s][c] = a;
  }
  for (int e = threadIdx.x; e < 2 * m; e += 256) {
    const int s = e / m, u = e % m;
    float a = 0.f;
    for (int n = 0; n < p.N; ++n) a += p.dhid[((long long)n * 2 + s) * m + u];
    p.db1[s][u] = a;
  }
  for (int e = threadIdx.x; e < p.N * 2 * C; e += 256) {    // dmean[s][n][c] = sum_u W1[u][c] dhid[n][s][u]
    const int c = e % C, s = (e / C) % 2, n = e / (2 * C);
    float a = 0.f;
    for (int u = 0; u < m; ++u) a = fmaf(p.w1[s][(long long)u * C + c], p.dhid[((long long)n * 2 + s) * m + u], a);
    p.dmean[s][(long long)n * C + c] = a;
  }
}

// ---- gated nearest upsampling
// (channel groups: ChanGroup / group_load / group_store of resample.h; the prologue is norm_z<T, true>: iunet_bn_relu_fwd's bits)
struct MaUp {
  const void* h; long long h_ss;                  // on the coarse grid D H W
  const float* sc; const float* sh;               // prologue of h (or null)
  const float* g;                                 // [N][C]
  const void* du; long long du_ss;                // backward: the slot's gradient, on the fine grid
  const float* dmean;                             // backward: [N][C], the gradient of mean(h)
  void* out; long long out_ss;                    // forward: the slot (fine grid); backward: dh (coarse grid)
  int D, H, W, C, N;
};

// one thread = one channel group of one fine voxel
template <typename T, int ND, bool ACT>
__global__ __launch_bounds__(256) void ma_up_gate_kernel(MaUp p) {
  constexpr int G = ChanGroup<T>::G;
  const int Df = ND == 3 ? 2 * p.D : 1, Hf = 2 * p.H, Wf = 2 * p.W;
  const long long vF = (long long)Df * Hf * Wf, vC = (long long)p.D * p.H * p.W;
  const int groups = p.C / G;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)p.N * groups * vF) return;
  const long long r = i % vF;
  const int g = (int)((i / vF) % groups), n = (int)(i / (vF * groups));
  const int w = (int)(r % Wf), hh = (int)((r / Wf) % Hf), d = (int)(r / ((long long)Wf * Hf));
  const long long src = ((long long)(ND == 3 ? d >> 1 : 0) * p.H + (hh >> 1)) * p.W + (w >> 1);
  float v[G];
  group_load<T>((const T*)p.h + (long long)n * p.h_ss, g, src, vC, v);
#pragma unroll
  for (int j = 0; j < G; ++j) {
    if constexpr (ACT) v[j] = norm_z<T, true>(p.sc[g * G + j], v[j], p.sh[g * G + j]);
    v[j] *= p.g[(long long)n * p.C + g * G + j];
  }
  group_store<T>((T*)p.out + (long long)n * p.out_ss, g, r, vF, v);
}

// the sum of du over the 2^ND children of a coarse voxel, in (d, h, w) order
template <typename T, int ND>
__device__ __forceinline__ void ma_child_sum(const T* du, int g, int d, int hh, int w, int H, int W, long long vF, float (&s)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = 0.f;
  const int Hf = 2 * H, Wf = 2 * W;
#pragma unroll
  for (int kd = 0; kd < (ND == 3 ? 2 : 1); ++kd)
#pragma unroll
    for (int kh = 0; kh < 2; ++kh)
#pragma unroll
      for (int kw = 0; kw < 2; ++kw) {
        float t[8];
        group_load<T>(du, g, ((long long)(ND == 3 ? 2 * d + kd : 0) * Hf + 2 * hh + kh) * Wf + 2 * w + kw, vF, t);
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] += t[j];
      }
}

// dg[n][c] = sum over the fine grid of du up(h) = sum over the coarse grid of h (the children's sum): a workgroup per (sample, channel
// group, part of the grid); a thread's voxels in order, the wave's xor tree, the four waves in order, then (more than one part) the parts in
// order by ma_dg_sum_kernel
constexpr int MA_DG_VOX = 2048;      // coarse voxels per part: 8 per thread
constexpr int MA_DG_PARTS = 64;

inline int ma_dg_parts(long long vox) {
  const long long n = (vox + MA_DG_VOX - 1) / MA_DG_VOX;
  return (int)(n < 1 ? 1 : n > MA_DG_PARTS ? MA_DG_PARTS : n);
}

template <typename T, int ND, bool ACT>
__global__ __launch_bounds__(256) void ma_up_gate_dg_kernel(MaUp p, float* out) {
  const int g = blockIdx.x % (p.C / 8), n = blockIdx.x / (p.C / 8);
  const long long vC = (long long)p.D * p.H * p.W, vF = vC * (ND == 3 ? 8 : 4);
  const long long chunk = (vC + gridDim.y - 1) / gridDim.y, lo = blockIdx.y * chunk, hi = min(vC, lo + chunk);
  const T* h = (const T*)p.h + (long long)n * p.h_ss;
  const T* du = (const T*)p.du + (long long)n * p.du_ss;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (long long cv = lo + threadIdx.x; cv < hi; cv += 256) {
    const int w = (int)(cv % p.W), hh = (int)((cv / p.W) % p.H), d = (int)(cv / ((long long)p.W * p.H));
    float hv[8], s[8];
    group_load<T>(h, g, cv, vC, hv);
    ma_child_sum<T, ND>(du, g, d, hh, w, p.H, p.W, vF, s);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if constexpr (ACT) hv[j] = norm_z<T, true>(p.sc[g * 8 + j], hv[j], p.sh[g * 8 + j]);
      acc[j] = fmaf(hv[j], s[j], acc[j]);
    }
  }
  __shared__ float red[4][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float s = wave_sum(acc[j]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][j] = s;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int j = threadIdx.x;
    out[((long long)blockIdx.y * p.N + n) * p.C + g * 8 + j] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
  }
}

__global__ __launch_bounds__(256) void ma_dg_sum_kernel(const float* __restrict__ part, float* __restrict__ dg, int parts, int NC) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= NC) return;
  float s = 0.f;
  for (int k = 0; k < parts; ++k) s += part[(long long)k * NC + i];
  dg[i] = s;
}

// dh[coarse] = g (the children's sum of du) + dmean_h / vox: one thread per (coarse voxel, channel group)
template <typename T, int ND>
__global__ __launch_bounds__(256) void ma_up_gate_bwd_kernel(MaUp p) {
  const long long vC = (long long)p.D * p.H * p.W, vF = vC * (ND == 3 ? 8 : 4);
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)p.N * (p.C / 8) * vC) return;
  const long long cv = i % vC;
  const int g = (int)((i / vC) % (p.C / 8)), n = (int)(i / (vC * (p.C / 8)));
  const int w = (int)(cv % p.W), hh = (int)((cv / p.W) % p.H), d = (int)(cv / ((long long)p.W * p.H));
  float s[8];
  ma_child_sum<T, ND>((const T*)p.du + (long long)n * p.du_ss, g, d, hh, w, p.H, p.W, vF, s);
  const float inv = 1.f / (float)vC;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const long long nc = (long long)n * p.C + g * 8 + j;
    s[j] = fmaf(p.g[nc], s[j], p.dmean != nullptr ? p.dmean[nc] * inv : 0.f);
  }
  group_store<T>((T*)p.out + (long long)n * p.out_ss, g, cv, vC, s);
}

// dx[n][c][v] += dmean[n][c] / vox (the skip's share of its gate's gradient)
template <typename T>
__global__ __launch_bounds__(256) void ma_add_mean_kernel(T* dx, long long dx_ss, const float* __restrict__ dmean, int C, int N, long long vox) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)N * (C / 8) * vox) return;
  const long long v = i % vox;
  const int g = (int)((i / vox) % (C / 8)), n = (int)(i / (vox * (C / 8)));
  float a[8];
  group_load<T>(dx + (long long)n * dx_ss, g, v, vox, a);
  const float inv = 1.f / (float)vox;
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = fmaf(dmean[(long long)n * C + g * 8 + j], inv, a[j]);
  group_store<T>(dx + (long long)n * dx_ss, g, v, vox, a);
}

int ma_check_attn(const char* what, int Cb, int T, int N) {
  IUNET_REQUIRE(Cb > 0 && Cb % MA_CH == 0 && Cb <= 512, "%s: Cb %d (a multiple of %d up to 512)", what, Cb, MA_CH);
  IUNET_REQUIRE(T > 0 && T <= MA_MAX_T, "%s: T %d tokens (1 .. %d)", what, T, MA_MAX_T);
  IUNET_REQUIRE(N > 0 && N < 65536, "%s: N %d", what, N);
  return IUNET_OK;
}

int ma_check_grid(const char* what, int nd, int N, int D, int H, int W, int C, int mult) {
  IUNET_REQUIRE(nd == 2 || nd == 3, "%s: nd must be 2 or 3, got %d", what, nd);
  IUNET_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && (nd == 3 || D == 1), "%s: bad grid N %d, %d x %d x %d (D = 1 in 2-D)", what, N, D, H, W);
  IUNET_REQUIRE((long long)D * H * W < (1ll << 27) && D < (1 << 20) && H < (1 << 20) && W < (1 << 20), "%s: grid %d x %d x %d is too large", what,
                D, H, W);
  IUNET_REQUIRE(C > 0 && C % mult == 0, "%s: C %d (a positive multiple of %d)", what, C, mult);
  return IUNET_OK;
}

int ma_attn_launch(int dtype, const char* what, const void* q, long long q_ss, const void* bq, const void* k, long long k_ss, const void* bk,
                   const void* v, long long v_ss, const void* x, long long x_ss, const void* bv, void* y, long long y_ss, void* lse, int Cb, int T,
                   int N, void* stream) {
  const int rc = ma_check_attn(what, Cb, T, N);
  if (rc != IUNET_OK) return rc;
  IUNET_REQUIRE(q && bq && k && bk && v && x && bv && y && lse, "%s: null pointer", what);
  MaAttn p;
  p.q = q; p.q_ss = q_ss; p.bq = (const float*)bq; p.k = k; p.k_ss = k_ss; p.bk = (const float*)bk; p.v = v; p.v_ss = v_ss;
  p.x = x; p.x_ss = x_ss; p.bv = (const float*)bv; p.y = y; p.y_ss = y_ss; p.lse = (float*)lse; p.Cb = Cb; p.T = T; p.N = N;
  const dim3 grid((T + MA_OWN - 1) / MA_OWN, Cb / MA_CH, N);
  if (dtype == 0) hipLaunchKernelGGL(ma_attn_fwd_kernel<f16>, grid, dim3(256), 0, (hipStream_t)stream, p);
  else if (dtype == 1) hipLaunchKernelGGL(ma_attn_fwd_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(ma_f32_attn_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

// the row launch of the backward, by Cb / 128 (ma_check_attn: 1 .. 4): the owned dY fragments are a register array of Cb / 32
template <typename T>
void ma_rows_launch(const MaAttnBwd& p, int blocks, hipStream_t stream) {
  const dim3 grid(blocks, 1, p.N);
  switch (p.Cb / MA_CH) {
    case 1: hipLaunchKernelGGL((ma_attn_rows_kernel<T, 4>), grid, dim3(256), 0, stream, p); break;
    case 2: hipLaunchKernelGGL((ma_attn_rows_kernel<T, 8>), grid, dim3(256), 0, stream, p); break;
    case 3: hipLaunchKernelGGL((ma_attn_rows_kernel<T, 12>), grid, dim3(256), 0, stream, p); break;
    default: hipLaunchKernelGGL((ma_attn_rows_kernel<T, 16>), grid, dim3(256), 0, stream, p); break;
  }
}

}  // namespace

extern "C" {

int iunet_ma_attn_fwd(int dtype, const void* q, long long q_ss, const void* bq, const void* k, long long k_ss, const void* bk, const void* v,
                      long long v_ss, const void* x, long long x_ss, const void* bv, void* y, long long y_ss, void* lse, int Cb, int T, int N,
                      void* stream) {
  IUNET_REQUIRE(dtype == 0 || dtype == 1, "ma_attn_fwd: dtype must be 0 (f16) or 1 (bf16), got %d", dtype);
  return ma_attn_launch(dtype, "ma_attn_fwd", q, q_ss, bq, k, k_ss, bk, v, v_ss, x, x_ss, bv, y, y_ss, lse, Cb, T, N, stream);
}

int iunet_ma_f32_attn_fwd(const void* q, long long q_ss, const void* bq, const void* k, long long k_ss, const void* bk, const void* v,
                          long long v_ss, const void* x, long long x_ss, const void* bv, void* y, long long y_ss, void* lse, int Cb, int T, int N,
                          void* stream) {
  return ma_attn_launch(2, "ma_f32_attn_fwd", q, q_ss, bq, k, k_ss, bk, v, v_ss, x, x_ss, bv, y, y_ss, lse, Cb, T, N, stream);
}

int iunet_ma_attn_bwd(int dtype, const void* q, long long q_ss, const void* bq, const void* k, long long k_ss, const void* bk, const void* v,
                      long long v_ss, const void* dy, long long dy_ss, const void* lse, void* delta, void* dq, long long dq_ss, void* dk,
                      long long dk_ss, void* dv, long long dv_ss, int Cb, int T, int N, void* stream) {
  IUNET_REQUIRE(dtype == 0 || dtype == 1, "ma_attn_bwd: dtype must be 0 (f16) or 1 (bf16), got %d", dtype);
  const int rc = ma_check_attn("ma_attn_bwd", Cb, T, N);
  if (rc != IUNET_OK) return rc;
  IUNET_REQUIRE(q && bq && k && bk && v && dy && lse && delta && dq && dk && dv, "ma_attn_bwd: null pointer");
  MaAttnBwd p;
  p.q = q; p.q_ss = q_ss; p.bq = (const float*)bq; p.k = k; p.k_ss = k_ss; p.bk = (const float*)bk; p.v = v; p.v_ss = v_ss;
  p.dy = dy; p.dy_ss = dy_ss; p.lse = (const float*)lse; p.delta = (float*)delta; p.dq = dq; p.dq_ss = dq_ss; p.dk = dk; p.dk_ss = dk_ss;
  p.dv = dv; p.dv_ss = dv_ss; p.Cb = Cb; p.T = T; p.N = N;
  const int blocks = (T + MA_OWN - 1) / MA_OWN;
  if (dtype == 0) {
    ma_rows_launch<f16>(p, blocks, (hipStream_t)stream);
    hipLaunchKernelGGL(ma_attn_cols_kernel<f16>, dim3(blocks, Cb / MA_CH + 1, N), dim3(256), 0, (hipStream_t)stream, p);
  } else {
    ma_rows_launch<bf16>(p, blocks, (hipStream_t)stream);
    hipLaunchKernelGGL(ma_attn_cols_kernel<bf16>, dim3(blocks, Cb / MA_CH + 1, N), dim3(256), 0, (hipStream_t)stream, p);
  }
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_ma_gate(const void* mean_h, const void* mean_skip, const void* w1_hl, const void* b1_hl, const void* w2_hl, const void* b2_hl,
                  const void* w1_ll, const void* b1_ll, const void* w2_ll, const void* b2_ll, void* g, void* hid, void* sig, int C, int m, int N,
                  void* stream) {
  IUNET_REQUIRE(C > 0 && m > 0 && N > 0 && m <= C, "ma_gate: C %d, m %d, N %d", C, m, N);
  IUNET_REQUIRE(mean_h && mean_skip && w1_hl && b1_hl && w2_hl && b2_hl && w1_ll && b1_ll && w2_ll && b2_ll && g && hid && sig,
                "ma_gate: null pointer");
  MaGate p;
  p.mean[0] = (const float*)mean_h; p.mean[1] = (const float*)mean_skip;
  p.w1[0] = (const float*)w1_hl; p.b1[0] = (const float*)b1_hl; p.w2[0] = (const float*)w2_hl; p.b2[0] = (const float*)b2_hl;
  p.w1[1] = (const float*)w1_ll; p.b1[1] = (const float*)b1_ll; p.w2[1] = (const float*)w2_ll; p.b2[1] = (const float*)b2_ll;
  p.g = (float*)g; p.hid = (float*)hid; p.sig = (float*)sig; p.C = C; p.m = m; p.N = N;
  hipLaunchKernelGGL(ma_gate_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, p);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_ma_gate_bwd(const void* dg, const void* mean_h, const void* mean_skip, const void* w1_hl, const void* w2_hl, const void* w1_ll,
                      const void* w2_ll, const void* hid, const void* sig, void* dhid, void* dw1_hl, void* db1_hl, void* dw2_hl, void* db2_hl,
                      void* dw1_ll, void* db1_ll, void* dw2_ll, void* db2_ll, void* dmean_h, void* dmean_skip, int C, int m, int N, void* stream) {
  IUNET_REQUIRE(C > 0 && m > 0 && N > 0 && m <= C, "ma_gate_bwd: C %d, m %d, N %d", C, m, N);
  IUNET_REQUIRE(dg && mean_h && mean_skip && w1_hl && w2_hl && w1_ll && w2_ll && hid && sig && dhid && dw1_hl && db1_hl && dw2_hl && db2_hl &&
                    dw1_ll && db1_ll && dw2_ll && db2_ll && dmean_h && dmean_skip,
                "ma_gate_bwd: null pointer");
  MaGateBwd p;
  p.dg = (const float*)dg; p.mean[0] = (const float*)mean_h; p.mean[1] = (const float*)mean_skip;
  p.w1[0] = (const float*)w1_hl; p.w2[0] = (const float*)w2_hl; p.w1[1] = (const float*)w1_ll; p.w2[1] = (const float*)w2_ll;
  p.hid = (const float*)hid; p.sig = (const float*)sig; p.dhid = (float*)dhid;
  p.dw1[0] = (float*)dw1_hl; p.db1[0] = (float*)db1_hl; p.dw2[0] = (float*)dw2_hl; p.db2[0] = (float*)db2_hl;
  p.dw1[1] = (float*)dw1_ll; p.db1[1] = (float*)db1_ll; p.dw2[1] = (float*)dw2_ll; p.db2[1] = (float*)db2_ll;
  p.dmean[0] = (float*)dmean_h; p.dmean[1] = (float*)dmean_skip; p.C = C; p.m = m; p.N = N;
  hipLaunchKernelGGL(ma_gate_bwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, p);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_ma_up_gate(int dtype, int nd, const void* h, long long h_ss, const void* scale, const void* shift, const void* g, void* dst,
                     long long dst_ss, int D, int H, int W, int C, int N, void* stream) {
  IUNET_REQUIRE(dtype >= 0 && dtype <= 2, "ma_up_gate: dtype must be 0 (f16), 1 (bf16) or 2 (planar f32), got %d", dtype);
  const int rc = ma_check_grid("ma_up_gate", nd, N, D, H, W, C, 8);
  if (rc != IUNET_OK) return rc;
  IUNET_REQUIRE(h && g && dst, "ma_up_gate: null pointer");
  IUNET_REQUIRE(!scale == !shift, "ma_up_gate: the activation needs both scale and shift");
  MaUp p = {};
  p.h = h; p.h_ss = h_ss; p.sc = (const float*)scale; p.sh = (const float*)shift; p.g = (const float*)g; p.out = dst; p.out_ss = dst_ss;
  p.D = D; p.H = H; p.W = W; p.C = C; p.N = N;
  const long long total = (long long)N * (dtype == 2 ? C : C / 8) * D * H * W * (nd == 3 ? 8 : 4);
  IUNET_REQUIRE(total < (1ll << 31), "ma_up_gate: %lld items exceed one launch", total);
  const dim3 grid((unsigned)((total + 255) / 256));
  iunet_dispatch<true>(dtype, nd, scale != nullptr, [&](auto t, auto ndc, auto act) {
    hipLaunchKernelGGL((ma_up_gate_kernel<decltype(t), ndc.value, act.value>), grid, dim3(256), 0, (hipStream_t)stream, p);
  });
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_ma_up_gate_dg_parts(int nd, int N, int D, int H, int W, int C) {
  const int rc = ma_check_grid("ma_up_gate_dg_parts", nd, N, D, H, W, C, 8);
  if (rc != IUNET_OK) return rc;
  return ma_dg_parts((long long)D * H * W);
}

int iunet_ma_up_gate_dg(int dtype, int nd, const void* du, long long du_ss, const void* h, long long h_ss, const void* scale, const void* shift,
                        void* part, void* dg, int D, int H, int W, int C, int N, void* stream) {
  IUNET_REQUIRE(dtype == 0 || dtype == 1, "ma_up_gate_dg: dtype must be 0 (f16) or 1 (bf16), got %d", dtype);
  const int rc = ma_check_grid("ma_up_gate_dg", nd, N, D, H, W, C, 8);
  if (rc != IUNET_OK) return rc;
  const int parts = ma_dg_parts((long long)D * H * W);
  IUNET_REQUIRE(du && h && dg && (part || parts == 1), "ma_up_gate_dg: null pointer");
  IUNET_REQUIRE(!scale == !shift, "ma_up_gate_dg: the activation needs both scale and shift");
  IUNET_REQUIRE((long long)N * C < (1ll << 30), "ma_up_gate_dg: N %d x C %d exceed one launch", N, C);
  MaUp p = {};
  p.h = h; p.h_ss = h_ss; p.sc = (const float*)scale; p.sh = (const float*)shift; p.du = du; p.du_ss = du_ss;
  p.D = D; p.H = H; p.W = W; p.C = C; p.N = N;
  float* out = parts == 1 ? (float*)dg : (float*)part;
  iunet_dispatch(dtype, nd, scale != nullptr, [&](auto t, auto ndc, auto act) {
    hipLaunchKernelGGL((ma_up_gate_dg_kernel<decltype(t), ndc.value, act.value>), dim3((unsigned)(N * (C / 8)), parts), dim3(256), 0,
                       (hipStream_t)stream, p, out);
  });
  if (parts > 1)
    hipLaunchKernelGGL(ma_dg_sum_kernel, dim3((N * C + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)part, (float*)dg, parts, N * C);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_ma_up_gate_bwd(int dtype, int nd, const void* du, long long du_ss, const void* g, const void* dmean_h, void* dh, long long dh_ss, int D,
                         int H, int W, int C, int N, void* stream) {
  IUNET_REQUIRE(dtype == 0 || dtype == 1, "ma_up_gate_bwd: dtype must be 0 (f16) or 1 (bf16), got %d", dtype);
  const int rc = ma_check_grid("ma_up_gate_bwd", nd, N, D, H, W, C, 8);
  if (rc != IUNET_OK) return rc;
  IUNET_REQUIRE(du && g && dh, "ma_up_gate_bwd: null pointer");
  MaUp p = {};
  p.du = du; p.du_ss = du_ss; p.g = (const float*)g; p.dmean = (const float*)dmean_h; p.out = dh; p.out_ss = dh_ss;
  p.D = D; p.H = H; p.W = W; p.C = C; p.N = N;
  const long long total = (long long)N * (C / 8) * D * H * W;
  IUNET_REQUIRE(total < (1ll << 31), "ma_up_gate_bwd: %lld items exceed one launch", total);
  const dim3 grid((unsigned)((total + 255) / 256));
  iunet_dispatch(dtype, nd, false, [&](auto t, auto ndc, auto) {
    hipLaunchKernelGGL((ma_up_gate_bwd_kernel<decltype(t), ndc.value>), grid, dim3(256), 0, (hipStream_t)stream, p);
  });
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_ma_add_mean_grad(int dtype, void* dx, long long dx_ss, const void* dmean, int C, int N, long long vox, void* stream) {
  IUNET_REQUIRE(dtype == 0 || dtype == 1, "ma_add_mean_grad: dtype must be 0 (f16) or 1 (bf16), got %d", dtype);
  IUNET_REQUIRE(dx && dmean, "ma_add_mean_grad: null pointer");
  IUNET_REQUIRE(C > 0 && C % 8 == 0 && N > 0 && vox > 0 && vox < (1ll << 30), "ma_add_mean_grad: C %d (multiple of 8), N %d, %lld voxels", C, N, vox);
  const long long total = (long long)N * (C / 8) * vox;
  IUNET_REQUIRE(total < (1ll << 31), "ma_add_mean_grad: %lld items exceed one launch", total);
  const dim3 grid((unsigned)((total + 255) / 256));
  iunet_dispatch(dtype, 2, false, [&](auto t, auto, auto) {
    using T = decltype(t);
    hipLaunchKernelGGL(ma_add_mean_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, (T*)dx, dx_ss, (const float*)dmean, C, N, vox);
  });
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

}  // extern "C"
