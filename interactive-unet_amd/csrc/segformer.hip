// Segformer decoder (Xie et al. 2021, smp's SegformerDecoder on this project's encoder), on the target grid T = the input grid / 4:
//   P_l = W_l X^l + b_l (per voxel), R_l = resize of level l's grid to T (linear, align_corners=False), concat deepest first,
//   Z = W_f concat (1x1, no bias), F = relu(bn(Z)), logits_T = head(F), logits = x4 (align_corners=True), softmax.
//
// Every step up to Z is linear and interpolation weights sum to 1 (also where the borders clamp), so with W_f,l the block of the fuse
// operator that reads level l:
//   Z = sum_l M_l R_l(X^l) + beta,   M_l = W_f,l W_l,   beta = sum_l W_f,l b_l.
// The forward is ONE GEMM [C] x [K = sum ch[l]] whose B operand is gathered resampled straight out of the encoder tensors: no C-channel
// tensor finer than T and no L C-channel concat ever exists.  The backward follows from the same identity (dZ from fuse.bn's backward,
// r = sum over (n, t) of dZ):
//   G_l = dZ R_l(X^l)^T (gather_gemm.h's staged weight gradient under the SfResample policy), dW_l = W_f,l^T G_l,
//   dW_f,l = G_l W_l^T + r b_l^T, db_l = W_f,l^T r (sf_param_grad_kernel),
//   dX^l = R_l^T(M_l^T dZ) (M^T dZ by iunet_dl_conv_fwd at rate 0 with the transposed operator, R^T by iunet_sf_adjoint).
//
// Resampling: resample_axis_f32 and the tap walk of resample.h.  The sources are the encoder's NHWC8c tensors (16-bit) or planar fp32
// tensors, each with its own grid: the kernels take any source grid, so the ratios -2 .. +3 of the network and odd grids are one code
// path.  The taps are rounded once to the MFMA input type.  An optional per-source relu(scale x + shift) prologue applies a BatchNorm +
// ReLU to each tap with iunet_bn_relu_fwd's bits before weighting it.
//
// All reductions are fixed-order (per-workgroup rows / slabs, then ordered sums): no float atomics, two identical calls are bit-identical.
#include <type_traits>

#include "common.h"
#include "gather_gemm.h"
#include "resample.h"

namespace {

constexpr int SF_MAXS = 6;           // sources (levels) per launch
constexpr int SF_COLS = 64;          // output voxels per workgroup of the forward GEMM
constexpr int SF_MAXC = 512;         // output channels (all of them in one workgroup: the gathered tile is built once)
constexpr int SF_LD16 = 40;          // LDS row stride (elements) of a [rows][32] 16-bit operand image
constexpr int SF_LD32 = 36;          // ... of a [rows][32] fp32 image

struct SfSrc {
  const void* x; long long x_ss;     // NHWC8c (16-bit) or planar [C][vox] (fp32), sample stride in elements
  const float* sc; const float* sh;  // optional relu(sc x + sh) prologue
  int C, koff;                       // channels, first operator column
  int D, H, W;                       // the source's grid
};

struct SfSrcs {
  int n;
  SfSrc s[SF_MAXS];
};

// The 8 channels c0 .. c0 + 7 of source s resampled at the T voxel whose per-axis taps are ad / ah / aw (fp32 sum, fixed tap order)
template <typename T, int ND, bool ACT>
__device__ __forceinline__ void sf_sample(const SfSrc& s, int n, int c0, const ResampleAx& ad, const ResampleAx& ah, const ResampleAx& aw,
                                          float out[8]) {
  constexpr int G = ChanGroup<T>::G;
#pragma unroll
  for (int j = 0; j < 8; ++j) out[j] = 0.f;
  const long long vs = (long long)s.D * s.H * s.W;
  const T* xs = (const T*)s.x + (long long)n * s.x_ss + (long long)c0 * vs;          // channel c0's plane / group in both layouts
  resample_taps<ND>(ad, ah, aw, s.H, s.W, [&](long long vox, float wgt) {
#pragma unroll
    for (int g = 0; g < 8 / G; ++g) {              // one 16-byte group, or eight planes
      float v[G];
      group_load<T>(xs, g, vox, vs, v);
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const int c = g * G + j;
        if constexpr (ACT) v[j] = norm_z<T, true>(s.sc[c0 + c], v[j], s.sh[c0 + c]);
        out[c] = fmaf(wgt, v[j], out[c]);
      }
    }
  });
}

struct SfGemm {
  SfSrcs src;
  const void* wpk; int K;            // operator [Cout][K], K = sum of the sources' channels
  const float* bias;                 // [Cout]: beta (epi 0) or the folded eval bias (epi 1)
  void* y; long long y_ss;           // Z (epi 0) / F (epi 1) on T: NHWC8c T or planar fp32
  float* stats;                      // [gridDim.x][Cout][2] or null (epi 0)
  int D, H, W;                       // T
  int Cout, epi;
  long long cols;
};

// One workgroup = 64 T voxels x all Cout rows.  Per chunk of 32 operator columns (one source's channels) its 256 threads gather the
// resampled B tile [64 voxels][32] (one 8-channel group of one voxel each) and copy the operator chunk [Cout][32] into LDS; wave w then
// runs row tiles w, w + 4, ... against the 4 column tiles, both operands read from LDS.
template <typename T, int ND, bool ACT>
__global__ __launch_bounds__(256) void sf_gemm_kernel(SfGemm p) {
  constexpr bool F32 = std::is_same<T, float>::value;
  constexpr int LD = F32 ? SF_LD32 : SF_LD16;
  extern __shared__ __attribute__((aligned(16))) unsigned char sf_smem[];
  T* sB = (T*)sf_smem;                                 // [64][LD]
  T* sA = sB + SF_COLS * LD;                           // [Cout][LD]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, l15 = lane & 15;
  const long long vT = (long long)p.D * p.H * p.W;
  const int ntile = p.Cout / 16;
  // this thread's gather slot: voxel gc, channel group gg of the chunk
  const int gc = threadIdx.x & 63, gg = threadIdx.x >> 6;
  const long long gcol = (long long)blockIdx.x * SF_COLS + gc;
  const bool gok = gcol < p.cols;
  const long long gcc = gok ? gcol : 0;
  const int gn = (int)(gcc / vT);
  const long long gr = gcc - (long long)gn * vT;
  const int gw = (int)(gr % p.W), gh = (int)((gr / p.W) % p.H), gd = (int)(gr / ((long long)p.W * p.H));
  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int si = 0; si < p.src.n; ++si) {
    const SfSrc& s = p.src.s[si];
    ResampleAx ad, ah, aw;
    ad = ND == 3 ? resample_axis_f32(gd, p.D, s.D) : ResampleAx{0, 0, 0.f};
    ah = resample_axis_f32(gh, p.H, s.H);
    aw = resample_axis_f32(gw, p.W, s.W);
    for (int c0 = 0; c0 < s.C; c0 += 32) {
      float v[8];
      if (gok) {
        sf_sample<T, ND, ACT>(s, gn, c0 + gg * 8, ad, ah, aw, v);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = 0.f;
      }
      __syncthreads();                                 // the previous chunk's operands are consumed
      if constexpr (F32) {
#pragma unroll
        for (int j = 0; j < 8; ++j) sB[gc * LD + gg * 8 + j] = v[j];
        const float* wk = (const float*)p.wpk + s.koff + c0;
        for (int e = threadIdx.x; e < p.Cout * 8; e += 256) {
          const int row = e >> 3, kk = (e & 7) * 4;
          *(f32x4*)(sA + row * LD + kk) = *(const f32x4*)(wk + (long long)row * p.K + kk);
        }
      } else {
        V8T<T> b;
#pragma unroll
        for (int j = 0; j < 8; ++j) b[j] = from_f32<T>(v[j]);
        *(V8T<T>*)(sB + gc * LD + gg * 8) = b;
        const T* wk = (const T*)p.wpk + s.koff + c0;
        for (int e = threadIdx.x; e < p.Cout * 4; e += 256) {
          const int row = e >> 2, kk = (e & 3) * 8;
          *(V8T<T>*)(sA + row * LD + kk) = *(const V8T<T>*)(wk + (long long)row * p.K + kk);
        }
      }
      __syncthreads();
      if constexpr (F32) {
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
          float bv[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) bv[t] = sB[(t * 16 + l15) * LD + ks * 4 + q];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const int a = wave + 4 * i;
            if (a < ntile) {
              const float av = sA[(a * 16 + l15) * LD + ks * 4 + q];
#pragma unroll
              for (int t = 0; t < 4; ++t) acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[t], acc[i][t], 0, 0, 0);
            }
          }
        }
      } else {
        V8T<T> bv[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) bv[t] = *(const V8T<T>*)(sB + (t * 16 + l15) * LD + q * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int a = wave + 4 * i;
          if (a < ntile) {
            const V8T<T> av = *(const V8T<T>*)(sA + (a * 16 + l15) * LD + q * 8);
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[i][t] = mfma16<T>(av, bv[t], acc[i][t]);
          }
        }
      }
    }
  }
  // epilogue: lane holds rows a*16 + q*4 + rr at column tile t, voxel l15
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int a = wave + 4 * i;
    if (a >= ntile) continue;
    const int co = a * 16 + q * 4;
    float ssum[4] = {0.f, 0.f, 0.f, 0.f}, ssq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const long long col = (long long)blockIdx.x * SF_COLS + t * 16 + l15;
      if (col >= p.cols) continue;
      const int n = (int)(col / vT);
      const long long r = col - (long long)n * vT;
      float o[4];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const float v = acc[i][t][rr] + p.bias[co + rr];
        if (p.epi == 0) {
          o[rr] = v;
          ssum[rr] += v;
          ssq[rr] += v * v;
        } else {
          o[rr] = fmaxf(v, 0.f);
        }
      }
      if constexpr (F32) {
        float* ys = (float*)p.y + (long long)n * p.y_ss + r;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) ys[(long long)(co + rr) * vT] = o[rr];
      } else {
        typename Vec4<T>::type ov;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) ov[rr] = from_f32<T>(o[rr]);
        *(typename Vec4<T>::type*)((T*)p.y + (long long)n * p.y_ss + ((long long)(co >> 3) * vT + r) * 8 + (co & 7)) = ov;
      }
    }
    if (p.stats != nullptr) {
      // the 16 voxels of a lane group (a fixed butterfly): one row per workgroup; each wave owns its rows
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        float s = ssum[rr], s2 = ssq[rr];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) { s += __shfl_xor(s, o); s2 += __shfl_xor(s2, o); }
        if (l15 == 0) {
          p.stats[((long long)blockIdx.x * p.Cout + co + rr) * 2] = s;
          p.stats[((long long)blockIdx.x * p.Cout + co + rr) * 2 + 1] = s2;
        }
      }
    }
  }
}

// ---- weight gradient G[Cout][K] = sum over (n, t) of dZ[co] R(X)[k]: gather_gemm.h's weight-gradient policy, B[k] = the source that
// owns operator column k, resampled at the T voxel
template <int ND>
struct SfResample {
  SfSrcs src;
  struct Lane { const SfSrc* s; int c0; };
  __device__ __forceinline__ Lane lane(int k_l, bool k_ok) const {
    int si = 0;
    if (k_ok)
      while (si + 1 < src.n && k_l >= src.s[si + 1].koff) ++si;
    return Lane{&src.s[si], k_l - src.s[si].koff};
  }
  template <typename T, bool ACT>
  __device__ __forceinline__ V8T<T> column(const Lane& l, int n, long long r, int D, int H, int W) const {
    const int w = (int)(r % W), h = (int)((r / W) % H), d = (int)(r / ((long long)W * H));
    const ResampleAx ad = ND == 3 ? resample_axis_f32(d, D, l.s->D) : ResampleAx{0, 0, 0.f};
    const ResampleAx ah = resample_axis_f32(h, H, l.s->H), aw = resample_axis_f32(w, W, l.s->W);
    float v[8];
    sf_sample<T, ND, ACT>(*l.s, n, l.c0, ad, ah, aw, v);
    V8T<T> vb;
#pragma unroll
    for (int j = 0; j < 8; ++j) vb[j] = from_f32<T>(v[j]);
    return vb;
  }
};

__global__ __launch_bounds__(256) void sf_wgrad_reduce_kernel(const float* __restrict__ slab, int splits, long long total, float* __restrict__ G) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  float s = 0.f;
  for (int sp = 0; sp < splits; ++sp) s += slab[(long long)sp * total + i];
  G[i] = s;
}

// ---- the small fp32 operator kernels (C^2 sum ch MACs; one thread per output, sums in ascending index order)
struct SfOps {
  const float* wf;                   // fuse.conv.weight [C][L C] (block j reads level L-1-j)
  const float* w[SF_MAXS];           // mlp{l}.weight [C][ch[l]]
  const float* b[SF_MAXS];           // mlp{l}.bias [C]
  int ch[SF_MAXS], koff[SF_MAXS];
  int L, C, K;
};

__device__ __forceinline__ int sf_level(const SfOps& o, int k) {
  int l = 0;
  while (l + 1 < o.L && k >= o.koff[l + 1]) ++l;
  return l;
}

// dst[c][k] = s_c sum_j W_f,l[c][j] W_l[j][k - koff_l] (s_c = the eval BatchNorm scale or 1); dstT[k][c] = the unscaled value;
// bias[c] = beta_c (no fold) or s_c (beta_c - mean_c) + bn.bias_c
template <typename OT>
__global__ __launch_bounds__(256) void sf_pack_kernel(SfOps o, const float* gamma, const float* bnb, const float* mean, const float* var, float eps,
                                                      OT* __restrict__ dst, OT* dstT, float* bias) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long nop = (long long)o.C * o.K;
  if (i < nop) {
    const int c = (int)(i / o.K), k = (int)(i - (long long)c * o.K);
    const int l = sf_level(o, k), kk = k - o.koff[l];
    const float* wf = o.wf + (long long)c * o.L * o.C + (long long)(o.L - 1 - l) * o.C;
    float s = 0.f;
    for (int j = 0; j < o.C; ++j) s = fmaf(wf[j], o.w[l][(long long)j * o.ch[l] + kk], s);
    const float sc = gamma != nullptr ? bn_fold_scale(gamma, var, eps, c) : 1.f;
    dst[i] = (OT)(s * sc);
    if (dstT != nullptr) dstT[(long long)k * o.C + c] = (OT)s;
  } else if (i < nop + o.C && bias != nullptr) {
    const int c = (int)(i - nop);
    float s = 0.f;
    for (int l = 0; l < o.L; ++l) {
      const float* wf = o.wf + (long long)c * o.L * o.C + (long long)(o.L - 1 - l) * o.C;
      for (int j = 0; j < o.C; ++j) s = fmaf(wf[j], o.b[l][j], s);
    }
    if (gamma != nullptr) {
      const float sc = bn_fold_scale(gamma, var, eps, c);
      s = sc * (s - mean[c]) + bnb[c];
    }
    bias[c] = s;
  }
}

// dW_l[j][k] = sum_c W_f,l[c][j] G[c][koff_l + k];  dW_f[c][(L-1-l) C + j] = sum_k G[c][koff_l + k] W_l[j][k] + r[c] b_l[j];
// db_l[j] = sum_c W_f,l[c][j] r[c];  r[c] = sum_n rs[n][c] (ascending n)
struct SfGrads {
  float* dw[SF_MAXS];
  float* db[SF_MAXS];
  float* dwf;
};

__global__ __launch_bounds__(256) void sf_param_grad_kernel(SfOps o, SfGrads g, const float* __restrict__ G, const float* __restrict__ rs, int N) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n1 = (long long)o.C * o.K, n2 = n1 + (long long)o.C * o.L * o.C, n3 = n2 + (long long)o.L * o.C;
  const int LC = o.L * o.C;
  if (i < n1) {
    const int j = (int)(i / o.K), k = (int)(i - (long long)j * o.K);
    const int l = sf_level(o, k), kk = k - o.koff[l];
    const int col = (o.L - 1 - l) * o.C + j;
    float s = 0.f;
    for (int c = 0; c < o.C; ++c) s = fmaf(o.wf[(long long)c * LC + col], G[(long long)c * o.K + k], s);
    g.dw[l][(long long)j * o.ch[l] + kk] = s;
  } else if (i < n2) {
    const long long e = i - n1;
    const int c = (int)(e / LC), colj = (int)(e - (long long)c * LC);
    const int l = o.L - 1 - colj / o.C, j = colj % o.C;
    float s = 0.f;
    const float* gr = G + (long long)c * o.K + o.koff[l];
    const float* wl = o.w[l] + (long long)j * o.ch[l];
    for (int k = 0; k < o.ch[l]; ++k) s = fmaf(gr[k], wl[k], s);
    float r = 0.f;
    for (int n = 0; n < N; ++n) r += rs[(long long)n * o.C + c];
    g.dwf[e] = fmaf(r, o.b[l][j], s);
  } else if (i < n3) {
    const long long e = i - n2;
    const int l = (int)(e / o.C), j = (int)(e % o.C);
    const int col = (o.L - 1 - l) * o.C + j;
    float s = 0.f;
    for (int c = 0; c < o.C; ++c) {
      float r = 0.f;
      for (int n = 0; n < N; ++n) r += rs[(long long)n * o.C + c];
      s = fmaf(o.wf[(long long)c * LC + col], r, s);
    }
    g.db[l][j] = s;
  }
}

// ---- host-side argument checks shared by the entry points
int sf_check_t(int nd, int N, int D, int H, int W) {
  IUNET_REQUIRE(nd == 2 || nd == 3, "segformer: nd must be 2 or 3, got %d", nd);
  IUNET_REQUIRE_GRID("segformer", N, D, H, W);
  IUNET_REQUIRE(nd == 3 || D == 1, "segformer: 2-D tensors have D = 1");
  return IUNET_OK;
}

int sf_build_srcs(SfSrcs& S, int nd, int nsrc, const void* const* x, const long long* x_ss, const int* cin, const int* dims,
                  const void* const* sc, const void* const* sh, bool& act) {
  IUNET_REQUIRE(nsrc >= 1 && nsrc <= SF_MAXS, "segformer: 1 .. %d sources, got %d", SF_MAXS, nsrc);
  IUNET_REQUIRE(x && x_ss && cin && dims, "segformer: null source table");
  IUNET_REQUIRE(!sc == !sh, "segformer: the prologue needs both scale and shift tables");
  S.n = nsrc;
  act = sc != nullptr;
  int koff = 0;
  for (int i = 0; i < nsrc; ++i) {
    SfSrc& s = S.s[i];
    IUNET_REQUIRE(x[i], "segformer: source %d is null", i);
    IUNET_REQUIRE(cin[i] > 0 && cin[i] % 32 == 0, "segformer: source %d has %d channels (a positive multiple of 32)", i, cin[i]);
    IUNET_REQUIRE(dims[3 * i] > 0 && dims[3 * i + 1] > 0 && dims[3 * i + 2] > 0 && (nd == 3 || dims[3 * i] == 1),
                  "segformer: source %d has a bad grid %d x %d x %d", i, dims[3 * i], dims[3 * i + 1], dims[3 * i + 2]);
    IUNET_REQUIRE(!act || (sc[i] && sh[i]), "segformer: source %d lacks its prologue scale / shift", i);
    s.x = x[i]; s.x_ss = x_ss[i];
    s.sc = act ? (const float*)sc[i] : nullptr; s.sh = act ? (const float*)sh[i] : nullptr;
    s.C = cin[i]; s.koff = koff; s.D = dims[3 * i]; s.H = dims[3 * i + 1]; s.W = dims[3 * i + 2];
    koff += cin[i];
  }
  return IUNET_OK;
}

int sf_build_ops(SfOps& o, int L, int C, const int* ch, const void* wf, const void* const* w, const void* const* b) {
  IUNET_REQUIRE(L >= 1 && L <= SF_MAXS, "segformer: 1 .. %d levels, got %d", SF_MAXS, L);
  IUNET_REQUIRE(C > 0 && C % 8 == 0, "segformer: C %d (a positive multiple of 8)", C);
  IUNET_REQUIRE(ch && wf && w && b, "segformer: null pointer");
  o.wf = (const float*)wf; o.L = L; o.C = C;
  int koff = 0;
  for (int l = 0; l < L; ++l) {
    IUNET_REQUIRE(ch[l] > 0 && ch[l] % 8 == 0, "segformer: level %d has %d channels (a positive multiple of 8)", l, ch[l]);
    IUNET_REQUIRE(w[l] && b[l], "segformer: level %d: null mlp weight / bias", l);
    o.w[l] = (const float*)w[l]; o.b[l] = (const float*)b[l]; o.ch[l] = ch[l]; o.koff[l] = koff;
    koff += ch[l];
  }
  o.K = koff;
  return IUNET_OK;
}

}  // namespace

extern "C" {

int iunet_sf_pack(int dtype, int L, int C, const int* ch, const void* wf, const void* const* w, const void* const* b, const void* gamma,
                  const void* beta, const void* mean, const void* var, float eps, void* dst, void* dstT, void* bias, void* stream) {
  IUNET_REQUIRE(dtype >= 0 && dtype <= 2, "sf_pack: dtype must be 0 (f16), 1 (bf16) or 2 (f32), got %d", dtype);
  SfOps o;
  const int rc = sf_build_ops(o, L, C, ch, wf, w, b);
  if (rc != IUNET_OK) return rc;
  IUNET_REQUIRE(dst, "sf_pack: null operator");
  IUNET_REQUIRE(!gamma || (beta && mean && var), "sf_pack: a BatchNorm fold needs gamma, beta, mean and var");
  const long long total = (long long)C * o.K + C;
  const dim3 grid((unsigned)((total + 255) / 256));
#define SFP(OT) hipLaunchKernelGGL(sf_pack_kernel<OT>, grid, dim3(256), 0, (hipStream_t)stream, o, (const float*)gamma, (const float*)beta, \
                                   (const float*)mean, (const float*)var, eps, (OT*)dst, (OT*)dstT, (float*)bias)
  if (dtype == 0) SFP(f16); else if (dtype == 1) SFP(bf16); else SFP(float);
#undef SFP
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_sf_stats_parts(int N, int D, int H, int W) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0) return -1;
  return (int)(((long long)N * D * H * W + SF_COLS - 1) / SF_COLS);
}

int iunet_sf_gemm(int dtype, int nd, int nsrc, const void* const* x, const long long* x_ss, const int* cin, const int* dims, const void* const* sc,
                  const void* const* sh, const void* wpk, const void* bias, void* y, long long y_ss, void* stats, int epi, int N, int D, int H,
                  int W, int Cout, void* stream) {
  IUNET_REQUIRE(dtype >= 0 && dtype <= 2, "sf_gemm: dtype must be 0 (f16), 1 (bf16) or 2 (planar f32), got %d", dtype);
  const int rc = sf_check_t(nd, N, D, H, W);
  if (rc != IUNET_OK) return rc;
  IUNET_REQUIRE(Cout > 0 && Cout % 16 == 0 && Cout <= SF_MAXC, "sf_gemm: Cout %d (a multiple of 16 up to %d)", Cout, SF_MAXC);
  IUNET_REQUIRE(wpk && bias && y, "sf_gemm: null pointer");
  IUNET_REQUIRE(epi == 0 || epi == 1, "sf_gemm: epi must be 0 (raw + statistics) or 1 (relu(acc + bias)), got %d", epi);
  IUNET_REQUIRE(epi == 0 || !stats, "sf_gemm: statistics are taken of the raw output (epi 0) only");
  SfGemm p;
  bool act = false;
  const int rs = sf_build_srcs(p.src, nd, nsrc, x, x_ss, cin, dims, sc, sh, act);
  if (rs != IUNET_OK) return rs;
  p.wpk = wpk; p.K = p.src.s[nsrc - 1].koff + p.src.s[nsrc - 1].C; p.bias = (const float*)bias;
  p.y = y; p.y_ss = y_ss; p.stats = (float*)stats;
  p.D = D; p.H = H; p.W = W; p.Cout = Cout; p.epi = epi;
  p.cols = (long long)N * D * H * W;
  const dim3 grid((unsigned)iunet_sf_stats_parts(N, D, H, W));
  const size_t es = dtype == 2 ? 4 : 2, ld = dtype == 2 ? SF_LD32 : SF_LD16;
  const size_t lds = (size_t)(SF_COLS + Cout) * ld * es;
  const int rl = iunet_dispatch<true>(dtype, nd, act, [&](auto t, auto ndc, auto a) -> int {
    if (lds > 65536) IUNET_SET_MAX_LDS((sf_gemm_kernel<decltype(t), ndc.value, a.value>), (int)lds);
    hipLaunchKernelGGL((sf_gemm_kernel<decltype(t), ndc.value, a.value>), grid, dim3(256), lds, (hipStream_t)stream, p);
    return IUNET_OK;
  });
  if (rl != IUNET_OK) return rl;
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

long long iunet_sf_wgrad_slab_floats(int N, int D, int H, int W, int K, int Cout) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || K <= 0 || Cout <= 0) return -1;
  const long long per = (long long)Cout * K;
  return gg_wgrad_splits((long long)N * D * H * W, per) * per;
}

int iunet_sf_wgrad(int dtype, int nd, int nsrc, const void* const* x, const long long* x_ss, const int* cin, const int* dims, const void* const* sc,
                   const void* const* sh, const void* dz, long long dz_ss, void* slab, void* G, int N, int D, int H, int W, int Cout, void* stream) {
  IUNET_REQUIRE(dtype == 0 || dtype == 1, "sf_wgrad: dtype must be 0 (f16) or 1 (bf16), got %d", dtype);
  const int rc = sf_check_t(nd, N, D, H, W);
  if (rc != IUNET_OK) return rc;
  IUNET_REQUIRE(Cout > 0 && Cout % 8 == 0, "sf_wgrad: Cout %d (a positive multiple of 8)", Cout);
  IUNET_REQUIRE(dz && slab && G, "sf_wgrad: null pointer");
  GgWg p;
  SfSrcs src;
  bool act = false;
  const int rs = sf_build_srcs(src, nd, nsrc, x, x_ss, cin, dims, sc, sh, act);
  if (rs != IUNET_OK) return rs;
  p.dy = dz; p.dy_ss = dz_ss; p.slab = (float*)slab;
  p.D = D; p.H = H; p.W = W; p.Cout = Cout; p.K = src.s[nsrc - 1].koff + src.s[nsrc - 1].C;
  p.cols = (long long)N * D * H * W;
  const long long per = (long long)Cout * p.K;
  const int splits = gg_wgrad_splits(p.cols, per);
  const long long nchunks = (p.cols + 31) / 32;
  p.chunks_per_split = (nchunks + splits - 1) / splits;
  const dim3 grid(splits, (Cout + 63) / 64, (p.K + 63) / 64);
  iunet_dispatch(dtype, nd, act, [&](auto t, auto ndc, auto a) {
    hipLaunchKernelGGL((gg_wgrad_kernel<decltype(t), a.value, SfResample<ndc.value>>), grid, dim3(256), 0, (hipStream_t)stream, p,
                       SfResample<ndc.value>{src});
  });
  IUNET_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(sf_wgrad_reduce_kernel, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)slab, splits,
                     per, (float*)G);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_sf_adjoint(int dtype, int nd, const void* u, long long u_ss, int Dt, int Ht, int Wt, void* dx, long long dx_ss, int Ds, int Hs, int Ws,
                     int C, int N, void* stream) {
  IUNET_REQUIRE(dtype == 0 || dtype == 1, "sf_adjoint: dtype must be 0 (f16) or 1 (bf16), got %d", dtype);
  int rc = sf_check_t(nd, N, Dt, Ht, Wt);
  if (rc != IUNET_OK) return rc;
  rc = sf_check_t(nd, N, Ds, Hs, Ws);
  if (rc != IUNET_OK) return rc;
  IUNET_REQUIRE(C > 0 && C % 8 == 0, "sf_adjoint: C %d (a positive multiple of 8)", C);
  IUNET_REQUIRE(u && dx, "sf_adjoint: null pointer");
  const long long total = (long long)N * (C / 8) * Ds * Hs * Ws;
  const dim3 grid((unsigned)((total + 255) / 256));
  // resample.h's gather in its thread-per-voxel form only: the wide form sums in another order
  iunet_dispatch(dtype, nd, false, [&](auto t, auto ndc, auto) {
    using T = decltype(t);
    hipLaunchKernelGGL((resample_adjoint_kernel<T, ndc.value, resample_axis_f32>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)u, u_ss, Dt,
                       Ht, Wt, (T*)dx, dx_ss, Ds, Hs, Ws, C, N, 0);
  });
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_sf_param_grads(int L, int C, const int* ch, const void* wf, const void* const* w, const void* const* b, const void* G, const void* rs,
                         int N, void* const* dw, void* const* db, void* dwf, void* stream) {
  SfOps o;
  const int rc = sf_build_ops(o, L, C, ch, wf, w, b);
  if (rc != IUNET_OK) return rc;
  IUNET_REQUIRE(G && rs && dw && db && dwf && N > 0, "sf_param_grads: null pointer or N %d", N);
  SfGrads g;
  for (int l = 0; l < L; ++l) {
    IUNET_REQUIRE(dw[l] && db[l], "sf_param_grads: level %d: null gradient", l);
    g.dw[l] = (float*)dw[l]; g.db[l] = (float*)db[l];
  }
  g.dwf = (float*)dwf;
  const long long total = (long long)C * o.K + (long long)C * L * C + (long long)L * C;
  hipLaunchKernelGGL(sf_param_grad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, o, g, (const float*)G,
                     (const float*)rs, N);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

}  // extern "C"
