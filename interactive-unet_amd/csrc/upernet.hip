// UPerNet decoder (unet.param_shapes(..., architecture='UPerNet')): the part of the graph that moves data between grids.  Every conv of
// the decoder runs on deeplab.hip's gathered GEMMs; this file adds
//   pn_resize_kernel        dst slot = [base +] R(act(src)): linear resampling (align_corners=False) from any grid to any grid
//   iunet_pn_resize_adjoint dx = [dx +] R^T(u): resample.h's gather over the source grid (its wide form: a workgroup per source voxel)
//   pn_pool_kernel          the four adaptive average pools (1, 2, 3, 6 bins per axis) of X^B in one launch
//   pn_pool_bwd_kernel      dX^B = the identity slot's gradient + sum_s pool_s^T(dA_s), one gather per voxel
//   pn_bias_relu_bwd_*      backward of relu(y + bias) of the norm-free 1-bin branch
// Tensors are NHWC8c (dtype 0 f16 / 1 bf16) or planar fp32 [N][C][vox] (dtype 2) with sample strides in elements, so a channel slot of a
// wider tensor is a pointer offset (c vox elements in both layouts) and the wider tensor's sample stride.
//
// Source index: resample_axis_exact of resample.h (align_corners=False on the integers, one rounding; the forward and its adjoint share it).
#include "common.h"
#include "resample.h"

namespace {

struct PnResize {
  const void* src; long long src_ss; int Ds, Hs, Ws;
  const float* sc; const float* sh;                       // prologue of src (template flag ACT)
  const void* base; long long base_ss;                    // optional, on the target grid
  const float* bsc; const float* bsh;                     // non-null: base is raw, relu(bsc y + bsh) is added
  void* dst; long long dst_ss; int Dt, Ht, Wt;
  int C, N;
};

// One thread = one channel group of one target voxel; consecutive lanes = consecutive voxels along W: 16-byte (fp32: 4-byte) stores,
// contiguous across the wave; the source rows a wave reads are contiguous runs too.
template <typename T, int ND, bool ACT>
__global__ __launch_bounds__(256) void pn_resize_kernel(PnResize p) {
  constexpr int G = ChanGroup<T>::G;
  const long long vT = (long long)p.Dt * p.Ht * p.Wt, vS = (long long)p.Ds * p.Hs * p.Ws;
  const int groups = p.C / G;
  const long long total = (long long)p.N * groups * vT;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long r = i % vT;
  const int g = (int)((i / vT) % groups), n = (int)(i / (vT * groups));
  const int tw = (int)(r % p.Wt), th = (int)((r / p.Wt) % p.Ht), td = (int)(r / ((long long)p.Wt * p.Ht));
  ResampleAx ad = {0, 0, 0.f};
  if (ND == 3) ad = resample_axis_exact(td, p.Dt, p.Ds);
  const ResampleAx ah = resample_axis_exact(th, p.Ht, p.Hs), aw = resample_axis_exact(tw, p.Wt, p.Ws);
  const T* s = (const T*)p.src + (long long)n * p.src_ss;
  float acc[G];
#pragma unroll
  for (int j = 0; j < G; ++j) acc[j] = 0.f;
  resample_taps<ND>(ad, ah, aw, p.Hs, p.Ws, [&](long long vox, float wgt) {
    float v[G];
    group_load<T>(s, g, vox, vS, v);
#pragma unroll
    for (int j = 0; j < G; ++j) {
      if constexpr (ACT) v[j] = norm_z<T, true>(p.sc[g * G + j], v[j], p.sh[g * G + j]);
      acc[j] = fmaf(wgt, v[j], acc[j]);
    }
  });
  if (p.base != nullptr) {
    float b[G];
    group_load<T>((const T*)p.base + (long long)n * p.base_ss, g, r, vT, b);
#pragma unroll
    for (int j = 0; j < G; ++j) {
      if (p.bsc != nullptr) b[j] = norm_z<T, true>(p.bsc[g * G + j], b[j], p.bsh[g * G + j]);
      acc[j] += b[j];
    }
  }
  group_store<T>((T*)p.dst + (long long)n * p.dst_ss, g, r, vT, acc);
}

// ---- the adjoint R^T: resample_adjoint_kernel / resample_adjoint_wide_kernel of resample.h under resample_axis_exact
constexpr long long PN_WIDE_FROM = 512;        // candidates per source voxel from which the workgroup-per-voxel kernel runs

// ---- adaptive average pooling, PyTorch's windows: bin i of s over n voxels = [floor(i n / s), ceil((i + 1) n / s))
constexpr int PN_NS = 4;
__host__ __device__ constexpr int pn_size(int k) { return k == 0 ? 1 : k == 1 ? 2 : k == 2 ? 3 : 6; }
__device__ __forceinline__ int pn_bin_lo(int i, int n, int s) { return (i * n) / s; }
__device__ __forceinline__ int pn_bin_hi(int i, int n, int s) { return ((i + 1) * n + s - 1) / s; }

struct PnPool {
  const void* x; long long x_ss;
  void* out[PN_NS]; long long out_ss[PN_NS];         // A_s on the grid s^ND, s = 1, 2, 3, 6
  int D, H, W, C, N;
};

// One wave = one bin of one channel group: its lanes walk the window (each lane's partial sum in window order, then the xor tree), the
// mean is sum / count
template <typename T, int ND>
__global__ __launch_bounds__(64) void pn_pool_kernel(PnPool p) {
  constexpr int G = ChanGroup<T>::G;
  constexpr int NB = ND == 3 ? 1 + 8 + 27 + 216 : 1 + 4 + 9 + 36;
  const int groups = p.C / G;
  const long long item = blockIdx.x;
  int b = (int)(item % NB);
  const int g = (int)((item / NB) % groups), n = (int)(item / ((long long)NB * groups));
  int k = 0;
  for (; k < PN_NS - 1; ++k) {
    const int nb = ND == 3 ? pn_size(k) * pn_size(k) * pn_size(k) : pn_size(k) * pn_size(k);
    if (b < nb) break;
    b -= nb;
  }
  const int s = pn_size(k);
  const int bw = b % s, bh = (b / s) % s, bd = ND == 3 ? b / (s * s) : 0;
  const int d0 = ND == 3 ? pn_bin_lo(bd, p.D, s) : 0, d1 = ND == 3 ? pn_bin_hi(bd, p.D, s) : 1;
  const int h0 = pn_bin_lo(bh, p.H, s), h1 = pn_bin_hi(bh, p.H, s), w0 = pn_bin_lo(bw, p.W, s), w1 = pn_bin_hi(bw, p.W, s);
  const int nw = w1 - w0, nh = h1 - h0, cnt = (d1 - d0) * nh * nw;
  const long long vox = (long long)p.D * p.H * p.W;
  const T* xs = (const T*)p.x + (long long)n * p.x_ss;
  float acc[G];
#pragma unroll
  for (int j = 0; j < G; ++j) acc[j] = 0.f;
  for (int e = threadIdx.x; e < cnt; e += 64) {
    const int ew = e % nw, eh = (e / nw) % nh, ed = e / (nw * nh);
    float v[G];
    group_load<T>(xs, g, ((long long)(d0 + ed) * p.H + (h0 + eh)) * p.W + (w0 + ew), vox, v);
#pragma unroll
    for (int j = 0; j < G; ++j) acc[j] += v[j];
  }
#pragma unroll
  for (int j = 0; j < G; ++j) acc[j] = wave_sum(acc[j]) / (float)cnt;
  if (threadIdx.x == 0) group_store<T>((T*)p.out[k] + (long long)n * p.out_ss[k], g, b, ND == 3 ? s * s * s : s * s, acc);
}

struct PnPoolBwd {
  const void* du; long long du_ss;                    // the identity slot's gradient on X^B's grid (or null)
  const void* da[PN_NS]; long long da_ss[PN_NS];      // dA_s on s^ND
  void* dx; long long dx_ss;
  int D, H, W, C, N;
};

// the bins of size s whose window holds index i (at most two per axis)
__device__ __forceinline__ void pn_bins_of(int i, int n, int s, int& lo, int& hi) {
  lo = s; hi = -1;
  for (int b = 0; b < s; ++b)
    if (pn_bin_lo(b, n, s) <= i && i < pn_bin_hi(b, n, s)) { lo = min(lo, b); hi = max(hi, b); }
}

template <typename T, int ND>
__global__ __launch_bounds__(256) void pn_pool_bwd_kernel(PnPoolBwd p) {
  const long long vox = (long long)p.D * p.H * p.W;
  const long long total = (long long)p.N * (p.C / 8) * vox;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long r = i % vox;
  const int pl = (int)((i / vox) % (p.C / 8)), n = (int)(i / (vox * (p.C / 8)));
  const int qw = (int)(r % p.W), qh = (int)((r / p.W) % p.H), qd = (int)(r / ((long long)p.W * p.H));
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  if (p.du != nullptr) group_load<T>((const T*)p.du + (long long)n * p.du_ss, pl, r, vox, acc);
  for (int k = 0; k < PN_NS; ++k) {
    const int s = pn_size(k);
    int dlo = 0, dhi = 0, hlo, hhi, wlo, whi;
    if (ND == 3) pn_bins_of(qd, p.D, s, dlo, dhi);
    pn_bins_of(qh, p.H, s, hlo, hhi);
    pn_bins_of(qw, p.W, s, wlo, whi);
    const T* a = (const T*)p.da[k] + (long long)n * p.da_ss[k];
    const long long nb = ND == 3 ? s * s * s : s * s;
    for (int bd = dlo; bd <= dhi; ++bd) {
      const int cd = ND == 3 ? pn_bin_hi(bd, p.D, s) - pn_bin_lo(bd, p.D, s) : 1;
      for (int bh = hlo; bh <= hhi; ++bh) {
        const int ch = cd * (pn_bin_hi(bh, p.H, s) - pn_bin_lo(bh, p.H, s));
        for (int bw = wlo; bw <= whi; ++bw) {
          const float inv = 1.f / (float)(ch * (pn_bin_hi(bw, p.W, s) - pn_bin_lo(bw, p.W, s)));
          float v[8];
          group_load<T>(a, pl, ((long long)bd * s + bh) * s + bw, nb, v);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] = fmaf(inv, v[j], acc[j]);
        }
      }
    }
  }
  group_store<T>((T*)p.dx + (long long)n * p.dx_ss, pl, r, vox, acc);
}

// ---- backward of q = relu(y + bias) (the 1-bin branch has no norm): dy = dz where the stored q is positive; dbias[c] = sum dy in (n, voxel) order
template <typename T>
__global__ __launch_bounds__(256) void pn_bias_relu_bwd_kernel(const T* __restrict__ dz, long long dz_ss, const T* __restrict__ y, long long y_ss,
                                                               const float* __restrict__ bias, T* __restrict__ dy, long long dy_ss, int C, int N,
                                                               long long vox) {
  const long long total = (long long)N * (C / 8) * vox;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long r = i % vox;
  const int pl = (int)((i / vox) % (C / 8)), n = (int)(i / (vox * (C / 8)));
  float g[8], v[8];
  group_load<T>(dz + (long long)n * dz_ss, pl, r, vox, g);
  group_load<T>(y + (long long)n * y_ss, pl, r, vox, v);
#pragma unroll
  for (int j = 0; j < 8; ++j) g[j] = norm_masked(norm_z<T, true>(1.f, v[j], bias[pl * 8 + j]), g[j]);
  group_store<T>(dy + (long long)n * dy_ss, pl, r, vox, g);
}

template <typename T>
__global__ __launch_bounds__(256) void pn_bias_sum_kernel(const T* __restrict__ dy, long long dy_ss, float* __restrict__ dbias, int C, int N,
                                                          long long vox) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (int n = 0; n < N; ++n)
    for (long long v = 0; v < vox; ++v) s += to_f32<T>(dy[(long long)n * dy_ss + ((long long)(c >> 3) * vox + v) * 8 + (c & 7)]);
  dbias[c] = s;
}

int pn_check_grid(const char* what, int nd, int N, int D, int H, int W) {
  IUNET_REQUIRE(nd == 2 || nd == 3, "%s: nd must be 2 or 3, got %d", what, nd);
  IUNET_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0 && (nd == 3 || D == 1), "%s: bad grid N %d, %d x %d x %d (D = 1 in 2-D)", what, N, D, H, W);
  IUNET_REQUIRE((long long)D * H * W < (1ll << 30) && D < (1 << 20) && H < (1 << 20) && W < (1 << 20), "%s: grid %d x %d x %d is too large", what, D,
                H, W);
  return IUNET_OK;
}

}  // namespace

extern "C" {

int iunet_pn_resize(int dtype, int nd, const void* src, long long src_ss, int Ds, int Hs, int Ws, const void* scale, const void* shift,
                    const void* base, long long base_ss, const void* base_scale, const void* base_shift, void* dst, long long dst_ss, int Dt,
                    int Ht, int Wt, int C, int N, void* stream) {
  IUNET_REQUIRE(dtype >= 0 && dtype <= 2, "pn_resize: dtype must be 0 (f16), 1 (bf16) or 2 (planar f32), got %d", dtype);
  int rc = pn_check_grid("pn_resize (source)", nd, N, Ds, Hs, Ws);
  if (rc != IUNET_OK) return rc;
  rc = pn_check_grid("pn_resize (target)", nd, N, Dt, Ht, Wt);
  if (rc != IUNET_OK) return rc;
  IUNET_REQUIRE(C > 0 && C % 8 == 0, "pn_resize: C %d (a positive multiple of 8)", C);
  IUNET_REQUIRE(src && dst, "pn_resize: null pointer");
  IUNET_REQUIRE(!scale == !shift, "pn_resize: the source activation needs both scale and shift");
  IUNET_REQUIRE(!base_scale == !base_shift && (base || !base_scale), "pn_resize: a raw base needs the base, its scale and its shift");
  PnResize p;
  p.src = src; p.src_ss = src_ss; p.Ds = Ds; p.Hs = Hs; p.Ws = Ws; p.sc = (const float*)scale; p.sh = (const float*)shift;
  p.base = base; p.base_ss = base_ss; p.bsc = (const float*)base_scale; p.bsh = (const float*)base_shift;
  p.dst = dst; p.dst_ss = dst_ss; p.Dt = Dt; p.Ht = Ht; p.Wt = Wt; p.C = C; p.N = N;
  const long long total = (long long)N * (dtype == 2 ? C : C / 8) * Dt * Ht * Wt;
  const dim3 grid((unsigned)((total + 255) / 256));
  iunet_dispatch<true>(dtype, nd, scale != nullptr, [&](auto t, auto ndc, auto act) {
    hipLaunchKernelGGL((pn_resize_kernel<decltype(t), ndc.value, act.value>), grid, dim3(256), 0, (hipStream_t)stream, p);
  });
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_pn_resize_adjoint(int dtype, int nd, const void* u, long long u_ss, int Dt, int Ht, int Wt, void* dx, long long dx_ss, int Ds, int Hs,
                            int Ws, int C, int N, int accumulate, void* stream) {
  IUNET_REQUIRE(dtype == 0 || dtype == 1, "pn_resize_adjoint: dtype must be 0 (f16) or 1 (bf16), got %d", dtype);
  int rc = pn_check_grid("pn_resize_adjoint (target)", nd, N, Dt, Ht, Wt);
  if (rc != IUNET_OK) return rc;
  rc = pn_check_grid("pn_resize_adjoint (source)", nd, N, Ds, Hs, Ws);
  if (rc != IUNET_OK) return rc;
  IUNET_REQUIRE(C > 0 && C % 8 == 0, "pn_resize_adjoint: C %d (a positive multiple of 8)", C);
  IUNET_REQUIRE(u && dx, "pn_resize_adjoint: null pointer");
  IUNET_REQUIRE(accumulate == 0 || accumulate == 1, "pn_resize_adjoint: accumulate must be 0 or 1, got %d", accumulate);
  const long long total = (long long)N * (C / 8) * Ds * Hs * Ws;
  const long long cand = (nd == 3 ? pn_adj_extent(Ds, Dt) : 1) * pn_adj_extent(Hs, Ht) * pn_adj_extent(Ws, Wt);
  const bool wide = cand >= PN_WIDE_FROM && total < (1ll << 31);
  const dim3 grid((unsigned)(wide ? total : (total + 255) / 256));
  iunet_dispatch(dtype, nd, wide, [&](auto t, auto ndc, auto w) {
    using T = decltype(t);
    if constexpr (w.value)
      hipLaunchKernelGGL((resample_adjoint_wide_kernel<T, ndc.value, resample_axis_exact>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)u,
                         u_ss, Dt, Ht, Wt, (T*)dx, dx_ss, Ds, Hs, Ws, C, N, accumulate);
    else
      hipLaunchKernelGGL((resample_adjoint_kernel<T, ndc.value, resample_axis_exact>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)u, u_ss,
                         Dt, Ht, Wt, (T*)dx, dx_ss, Ds, Hs, Ws, C, N, accumulate);
  });
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_pn_pool(int dtype, int nd, const void* x, long long x_ss, int D, int H, int W, void* const* out, const long long* out_ss, int C, int N,
                  void* stream) {
  IUNET_REQUIRE(dtype >= 0 && dtype <= 2, "pn_pool: dtype must be 0 (f16), 1 (bf16) or 2 (planar f32), got %d", dtype);
  const int rc = pn_check_grid("pn_pool", nd, N, D, H, W);
  if (rc != IUNET_OK) return rc;
  IUNET_REQUIRE(C > 0 && C % 8 == 0, "pn_pool: C %d (a positive multiple of 8)", C);
  IUNET_REQUIRE(x && out && out_ss, "pn_pool: null pointer");
  PnPool p;
  p.x = x; p.x_ss = x_ss; p.D = D; p.H = H; p.W = W; p.C = C; p.N = N;
  for (int k = 0; k < PN_NS; ++k) {
    IUNET_REQUIRE(out[k], "pn_pool: null output %d", k);
    p.out[k] = out[k]; p.out_ss[k] = out_ss[k];
  }
  const long long items = (long long)N * (dtype == 2 ? C : C / 8) * (nd == 3 ? 252 : 50);
  IUNET_REQUIRE(items < (1ll << 31), "pn_pool: %lld bins exceed one launch", items);
  iunet_dispatch<true>(dtype, nd, false, [&](auto t, auto ndc, auto) {
    hipLaunchKernelGGL((pn_pool_kernel<decltype(t), ndc.value>), dim3((unsigned)items), dim3(64), 0, (hipStream_t)stream, p);
  });
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_pn_pool_bwd(int dtype, int nd, const void* du, long long du_ss, const void* const* da, const long long* da_ss, void* dx, long long dx_ss,
                      int D, int H, int W, int C, int N, void* stream) {
  IUNET_REQUIRE(dtype == 0 || dtype == 1, "pn_pool_bwd: dtype must be 0 (f16) or 1 (bf16), got %d", dtype);
  const int rc = pn_check_grid("pn_pool_bwd", nd, N, D, H, W);
  if (rc != IUNET_OK) return rc;
  IUNET_REQUIRE(C > 0 && C % 8 == 0, "pn_pool_bwd: C %d (a positive multiple of 8)", C);
  IUNET_REQUIRE(da && da_ss && dx, "pn_pool_bwd: null pointer");
  PnPoolBwd p;
  p.du = du; p.du_ss = du_ss; p.dx = dx; p.dx_ss = dx_ss; p.D = D; p.H = H; p.W = W; p.C = C; p.N = N;
  for (int k = 0; k < PN_NS; ++k) {
    IUNET_REQUIRE(da[k], "pn_pool_bwd: null gradient %d", k);
    p.da[k] = da[k]; p.da_ss[k] = da_ss[k];
  }
  const long long total = (long long)N * (C / 8) * D * H * W;
  const dim3 grid((unsigned)((total + 255) / 256));
  iunet_dispatch(dtype, nd, false, [&](auto t, auto ndc, auto) {
    hipLaunchKernelGGL((pn_pool_bwd_kernel<decltype(t), ndc.value>), grid, dim3(256), 0, (hipStream_t)stream, p);
  });
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_pn_bias_relu_bwd(int dtype, const void* dz, long long dz_ss, const void* y, long long y_ss, const void* bias, void* dy, long long dy_ss,
                           void* dbias, int C, int N, long long vox, void* stream) {
  IUNET_REQUIRE(dtype == 0 || dtype == 1, "pn_bias_relu_bwd: dtype must be 0 (f16) or 1 (bf16), got %d", dtype);
  IUNET_REQUIRE(dz && y && bias && dy && dbias, "pn_bias_relu_bwd: null pointer");
  IUNET_REQUIRE(C > 0 && C % 8 == 0 && N > 0 && vox > 0 && vox < (1ll << 30), "pn_bias_relu_bwd: C %d (multiple of 8), N %d, %lld voxels", C, N, vox);
  const long long total = (long long)N * (C / 8) * vox;
  const dim3 grid((unsigned)((total + 255) / 256));
  iunet_dispatch(dtype, 2, false, [&](auto t, auto, auto) {
    using T = decltype(t);
    hipLaunchKernelGGL(pn_bias_relu_bwd_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, (const T*)dz, dz_ss, (const T*)y, y_ss, (const float*)bias,
                       (T*)dy, dy_ss, C, N, vox);
    hipLaunchKernelGGL(pn_bias_sum_kernel<T>, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const T*)dy, dy_ss, (float*)dbias, C, N, vox);
  });
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

}  // extern "C"
