// Weight gradient of the 3^d convolution:
//     dW[co][ci][tap] = sum_{n, v} dy[n][co][v] * x[n][ci][v + tap - 1]
// The voxel-walking kernels (conv3_wgrad_v2.hip in 3-D, conv2_wgrad_v2.hip in 2-D) leave one fp32 slab row
// [Cout/32][Cin/32][taps][32][32] per workgroup (or two); the reduce kernels here sum the rows in a fixed order into dW
// (deterministic, no float atomics).  This file holds the reduce kernels and the extern "C" entries.
#include "common.h"

namespace {

// dW[co][ci][tap] = alpha * sum_b slab[b][cob][cib][tap][co%32][ci%32]; threads walk the slab
// order (coalesced reads of every part), the small dW write is scattered.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ slab, int nb, int Cout, int Cin, int taps,
                                                           float* __restrict__ dW, float alpha) {
  // 64 slab columns per block as 16 float4 lanes x 16 row groups (per_b is a multiple of 1024): 16-byte loads, nb / 16 of them
  // per thread; fixed summation order
  __shared__ f32x4 red[16][16];
  const long long per_b4 = (long long)Cout * Cin * taps / 4;
  const int col4 = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const long long j4 = (long long)blockIdx.x * 16 + col4;
  const f32x4* slab4 = (const f32x4*)slab;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int b = grp; b < nb; b += 16) s += slab4[b * per_b4 + j4];
  red[grp][col4] = s;
  __syncthreads();
  if (grp != 0) return;
#pragma unroll
  for (int g = 1; g < 16; ++g) s += red[g][col4];
  const int ncib = Cin / 32;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long j = j4 * 4 + k;
    const int c = (int)(j & 31), r = (int)((j >> 5) & 31);
    long long t = j >> 10;
    const int tap = (int)(t % taps); t /= taps;
    const int cib = (int)(t % ncib), cob = (int)(t / ncib);
    dW[((long long)(cob * 32 + r) * Cin + cib * 32 + c) * taps + tap] = alpha * s[k];
  }
}

// Wide layers (many 32 x 32 filter blocks, few slab rows -- C5's 512- and 1024-channel convs have one row of 57-113 MB): one
// workgroup per filter block sums its rows into LDS ([tap][32 co][32 ci], tap stride 1025) and writes dW as whole (ci, tap) runs
// of 864 floats per output channel.  The column-parallel kernel above scatters 4-byte writes at a stride of `taps` floats:
// 1.2 TB/s on those layers.
__global__ __launch_bounds__(256) void wgrad_reduce_block_kernel(const float* __restrict__ slab, int nb, int Cout, int Cin, int taps,
                                                                 float* __restrict__ dW, float alpha) {
  extern __shared__ float blk[];                                   // taps x 1025
  const int ncib = Cin / 32;
  const int cib = blockIdx.x % ncib, cob = blockIdx.x / ncib;
  const long long per_b = (long long)Cout * Cin * taps;
  const float* src = slab + (long long)blockIdx.x * taps * 1024;  // this block's [tap][co][ci] in row 0
  const int n4 = taps * 256;                                       // float4 items
  for (int i = threadIdx.x; i < n4; i += 256) {
    f32x4 s = *(const f32x4*)(src + i * 4);
    for (int b = 1; b < nb; ++b) s += *(const f32x4*)(src + b * per_b + i * 4);
    const int tap = i >> 8, rem = (i & 255) * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) blk[tap * 1025 + rem + k] = s[k];
  }
  __syncthreads();
  const int run = 32 * taps;                                       // (ci, tap) elements of one output channel of this block
  for (int r = 0; r < 32; ++r) {
    float* dst = dW + ((long long)(cob * 32 + r) * Cin + cib * 32) * taps;
    for (int e = threadIdx.x; e < run; e += 256) {
      const int c = e / taps, tap = e - c * taps;
      dst[e] = alpha * blk[tap * 1025 + r * 32 + c];
    }
  }
}

}  // namespace

extern "C" {

// number of slab rows (one or two per voxel-walking workgroup) of a (co, ci) block and the slab size they need
int iunet_conv3_wgrad_blocks(int nd, int N, int D, int H, int W, int Cin, int Cout) {
  if (N < 1 || D < 1 || H < 1 || W < 1 || Cin < 32 || Cout < 32 || (nd != 2 && nd != 3)) return 0;
  if (nd == 3) return iunet_conv3_wgrad_v2_blocks(N, D, H, W, Cin, Cout);
  int rows = 0;
  iunet_conv2_wgrad_v2_blocks(N, H, W, Cin, Cout, &rows);            // (the 32 x 32 block writes two slab rows per workgroup)
  return rows;
}

long long iunet_conv3_wgrad_slab_floats(int nd, int N, int D, int H, int W, int Cin, int Cout) {
  const int taps = nd == 3 ? 27 : 9;
  return (long long)iunet_conv3_wgrad_blocks(nd, N, D, H, W, Cin, Cout) * (Cout / 32) * (Cin / 32) * taps * 1024;
}

static int wgrad_impl(int dtype, int nd, const void* x, long long x_ss, const void* dy, long long dy_ss, void* slab,
                      void* dW, float alpha, int N, int D, int H, int W, int Cin, int Cout, const float* x_scale,
                      const float* x_shift, void* stream) {
  IUNET_REQUIRE(dtype == 0 || dtype == 1, "conv3_wgrad: bad dtype %d", dtype);
  IUNET_REQUIRE(nd == 2 || nd == 3, "conv3_wgrad: nd must be 2 or 3");
  IUNET_REQUIRE(Cin >= 32 && Cout >= 32 && Cin % 32 == 0 && Cout % 32 == 0, "conv3_wgrad: channels must be positive multiples of 32 (%d, %d)", Cin, Cout);
  IUNET_REQUIRE_GRID("conv3_wgrad", N, D, H, W);
  IUNET_REQUIRE(nd == 3 || D == 1, "conv3_wgrad: 2-D needs D == 1");
  IUNET_REQUIRE(x && dy && slab && dW, "conv3_wgrad: null pointer");
  const int nb = iunet_conv3_wgrad_blocks(nd, N, D, H, W, Cin, Cout);
  const int rc = nd == 2 ? iunet_conv2_wgrad_v2_launch(dtype, x, x_ss, dy, dy_ss, (float*)slab, N, H, W, Cin, Cout, x_scale, x_shift, (hipStream_t)stream)
                         : iunet_conv3_wgrad_v2_launch(dtype, x, x_ss, dy, dy_ss, (float*)slab, N, D, H, W, Cin, Cout, x_scale, x_shift, (hipStream_t)stream);
  if (rc != IUNET_OK) return rc;
  const int taps = nd == 3 ? 27 : 9;
  const long long total = (long long)Cout * Cin * taps;
  const int nblk = (Cout / 32) * (Cin / 32);
  if (nblk >= 128 && nb <= 4) {                        // wide layer: LDS-transposing reduce, one workgroup per filter block
    const int lds = taps * 1025 * 4;
    IUNET_SET_MAX_LDS(wgrad_reduce_block_kernel, lds);
    hipLaunchKernelGGL(wgrad_reduce_block_kernel, dim3(nblk), dim3(256), lds, (hipStream_t)stream,
                       (const float*)slab, nb, Cout, Cin, taps, (float*)dW, alpha);
  } else {
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)(total / 64)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)slab, nb, Cout, Cin, taps, (float*)dW, alpha);
  }
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

// dW fp32 [Cout][Cin][taps] = alpha * sum over samples and voxels of dy (x) shifted x
int iunet_conv3_wgrad(int dtype, int nd, const void* x, long long x_ss, const void* dy, long long dy_ss, void* slab,
                      void* dW, float alpha, int N, int D, int H, int W, int Cin, int Cout, void* stream) {
  return wgrad_impl(dtype, nd, x, x_ss, dy, dy_ss, slab, dW, alpha, N, D, H, W, Cin, Cout, nullptr, nullptr, stream);
}

// the same with the conv input given as relu(x_scale[c] * x + x_shift[c]) (see iunet_conv3_fwd_act)
int iunet_conv3_wgrad_act(int dtype, int nd, const void* x, long long x_ss, const void* dy, long long dy_ss, void* slab,
                          void* dW, float alpha, const void* x_scale, const void* x_shift, int N, int D, int H, int W,
                          int Cin, int Cout, void* stream) {
  IUNET_REQUIRE(x_scale && x_shift, "conv3_wgrad_act: null scale / shift");
  return wgrad_impl(dtype, nd, x, x_ss, dy, dy_ss, slab, dW, alpha, N, D, H, W, Cin, Cout, (const float*)x_scale,
                    (const float*)x_shift, stream);
}

}  // extern "C"
