// The 3^d stage convolution (d = 2, 3; stride 1, pad 1): host entry and operator packing.  The kernel is conv3_v4.hip's
// (an im2col-free implicit GEMM on the gfx950 matrix cores, used for the forward stage convs and, with repacked weights, for their
// data gradients); this file checks a launch's arguments and hands it on, and holds the kernels that put fp32 weights
// [Cout][Cin][taps] into the two fragment orders that kernel reads: the padded K16 order (layout 2) and the compact K16 order (layout 3).
#include "common.h"

namespace {

// K16 packing (layout 2 of conv3_v4.hip): [cob32][chunk16][column pair][dy][2][64][8].
// A filter "column" is a (dz, dx) pair (9 in 3-D, 3 in 2-D); a k-step holds two columns x 16 channels:
// lane (row = l & 15, q = l >> 4), element j -> column 2 pair + (q >> 1), cin = 16 chunk + 8 (q & 1) + j.
template <typename T>
__global__ void pack_conv3_k16_kernel(const float* __restrict__ w, const float* __restrict__ scale, T* __restrict__ dst,
                                      int CoutP, int CinP, int taps, int dgrad, int CinO) {
  const int ncol = taps / 3, ncmb = (ncol + 1) / 2, nchunk = CinP >> 4;
  const long long total = (long long)(CoutP / 32) * nchunk * ncmb * 3 * 2 * 64 * 8;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    long long r = i;
    const int j = r & 7; r >>= 3;
    const int lane = r & 63; r >>= 6;
    const int m = r & 1; r >>= 1;
    const int dy = r % 3; r /= 3;
    const int c = r % ncmb; r /= ncmb;
    const int chunk = r % nchunk;
    const int cob = r / nchunk;
    const int row = lane & 15, qq = lane >> 4;
    const int co = cob * 32 + 8 * (row >> 2) + 4 * m + (row & 3);
    const int ci = chunk * 16 + 8 * (qq & 1) + j;
    const int col = 2 * c + (qq >> 1);
    float v = 0.f;
    if (col < ncol) {
      const int tap = ((col / 3) * 3 + dy) * 3 + (col % 3);       // (dz, dy, dx) -> linear tap
      if (!dgrad) { v = w[((long long)co * CinO + ci) * taps + tap]; if (scale) v *= scale[co]; }
      else v = w[((long long)ci * CinO + co) * taps + (taps - 1 - tap)];
    }
    dst[i] = from_f32<T>(v);
  }
}

// Compact K16 order (mode bit 2; conv3_v4.hip's padding-free step): the last filter column -- (dz, dx) column 8 of the 3^3 filter, dx
// column 2 of the 3^2 filter -- of two consecutive 16-channel chunks shares one k-step instead of being padded to a pair with zeros.
// Per Cout tile and chunk PAIR (32 channels), NR = 4 (3-D) / 1 (2-D) regular column pairs:
//   [even chunk: column pairs 0..NR-1][dy][2][64][8]  (24 / 6 KB)  |  [odd chunk: the same]  |  [cross: dy][2][64][8]  (6 KB),
// cross lanes q >> 1 = 0: the last column of the even chunk, q >> 1 = 1: of the odd chunk.  Cout x Cin x taps elements: no padding.
// 2-D: the pair block IS one 32-channel step of conv3_v4.hip -- three k-groups instead of four (-25 % MFMAs and fragment reads).
template <typename T>
__global__ void pack_conv3_k16c_kernel(const float* __restrict__ w, const float* __restrict__ scale, T* __restrict__ dst,
                                       int CoutP, int CinP, int taps, int dgrad, int CinO) {
  constexpr int FR = 512;                                           // elements of one fragment (64 lanes x 8)
  const int ncol = taps / 3, nreg = ncol / 2;                       // 9 columns: 4 regular pairs; 3 columns: 1
  const int EVEN = nreg * 3 * 2 * FR, PAIR = 2 * EVEN + 3 * 2 * FR, NF = nreg * 6;      // elements; fragments of a chunk's regular part
  const int npair = CinP >> 5;
  const long long total = (long long)(CoutP / 32) * npair * PAIR;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int e = (int)(i % PAIR);
    long long r = i / PAIR;
    const int pr = (int)(r % npair), cob = (int)(r / npair);
    const int j = e & 7, lane = (e >> 3) & 63;
    const int row = lane & 15, qq = lane >> 4;
    int frag = e >> 9, chunk, col;                                  // fragment index within the pair block
    if (frag < 2 * NF) { chunk = 2 * pr + frag / NF; frag %= NF; col = 2 * (frag / 6) + (qq >> 1); frag %= 6; }
    else { frag -= 2 * NF; chunk = 2 * pr + (qq >> 1); col = ncol - 1; }
    const int dy = frag >> 1, m = frag & 1;
    const int co = cob * 32 + 8 * (row >> 2) + 4 * m + (row & 3);
    const int ci = chunk * 16 + 8 * (qq & 1) + j;
    const int tap = ((col / 3) * 3 + dy) * 3 + (col % 3);
    float v;
    if (!dgrad) { v = w[((long long)co * CinO + ci) * taps + tap]; if (scale) v *= scale[co]; }
    else v = w[((long long)ci * CinO + co) * taps + (taps - 1 - tap)];
    dst[i] = from_f32<T>(v);
  }
}

}  // namespace

// Host entry used by the net runtime and the per-kernel C ABI.  layout: 2 = the padded K16 operator, 3 = the compact one.
int iunet_conv3_launch(int dtype, int nd, const void* x, long long x_sstride, void* y, long long y_sstride,
                       const void* wpk, const float* bias, float* stats, int N, int D, int H, int W, int Cin,
                       int Cout, int epi, int layout, hipStream_t stream, const float* in_scale, const float* in_shift,
                       const void* bw_y, long long bw_y_ss, const float* const* bw_par) {
  IUNET_REQUIRE(nd == 2 || nd == 3, "conv3: nd must be 2 or 3 (got %d)", nd);
  IUNET_REQUIRE(Cin % 32 == 0 && Cout % 32 == 0, "conv3: Cin (%d) and Cout (%d) must be multiples of 32", Cin, Cout);
  IUNET_REQUIRE(nd == 3 || D == 1, "conv3: 2-D conv needs D == 1");
  IUNET_REQUIRE(epi == 0 || bias != nullptr, "conv3: epilogue %d needs a bias", epi);
  IUNET_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), "conv3: in_scale and in_shift come together");
  IUNET_REQUIRE(layout == 2 || layout == 3, "conv3: layout must be 2 or 3 (got %d)", layout);
  IUNET_REQUIRE(bw_y == nullptr || layout == 2 || (nd == 2 && Cin <= 64), "conv3: the fused BatchNorm-backward sums need layout 2, or layout 3 in 2-D up to 64 input channels (got %d)", layout);
  return iunet_conv3_v4_launch(dtype, nd, x, x_sstride, y, y_sstride, wpk, bias, stats, N, D, H, W, Cin, Cout, epi,
                               in_scale, in_shift, stream, bw_y, bw_y_ss, bw_par, layout == 3);
}

// tiles of the first conv's grid (iunet_conv3_num_tiles: the rows its statistics epilogue writes)
int iunet_conv3_tiles(int nd, int N, int D, int H, int W) {
  const int TZ = nd == 3 ? 4 : 1, TY = nd == 3 ? 8 : 16, TX = nd == 3 ? 16 : 32;
  return N * ((D + TZ - 1) / TZ) * ((H + TY - 1) / TY) * ((W + TX - 1) / TX);
}

#define PACK_MODE_OK(mode) IUNET_REQUIRE((mode) & 2, "pack_conv3: mode %d has no K16 bit (2, 3: the padded K16 operator / its data-gradient form; 6, 7: the compact one)", (mode))

// elements of the packed operator (mode bit 0: data-gradient operator; bit 1: K16 order, always set; bit 2: compact, no padding)
long long iunet_pack_conv3_size(int Cout, int Cin, int taps, int mode) {
  PACK_MODE_OK(mode);
  if (mode & 4) return (long long)Cout * Cin * taps;
  return (long long)Cout * Cin * ((taps / 3 + 1) / 2) * 6;             // the padded K16 order pads the filter columns to pairs
}

int iunet_pack_conv3_launch(int dtype, const float* w, const float* scale, void* dst, int Cout, int Cin, int taps,
                            int mode, hipStream_t stream) {
  const int dg = mode & 1;            // data-gradient operator (Cin x Cout, taps mirrored)
  const int CoutP = dg == 0 ? Cout : Cin, CinP = dg == 0 ? Cin : Cout;
  IUNET_REQUIRE(CoutP % 32 == 0 && CinP % 32 == 0, "pack_conv3: channel counts must be multiples of 32 (%d, %d)", CoutP, CinP);
  PACK_MODE_OK(mode);

  if (mode & 4) {     // compact K16 (conv3_v4.hip: layout 3 in 3-D, the cross-pair step of the 2-D split-precision conv)
    const long long tot = (long long)CoutP * CinP * taps;
    const int nb = (int)((tot + 255) / 256 < 4096 ? (tot + 255) / 256 : 4096);
    if (dtype == 0) hipLaunchKernelGGL(pack_conv3_k16c_kernel<f16>, dim3(nb), dim3(256), 0, stream, w, scale, (f16*)dst, CoutP, CinP, taps, dg, Cin);
    else hipLaunchKernelGGL(pack_conv3_k16c_kernel<bf16>, dim3(nb), dim3(256), 0, stream, w, scale, (bf16*)dst, CoutP, CinP, taps, dg, Cin);
    IUNET_CHECK_HIP(hipGetLastError());
    return IUNET_OK;
  }
  const long long tot = (long long)(CoutP / 32) * (CinP / 16) * ((taps / 3 + 1) / 2) * 3 * 1024;
  const int nb = (int)((tot + 255) / 256 < 4096 ? (tot + 255) / 256 : 4096);
  if (dtype == 0) hipLaunchKernelGGL(pack_conv3_k16_kernel<f16>, dim3(nb), dim3(256), 0, stream, w, scale, (f16*)dst, CoutP, CinP, taps, dg, Cin);
  else hipLaunchKernelGGL(pack_conv3_k16_kernel<bf16>, dim3(nb), dim3(256), 0, stream, w, scale, (bf16*)dst, CoutP, CinP, taps, dg, Cin);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}
