// 3-D patch batch producer: the 3-D form of VolumeData.sample + load_resliced_annotations
// (volumedata.py:68-80, loader.py:48-82) as ONE gather launch per batch -- random oblique patches of uint8 image / mask / weight
// volumes, image at spline order 0 or 1, mask and weight at order 0, as the fp16 (X, y, w) a dim = 3 training step takes.
//
// The arithmetic, bit for bit (tests/patch_ref.py restates it in numpy float32: plain float32 multiplies and adds, each rounded,
// in exactly this order, no fma -- contraction is off; the voxel's body is patch_gather.h's patch_gather_voxel, which
// iunet_patch_batch_extra in patch_augment.hip calls too):
//   output voxel (oz, oy, ox) of a patch SZ x SY x SX, sample descriptor d:
//     t_j = (float)o_j - (S_j - 1) / 2                                            (exact)
//     p_a = ((d.m[3 a] * t_z + d.m[3 a + 1] * t_y) + d.m[3 a + 2] * t_x) + d.c[a]     a = 0, 1, 2: source axes z, y, x
//     r_a = rintf(p_a)   (ties to even);   inside <=> 0 <= r_a <= dim_a - 1 on all three axes
//   mask and weight (order 0 always), k = mask[r], lit = inside && (image[r][0] != 0 || d.keep_dark):
//     y[c] = lit && k == c ? lut[255] : lut[0];   w[c] = lit ? lut[weight[r]] : lut[0]   (a class id >= C sets no channel)
//   image, order 0:  X[c] = inside ? lut[image[r][c]] : lut[0]
//   image, order 1:  trilinear over the 8 neighbours of floorf(p), taps outside the volume count as 0, f_a = p_a - floorf(p_a),
//                    lerp a + f * (b - a) along x, then y, then z;  X[c] = fp16(v / 255.0f)
// Outside the volume: image 0, no class, weight 0 (the zero padding of the 2-D producer's rotation).  Memory is read only behind the
// inside tests.  One lane per output voxel along x, a wave per (oz, oy) row; HBM-bound: (ch + 2 C) halves written and at most
// ch + 2 bytes (order 1: 8 ch + 2) gathered per voxel.
#include "patch_gather.h"

namespace {

struct PatchParams {
  const PatchDesc* descs;
  int B, ch, C, SZ, SY, SX, order;
  const f16* lut;                // fp16(float32(v / 255)) for v = 0..255
  f16* X; f16* y; f16* w;        // [B][ch][SZ][SY][SX], [B][C][SZ][SY][SX] twice
};

struct PatchStoreX {             // the image of patch_gather_voxel straight to X: lut[byte], or fp16(v / 255)
  const PatchParams& p;
  int b;
  long long vol, o;
  __device__ __forceinline__ f16& at(int c) { return p.X[((long long)b * p.ch + c) * vol + o]; }
  __device__ __forceinline__ void byte(int c, bool inside, const unsigned char* v, f16 zero) { at(c) = inside ? p.lut[*v] : zero; }
  __device__ __forceinline__ void value(int c, float v) { at(c) = (f16)(v / 255.0f); }
  __device__ __forceinline__ void nothing(int c, f16 zero) { at(c) = zero; }
};

__global__ __launch_bounds__(PATCH_TX * PATCH_TY) void patch_batch_kernel(PatchParams p) {
#pragma clang fp contract(off)
  const int ox = blockIdx.x * PATCH_TX + threadIdx.x, oy = blockIdx.y * PATCH_TY + threadIdx.y;
  const int b = blockIdx.z / p.SZ, oz = blockIdx.z - b * p.SZ;
  if (ox >= p.SX || oy >= p.SY) return;
  const float tz = (float)oz - 0.5f * (float)(p.SZ - 1), ty = (float)oy - 0.5f * (float)(p.SY - 1),
              tx = (float)ox - 0.5f * (float)(p.SX - 1);
  const long long vol = (long long)p.SZ * p.SY * p.SX, o = ((long long)oz * p.SY + oy) * p.SX + ox;
  PatchStoreX sink{p, b, vol, o};
  patch_gather_voxel(p, b, tz, ty, tx, vol, o, sink);
}

}  // namespace

extern "C" {

long long iunet_patch_desc_bytes(void) { return (long long)sizeof(PatchDesc); }

int iunet_patch_batch(const void* descs, int B, int ch, int C, int SZ, int SY, int SX, int order, const void* lut_f16, void* X,
                      void* y, void* w, void* stream) {
  IUNET_REQUIRE(descs && lut_f16 && X && y && w, "patch_batch: null pointer");
  PATCH_REQUIRE_RANGES("patch_batch", B, ch, C, SZ, SY, SX, order);
  PatchParams p;
  p.descs = (const PatchDesc*)descs; p.B = B; p.ch = ch; p.C = C; p.SZ = SZ; p.SY = SY; p.SX = SX; p.order = order;
  p.lut = (const f16*)lut_f16; p.X = (f16*)X; p.y = (f16*)y; p.w = (f16*)w;
  const dim3 grid((SX + PATCH_TX - 1) / PATCH_TX, (SY + PATCH_TY - 1) / PATCH_TY, B * SZ);
  hipLaunchKernelGGL(patch_batch_kernel, grid, dim3(PATCH_TX, PATCH_TY), 0, (hipStream_t)stream, p);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

}  // extern "C"
