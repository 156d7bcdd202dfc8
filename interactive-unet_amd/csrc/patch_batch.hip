// 3-D patch batch producer: the 3-D form of VolumeData.sample + load_resliced_annotations
// (volumedata.py:68-80, loader.py:48-82) as ONE gather launch per batch -- random oblique patches of uint8 image / mask / weight
// volumes, image at spline order 0 or 1, mask and weight at order 0, as the fp16 (X, y, w) a dim = 3 training step takes.
//
// The arithmetic, bit for bit (tests/patch_ref.py restates it in numpy float32: plain float32 multiplies and adds, each rounded,
// in exactly this order, no fma -- the file is compiled with contraction off):
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
#include "common.h"

namespace {

struct PatchDesc {               // one sample of the batch (mirrored by interactive_unet/loader.py: PatchDesc)
  const unsigned char* image;    // uint8 [Z][Y][X][ch]
  const unsigned char* mask;     // uint8 [Z][Y][X] class ids
  const unsigned char* weight;   // uint8 [Z][Y][X], element stride wstride (channel k of a [Z][Y][X][2] volume: base + k, stride 2)
  int wstride;
  int Z, Y, X;
  float m[9];                    // row-major 3 x 3: rows = source axes z, y, x; columns = patch axes z, y, x
  float c[3];                    // source coordinate of the patch centre
  int keep_dark;                 // 1: mask / weight are NOT zeroed where image channel 0 is 0
};

struct PatchParams {
  const PatchDesc* descs;
  int B, ch, C, SZ, SY, SX, order;
  const f16* lut;                // fp16(float32(v / 255)) for v = 0..255
  f16* X; f16* y; f16* w;        // [B][ch][SZ][SY][SX], [B][C][SZ][SY][SX] twice
};

constexpr int PATCH_TX = 64, PATCH_TY = 4;       // a block: 4 rows (oy) of 64 voxels along x

__device__ __forceinline__ float patch_coord(const float* m, float tz, float ty, float tx, float c) {
#pragma clang fp contract(off)
  const float a = m[0] * tz, b = m[1] * ty, e = m[2] * tx;
  return ((a + b) + e) + c;
}
__device__ __forceinline__ float patch_lerp(float a, float b, float f) {
#pragma clang fp contract(off)
  const float d = b - a, s = f * d;
  return a + s;
}

__global__ __launch_bounds__(PATCH_TX * PATCH_TY) void patch_batch_kernel(PatchParams p) {
#pragma clang fp contract(off)
  const int ox = blockIdx.x * PATCH_TX + threadIdx.x, oy = blockIdx.y * PATCH_TY + threadIdx.y;
  const int b = blockIdx.z / p.SZ, oz = blockIdx.z - b * p.SZ;
  if (ox >= p.SX || oy >= p.SY) return;
  const PatchDesc& d = p.descs[b];
  const int Z = d.Z, Y = d.Y, X = d.X;
  const float tz = (float)oz - 0.5f * (float)(p.SZ - 1), ty = (float)oy - 0.5f * (float)(p.SY - 1),
              tx = (float)ox - 0.5f * (float)(p.SX - 1);
  const float pz = patch_coord(d.m, tz, ty, tx, d.c[0]), py = patch_coord(d.m + 3, tz, ty, tx, d.c[1]),
              px = patch_coord(d.m + 6, tz, ty, tx, d.c[2]);
  const float fz = rintf(pz), fy = rintf(py), fx = rintf(px);
  const bool inside = fz >= 0.f && fz <= (float)(Z - 1) && fy >= 0.f && fy <= (float)(Y - 1) && fx >= 0.f && fx <= (float)(X - 1);
  const long long src = inside ? ((long long)(int)fz * Y + (int)fy) * X + (int)fx : 0;
  const long long vol = (long long)p.SZ * p.SY * p.SX, o = ((long long)oz * p.SY + oy) * p.SX + ox;
  const f16 zero = p.lut[0], one = p.lut[255];

  // mask and weight: the nearest voxel, whatever the image's order
  bool lit = false;
  if (inside) lit = d.image[src * p.ch] != 0 || d.keep_dark;
  const int k = lit ? (int)d.mask[src] : -1;
  const f16 wv = lit ? p.lut[d.weight[src * d.wstride]] : zero;
  for (int c = 0; c < p.C; ++c) {
    p.y[((long long)b * p.C + c) * vol + o] = k == c ? one : zero;
    p.w[((long long)b * p.C + c) * vol + o] = wv;
  }

  if (p.order == 0) {
    for (int c = 0; c < p.ch; ++c) p.X[((long long)b * p.ch + c) * vol + o] = inside ? p.lut[d.image[src * p.ch + c]] : zero;
    return;
  }
  // order 1: the 8 neighbours of floor(p); a tap outside the volume is 0
  const float lz = floorf(pz), ly = floorf(py), lx = floorf(px);
  const bool any = lz >= -1.f && lz <= (float)(Z - 1) && ly >= -1.f && ly <= (float)(Y - 1) && lx >= -1.f && lx <= (float)(X - 1);
  if (!any) {                                          // every tap is outside: all lerps give 0
    for (int c = 0; c < p.ch; ++c) p.X[((long long)b * p.ch + c) * vol + o] = zero;
    return;
  }
  const float gz = pz - lz, gy = py - ly, gx = px - lx;
  const int z0 = (int)lz, y0 = (int)ly, x0 = (int)lx;
  const bool zin[2] = {z0 >= 0, z0 + 1 <= Z - 1}, yin[2] = {y0 >= 0, y0 + 1 <= Y - 1}, xin[2] = {x0 >= 0, x0 + 1 <= X - 1};
  const long long base = ((long long)z0 * Y + y0) * X + x0;          // may point outside: only offsets of taps that are inside are used
  for (int c = 0; c < p.ch; ++c) {
    float v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int dz = t >> 2, dy = (t >> 1) & 1, dx = t & 1;
      const bool ok = zin[dz] && yin[dy] && xin[dx];
      const long long off = base + ((long long)dz * Y + dy) * X + dx;
      v[t] = ok ? (float)d.image[off * p.ch + c] : 0.f;
    }
    const float x00 = patch_lerp(v[0], v[1], gx), x01 = patch_lerp(v[2], v[3], gx), x10 = patch_lerp(v[4], v[5], gx),
                x11 = patch_lerp(v[6], v[7], gx);
    const float y0v = patch_lerp(x00, x01, gy), y1v = patch_lerp(x10, x11, gy);
    const float val = patch_lerp(y0v, y1v, gz);
    p.X[((long long)b * p.ch + c) * vol + o] = (f16)(val / 255.0f);
  }
}

}  // namespace

extern "C" {

long long iunet_patch_desc_bytes(void) { return (long long)sizeof(PatchDesc); }

int iunet_patch_batch(const void* descs, int B, int ch, int C, int SZ, int SY, int SX, int order, const void* lut_f16, void* X,
                      void* y, void* w, void* stream) {
  IUNET_REQUIRE(descs && lut_f16 && X && y && w, "patch_batch: null pointer");
  IUNET_REQUIRE(B >= 1 && ch >= 1 && ch <= 4 && C >= 1 && C <= 16, "patch_batch: B %d, channels %d (1 .. 4), classes %d (1 .. 16)", B, ch, C);
  IUNET_REQUIRE(SZ >= 1 && SY >= 1 && SX >= 1 && SZ <= 65535 && SY <= 65535 * PATCH_TY && SX <= (1 << 20),
                "patch_batch: patch %d x %d x %d", SZ, SY, SX);
  IUNET_REQUIRE(order == 0 || order == 1, "patch_batch: spline order %d (0 or 1)", order);
  IUNET_REQUIRE((long long)B * SZ <= 65535, "patch_batch: B * SZ = %lld exceeds the grid limit 65535", (long long)B * SZ);
  PatchParams p;
  p.descs = (const PatchDesc*)descs; p.B = B; p.ch = ch; p.C = C; p.SZ = SZ; p.SY = SY; p.SX = SX; p.order = order;
  p.lut = (const f16*)lut_f16; p.X = (f16*)X; p.y = (f16*)y; p.w = (f16*)w;
  const dim3 grid((SX + PATCH_TX - 1) / PATCH_TX, (SY + PATCH_TY - 1) / PATCH_TY, B * SZ);
  hipLaunchKernelGGL(patch_batch_kernel, grid, dim3(PATCH_TX, PATCH_TY), 0, (hipStream_t)stream, p);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

}  // extern "C"
