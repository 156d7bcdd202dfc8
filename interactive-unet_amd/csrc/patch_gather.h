// One output voxel of the 3-D patch producers, written once: iunet_patch_batch (patch_batch.hip) evaluates it at the voxel's own
// centred patch coordinate t, iunet_patch_batch_extra (patch_augment.hip) at the elastically displaced t' = t + d.  The arithmetic,
// bit for bit (tests/patch_ref.py restates it in numpy float32: plain float32 multiplies and adds, each rounded, in exactly this
// order, no fma -- every body below is under its own `fp contract(off)`, the pragma is lexical):
//     p_a = ((d.m[3 a] * t_z + d.m[3 a + 1] * t_y) + d.m[3 a + 2] * t_x) + d.c[a]     a = 0, 1, 2: source axes z, y, x
//     r_a = rintf(p_a)   (ties to even);   inside <=> 0 <= r_a <= dim_a - 1 on all three axes
//   mask and weight (order 0 always), k = mask[r], lit = inside && (image[r][0] != 0 || d.keep_dark):
//     y[c] = lit && k == c ? lut[255] : lut[0];   w[c] = lit ? lut[weight[r]] : lut[0]   (a class id >= C sets no channel)
//   image, order 0:  the byte image[r][c] (none outside)
//   image, order 1:  trilinear over the 8 neighbours of floorf(p), taps outside the volume count as 0, f_a = p_a - floorf(p_a),
//                    lerp a + f * (b - a) along x, then y, then z: the value v in [0, 255]
// y and w are stored here in final form; what becomes of the image is the caller's Sink:
//     sink.byte(c, inside, ptr, zero)   order 0: where the byte of channel c lies (to be read only if inside); zero = lut[0]
//     sink.value(c, v)                  order 1: the interpolated value
//     sink.nothing(c, zero)             order 1, every tap outside the volume
// Memory is read only behind the inside tests.
#pragma once
#include "common.h"

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

// the range checks both entry points share; SY's bound is the grid's (PATCH_TY rows a block)
#define PATCH_REQUIRE_RANGES(who, B, ch, C, SZ, SY, SX, order)                                                                          \
  do {                                                                                                                                  \
    IUNET_REQUIRE(B >= 1 && ch >= 1 && ch <= 4 && C >= 1 && C <= 16, who ": B %d, channels %d (1 .. 4), classes %d (1 .. 16)", B, ch, C); \
    IUNET_REQUIRE(SZ >= 1 && SY >= 1 && SX >= 1 && SZ <= 65535 && SY <= 65535 * PATCH_TY && SX <= (1 << 20),                           \
                  who ": patch %d x %d x %d", SZ, SY, SX);                                                                              \
    IUNET_REQUIRE(order == 0 || order == 1, who ": spline order %d (0 or 1)", order);                                                   \
    IUNET_REQUIRE((long long)B * SZ <= 65535, who ": B * SZ = %lld exceeds the grid limit 65535", (long long)B * SZ);                   \
  } while (0)

// voxel o (its offset in the [SZ][SY][SX] patch of `vol` voxels) of sample b at centred patch coordinate (tz, ty, tx).  P: the
// kernel's parameter struct -- descs, ch, C, order, lut, y, w ([B][C][SZ][SY][SX]) are read from it
template <typename P, typename Sink>
__device__ __forceinline__ void patch_gather_voxel(const P& p, int b, float tz, float ty, float tx, long long vol, long long o, Sink& sink) {
#pragma clang fp contract(off)
  const PatchDesc& d = p.descs[b];
  const int ch = p.ch;
  const f16* lut = p.lut;
  const int Z = d.Z, Y = d.Y, X = d.X;
  const float pz = patch_coord(d.m, tz, ty, tx, d.c[0]), py = patch_coord(d.m + 3, tz, ty, tx, d.c[1]),
              px = patch_coord(d.m + 6, tz, ty, tx, d.c[2]);
  const float fz = rintf(pz), fy = rintf(py), fx = rintf(px);
  const bool inside = fz >= 0.f && fz <= (float)(Z - 1) && fy >= 0.f && fy <= (float)(Y - 1) && fx >= 0.f && fx <= (float)(X - 1);
  const long long src = inside ? ((long long)(int)fz * Y + (int)fy) * X + (int)fx : 0;
  const f16 zero = lut[0], one = lut[255];

  // mask and weight: the nearest voxel, whatever the image's order
  bool lit = false;
  if (inside) lit = d.image[src * ch] != 0 || d.keep_dark;
  const int k = lit ? (int)d.mask[src] : -1;
  const f16 wv = lit ? lut[d.weight[src * d.wstride]] : zero;
  for (int c = 0; c < p.C; ++c) {
    p.y[((long long)b * p.C + c) * vol + o] = k == c ? one : zero;
    p.w[((long long)b * p.C + c) * vol + o] = wv;
  }

  if (p.order == 0) {
    for (int c = 0; c < ch; ++c) sink.byte(c, inside, d.image + (src * ch + c), zero);
    return;
  }
  // order 1: the 8 neighbours of floor(p); a tap outside the volume is 0
  const float lz = floorf(pz), ly = floorf(py), lx = floorf(px);
  const bool any = lz >= -1.f && lz <= (float)(Z - 1) && ly >= -1.f && ly <= (float)(Y - 1) && lx >= -1.f && lx <= (float)(X - 1);
  if (!any) {                                          // every tap is outside: all lerps give 0
    for (int c = 0; c < ch; ++c) sink.nothing(c, zero);
    return;
  }
  const float gz = pz - lz, gy = py - ly, gx = px - lx;
  const int z0 = (int)lz, y0 = (int)ly, x0 = (int)lx;
  const bool zin[2] = {z0 >= 0, z0 + 1 <= Z - 1}, yin[2] = {y0 >= 0, y0 + 1 <= Y - 1}, xin[2] = {x0 >= 0, x0 + 1 <= X - 1};
  const long long base = ((long long)z0 * Y + y0) * X + x0;          // may point outside: only offsets of taps that are inside are used
  for (int c = 0; c < ch; ++c) {
    float v[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int dz = t >> 2, dy = (t >> 1) & 1, dx = t & 1;
      const bool ok = zin[dz] && yin[dy] && xin[dx];
      const long long off = base + ((long long)dz * Y + dy) * X + dx;
      v[t] = ok ? (float)d.image[off * ch + c] : 0.f;
    }
    const float x00 = patch_lerp(v[0], v[1], gx), x01 = patch_lerp(v[2], v[3], gx), x10 = patch_lerp(v[4], v[5], gx),
                x11 = patch_lerp(v[6], v[7], gx);
    const float y0v = patch_lerp(x00, x01, gy), y1v = patch_lerp(x10, x11, gy);
    sink.value(c, patch_lerp(y0v, y1v, gz));
  }
}
