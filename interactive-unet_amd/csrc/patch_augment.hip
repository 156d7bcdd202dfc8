// Elastic deformation, intensity jitter and "Gaussian blur or Gaussian noise" for the 3-D patch batch producer (DESIGN.md section
// 18): the three further transforms of the reference's list (loader.py:115-123) that section 17 gave the 2-D producer, in 3-D,
// through iunet_patch_batch_extra.  The definition is tests/patch_augment_ref.py: plain float32, every multiply and add rounded on
// its own (contraction is off for the whole file), Philox4x32-10 keyed per sample as the noise source -- counter (ox, oy, oz, 2 c)
// for elastic field c (0 / 1 / 2: the displacement along patch z / y / x), (ox, oy, oz, 2 q + 1) for the noise of image channel q.
// The producer samples the volume at a continuous coordinate anyway, so the deformation is a displacement d of the centred patch
// coordinate, t' = t + d (not rounded), and costs no second resampling.  The data dependencies make a pipeline on one stream, nothing
// goes through the host; `use` leaves out what no sample of the batch needs:
//   elastic_x_kernel           (elastic)  the three noise fields' K-tap pass along x; the noise of a row segment plus r on each side
//                                         is generated once into LDS                                -> fp32 A [B][3][SZ][SY][SX]
//   elastic_axis_kernel  x 2   (elastic)  the passes along y (A -> B) and z (B -> A, times a2) through LDS tiles with a halo of r
//                                         along the pass axis: d
//   patch_gather_extra_kernel             patch_gather.h's voxel at t + d: y and w in final form; X directly for a sample with no
//                                         image transform, else the float32 image -> [B][ch][SZ][SY][SX] and (jitter) the 256-bin
//                                         histogram of its bytes, per block in LDS, merged with integer atomics
//   jitter_mean_kernel         (jitter)   the contrast mean from the histogram, in float64 in ascending byte value by ONE lane
//   patch_finish_kernel        (any image transform)  jitter as a tile is loaded, the three 5-tap passes inside the tile (halo 2 on
//                                         every axis), or Box-Muller noise; one fp16 store
// No float atomics anywhere: a repeated call gives the same bits.  Lanes run along x.  What this pipeline has in common with the 2-D
// batch producer's (augment.hip) -- Philox, the jitter, the contrast mean, the histogram, the elastic passes, the entry point's
// checks -- is in augment_common.h.
#include "augment_common.h"
#include "patch_gather.h"

#pragma clang fp contract(off)

namespace {

struct PatchExtraDesc {          // one sample's further transforms (mirrored by interactive_unet/loader.py: PatchExtraDesc)
  int flags;                     // AUG_ELASTIC | AUG_JITTER where the sample has them
  int kind;                      // 0 neither, 1 blur, 2 noise
  unsigned ekey[2];              // elastic Philox key: low word, high word
  float a2;                      // float32(alpha / 2)
  float brightness, contrast;
  int contrast_first;
  float taps[5];                 // blur: the five float32 taps
  unsigned nkey[2];              // noise Philox key
  float sigma_n;
};

struct PatchExtraParams {
  const PatchDesc* descs;
  const PatchExtraDesc* extras;
  int use, B, ch, C, SZ, SY, SX, order, K;
  const f16* lut;                // fp16(float32(v / 255))
  const float* taps;             // K float32 taps of the elastic Gaussian
  float* fa; float* fb;          // workspace: the noise fields, [B][3][SZ][SY][SX] each: x pass -> fa, y pass -> fb, z pass -> fa = d
  float* img;                    // workspace: the float32 image before jitter / blur / noise, [B][ch][SZ][SY][SX]
  unsigned* hist;                // workspace: [B][256], zeroed before the gather
  float* mean;                   // workspace: [B]
  f16* X; f16* y; f16* w;
};

struct PatchWorkspace { long long fa, fb, img, hist, mean, total; };      // byte offsets of the workspace's parts
inline PatchWorkspace patch_workspace(int B, int ch, int SZ, int SY, int SX) {
  const long long vol = (long long)SZ * SY * SX;
  PatchWorkspace s;
  s.fa = 0;
  s.fb = aug_align256(12 * B * vol);
  s.img = s.fb + aug_align256(12 * B * vol);
  s.hist = s.img + aug_align256(4 * B * ch * vol);
  s.mean = s.hist + 1024LL * B;
  s.total = s.mean + aug_align256(4LL * B);
  return s;
}

// Elastic, pass along x (augment_common.h: aug_row_pass).  A block: two rows (oy) of 128 voxels of one z plane of one elastic sample,
// a line of LDS each, the three fields; counter (x, oy, oz, 2 c).
constexpr int PA_XT = 128, PA_XR = 2;
__global__ __launch_bounds__(PA_XT * PA_XR) void elastic_x_kernel(PatchExtraParams p) {
  __shared__ float noise[PA_XR][PA_XT + AUG_MAX_TAPS - 1];
  const int b = blockIdx.z / p.SZ, oz = blockIdx.z - b * p.SZ;
  const PatchExtraDesc& e = p.extras[b];
  if (!(e.flags & AUG_ELASTIC)) return;              // the same in every lane of the block
  const int x0 = blockIdx.x * PA_XT, oy = blockIdx.y * PA_XR + threadIdx.y, ox = x0 + threadIdx.x;
  const bool row = oy < p.SY;
  const unsigned k0 = e.ekey[0], k1 = e.ekey[1];
  const long long vol = (long long)p.SZ * p.SY * p.SX;
  for (int c = 0; c < 3; ++c) {
    const float acc = aug_row_pass<PA_XT>(noise[threadIdx.y], threadIdx.x, row, x0, p.SX, (unsigned)oy, (unsigned)oz, (unsigned)(2 * c), k0, k1,
                                          p.taps, p.K);
    if (row && ox < p.SX) p.fa[((long long)b * 3 + c) * vol + ((long long)oz * p.SY + oy) * p.SX + ox] = acc;
    __syncthreads();
  }
}

// Elastic, pass along y or z (augment_common.h: aug_tile_pass; `axis`: nA voxels, sA elements apart; the other of the two: nO voxels,
// sO apart).  A block: a tile of 64 voxels along x by 32 along the axis, at one position of the other axis, of one elastic sample, the
// three fields.  `last`: the result is multiplied by a2 -- the displacement.
__global__ __launch_bounds__(AUG_TILE_LANES) void elastic_axis_kernel(PatchExtraParams p, const float* src, float* dst, int nA, long long sA,
                                                                      int nO, long long sO, int last) {
  __shared__ float tile[AUG_TILE_FLOATS];
  const int b = blockIdx.z / nO, other = blockIdx.z - b * nO;
  const PatchExtraDesc& e = p.extras[b];
  if (!(e.flags & AUG_ELASTIC)) return;              // the same in every lane of the block
  const int x0 = blockIdx.x * AUG_TILE_X, a0 = blockIdx.y * AUG_TILE_A;
  const long long vol = (long long)p.SZ * p.SY * p.SX;
  const float a2 = e.a2;
  for (int c = 0; c < 3; ++c) {
    const long long base = ((long long)b * 3 + c) * vol + other * sO;
    aug_tile_pass(tile, src + base, x0, a0, p.SX, nA, sA, p.taps, p.K,
                  [&](int, int oa, int ox, float acc) { dst[base + oa * sA + ox] = last ? acc * a2 : acc; });
  }
}

// The image of patch_gather_voxel for a sample of the extended batch: straight to X where the sample has no image transform (the
// bits of iunet_patch_batch), else the float32 value that iunet_patch_batch rounds to fp16 -- order 0: float32(byte / 255), 0
// outside; order 1: v / 255 -- into the workspace, and for a jitter sample its byte (order 1: rint(v), ties to even) into the
// block's histogram.
struct PatchStoreExtra {
  const PatchExtraParams& p;
  int b;
  long long vol, o;
  unsigned* hist;                // the block's 256 bins in LDS, or null
  bool direct;
  __device__ __forceinline__ long long at(int c) const { return ((long long)b * p.ch + c) * vol + o; }
  __device__ __forceinline__ void put(int c, float x, int v) {
    p.img[at(c)] = x;
    if (hist) atomicAdd(&hist[v], 1u);
  }
  __device__ __forceinline__ void byte(int c, bool inside, const unsigned char* ptr, f16 zero) {
    const unsigned char v = inside ? *ptr : (unsigned char)0;
    if (direct) p.X[at(c)] = inside ? p.lut[v] : zero;
    else put(c, (float)v / 255.0f, v);
  }
  __device__ __forceinline__ void value(int c, float v) {
    if (direct) p.X[at(c)] = (f16)(v / 255.0f);
    else put(c, v / 255.0f, min(max((int)rintf(v), 0), 255));
  }
  __device__ __forceinline__ void nothing(int c, f16 zero) {
    if (direct) p.X[at(c)] = zero;
    else put(c, 0.f, 0);
  }
};

// The gather: patch_batch_kernel's voxel behind a prologue that adds an elastic sample's displacement to the centred coordinate.
// One lane per voxel along x, a wave per row as there, but a block walks PA_GATHER_ROWS groups of PATCH_TY rows: every block of a
// jitter sample adds up to 256 counts to its sample's 256 words, and with 2 048 voxels a block those atomics are not the cost.
constexpr int PA_GATHER_ROWS = 8;
__global__ __launch_bounds__(PATCH_TX * PATCH_TY) void patch_gather_extra_kernel(PatchExtraParams p) {
  __shared__ unsigned hist[256];
  const int tid = threadIdx.y * PATCH_TX + threadIdx.x;
  const int b = blockIdx.z / p.SZ, oz = blockIdx.z - b * p.SZ, ox = blockIdx.x * PATCH_TX + threadIdx.x;
  const PatchExtraDesc& e = p.extras[b];
  const bool elastic = p.use & e.flags & AUG_ELASTIC, jitter = p.use & e.flags & AUG_JITTER;
  const bool direct = !jitter && !((e.kind == 1 && (p.use & AUG_BLUR)) || (e.kind == 2 && (p.use & AUG_NOISE)));
  if (jitter) aug_hist_zero(hist, tid);
  const long long vol = (long long)p.SZ * p.SY * p.SX;
  const float tz = (float)oz - 0.5f * (float)(p.SZ - 1), tx = (float)ox - 0.5f * (float)(p.SX - 1);
  for (int q = 0; q < PA_GATHER_ROWS; ++q) {
    const int oy = (blockIdx.y * PA_GATHER_ROWS + q) * PATCH_TY + threadIdx.y;
    if (ox >= p.SX || oy >= p.SY) continue;
    const long long o = ((long long)oz * p.SY + oy) * p.SX + ox;
    const float ty = (float)oy - 0.5f * (float)(p.SY - 1);
    float ez = tz, ey = ty, ex = tx;
    if (elastic) {
      const float* d = p.fa + (long long)b * 3 * vol + o;
      ez = tz + d[0]; ey = ty + d[vol]; ex = tx + d[2 * vol];
    }
    PatchStoreExtra sink{p, b, vol, o, jitter ? hist : nullptr, direct};
    patch_gather_voxel(p, b, ez, ey, ex, vol, o, sink);
  }
  if (jitter) aug_hist_flush(hist, tid, p.hist + (long long)b * 256);
}

// The contrast mean of a jitter sample (augment_common.h: aug_contrast_mean): one block per sample, one lane per byte value v,
// L = float32(v / 255) by one float32 division.
__global__ __launch_bounds__(256) void jitter_mean_kernel(PatchExtraParams p) {
  __shared__ double term[256];
  const int b = blockIdx.x, v = threadIdx.x;
  const PatchExtraDesc& e = p.extras[b];
  if (!(e.flags & AUG_JITTER)) return;
  const float m = aug_contrast_mean(p.hist + (long long)b * 256, v, (float)v / 255.0f, e.brightness, e.contrast_first != 0,
                                    (long long)p.ch * p.SZ * p.SY * p.SX, term);
  if (v == 0) p.mean[b] = m;
}

// X of a sample with an image transform, from the workspace image.  A block: a tile of 4 x 8 x 64 voxels (z, y, x) of one sample.
// Blur: the tile plus 2 on every side (reflected at the patch's borders) is loaded into LDS, jittered on the way -- jitter is
// pointwise, so the blur's neighbours are jittered on load --, the three 5-tap passes run inside it (x: every row of the haloed
// tile; y: every plane; z), ascending taps.  Reflection commutes with the passes that came before: the x pass of a reflected row is
// the reflected row of the x pass.  Noise: Box-Muller on two Philox words with the library's sqrtf / logf / cosf, whose last-ulp
// differences from a correctly rounded pair are the one place the output may leave the definition, by one fp16 step.  Jitter alone:
// pointwise, no tile.
constexpr int PF_Z = 4, PF_Y = 8, PF_X = 64, PF_H = 2;
constexpr int PF_ZH = PF_Z + 2 * PF_H, PF_YH = PF_Y + 2 * PF_H, PF_XH = PF_X + 2 * PF_H;
__global__ __launch_bounds__(256) void patch_finish_kernel(PatchExtraParams p, int ztiles) {
  __shared__ float S0[PF_ZH * PF_YH * PF_XH];        // the haloed tile; after the y pass: [PF_ZH][PF_Y][PF_X]
  __shared__ float S1[PF_ZH * PF_YH * PF_X];         // after the x pass: [PF_ZH][PF_YH][PF_X]
  const int b = blockIdx.z / ztiles, z0 = (blockIdx.z - b * ztiles) * PF_Z, y0 = blockIdx.y * PF_Y, x0 = blockIdx.x * PF_X;
  const PatchExtraDesc& e = p.extras[b];
  const bool jitter = p.use & e.flags & AUG_JITTER;
  const int kind = (e.kind == 1 && (p.use & AUG_BLUR)) ? 1 : (e.kind == 2 && (p.use & AUG_NOISE)) ? 2 : 0;
  if (!jitter && kind == 0) return;                  // the gather wrote X; the same in every lane of the block
  const int SZ = p.SZ, SY = p.SY, SX = p.SX;
  const long long vol = (long long)SZ * SY * SX;
  const float br = e.brightness, co = e.contrast, m = jitter ? p.mean[b] : 0.f;
  const bool cf = e.contrast_first != 0;
  const int tid = threadIdx.x;
  for (int q = 0; q < p.ch; ++q) {
    const float* src = p.img + ((long long)b * p.ch + q) * vol;
    f16* dst = p.X + ((long long)b * p.ch + q) * vol;
    if (kind == 1) {
      float k[5];
#pragma unroll
      for (int i = 0; i < 5; ++i) k[i] = e.taps[i];
      for (int t = tid; t < PF_ZH * PF_YH * PF_XH; t += 256) {
        const int lx = t % PF_XH, ly = (t / PF_XH) % PF_YH, lz = t / (PF_XH * PF_YH);
        const int gx = x0 - PF_H + lx, gy = y0 - PF_H + ly, gz = z0 - PF_H + lz;
        float v = 0.f;                               // beyond the halo of the patch's last voxel: read by no output that is stored
        if (gx < SX + PF_H && gy < SY + PF_H && gz < SZ + PF_H) {
          v = src[((long long)aug_reflect(gz, SZ) * SY + aug_reflect(gy, SY)) * SX + aug_reflect(gx, SX)];
          if (jitter) v = aug_jitter(v, br, co, cf, m);
        }
        S0[t] = v;
      }
      __syncthreads();
      for (int t = tid; t < PF_ZH * PF_YH * PF_X; t += 256) {          // x: every row of the haloed tile
        const int x = t % PF_X, row = t / PF_X;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 5; ++i) acc += k[i] * S0[row * PF_XH + x + i];
        S1[t] = acc;
      }
      __syncthreads();
      for (int t = tid; t < PF_ZH * PF_Y * PF_X; t += 256) {           // y
        const int x = t % PF_X, y = (t / PF_X) % PF_Y, lz = t / (PF_X * PF_Y);
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 5; ++i) acc += k[i] * S1[(lz * PF_YH + y + i) * PF_X + x];
        S0[t] = acc;
      }
      __syncthreads();
      for (int t = tid; t < PF_Z * PF_Y * PF_X; t += 256) {            // z, and the store
        const int x = t % PF_X, y = (t / PF_X) % PF_Y, z = t / (PF_X * PF_Y);
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 5; ++i) acc += k[i] * S0[((z + i) * PF_Y + y) * PF_X + x];
        const int ox = x0 + x, oy = y0 + y, oz = z0 + z;
        if (ox < SX && oy < SY && oz < SZ) dst[((long long)oz * SY + oy) * SX + ox] = (f16)acc;
      }
      __syncthreads();                               // the next channel's load overwrites S0
    } else {
      for (int t = tid; t < PF_Z * PF_Y * PF_X; t += 256) {
        const int ox = x0 + t % PF_X, oy = y0 + (t / PF_X) % PF_Y, oz = z0 + t / (PF_X * PF_Y);
        if (ox >= SX || oy >= SY || oz >= SZ) continue;
        const long long o = ((long long)oz * SY + oy) * SX + ox;
        float v = src[o];
        if (jitter) v = aug_jitter(v, br, co, cf, m);
        if (kind == 2) {
          unsigned w0, w1;
          philox4x32_10((unsigned)ox, (unsigned)oy, (unsigned)oz, (unsigned)(2 * q + 1), e.nkey[0], e.nkey[1], w0, w1);
          v = aug_clamp01(v + e.sigma_n * aug_gauss(w0, w1));
        }
        dst[o] = (f16)v;
      }
    }
  }
}

}  // namespace

extern "C" {

long long iunet_patch_extra_desc_bytes(void) { return (long long)sizeof(PatchExtraDesc); }

long long iunet_patch_extra_ws_bytes(int B, int ch, int SZ, int SY, int SX) {
  if (!(B >= 1 && ch >= 1 && ch <= 4 && SZ >= 1 && SY >= 1 && SX >= 1 && SZ <= 65535 && SY <= 65535 * PATCH_TY && SX <= (1 << 20) &&
        (long long)B * SZ <= 65535)) {
    iunet_set_error("patch_extra_ws_bytes: B %d, channels %d, patch %d x %d x %d", B, ch, SZ, SY, SX);
    return IUNET_ERR_ARG;
  }
  return patch_workspace(B, ch, SZ, SY, SX).total;
}

int iunet_patch_batch_extra(const void* descs, const void* extras, int use, int B, int ch, int C, int SZ, int SY, int SX, int order,
                            const void* lut_f16, const void* taps_f32, int K, void* ws, long long ws_bytes, void* X, void* y, void* w,
                            void* stream) {
  IUNET_REQUIRE(descs && extras && lut_f16 && ws && X && y && w, "patch_batch_extra: null pointer");
  PATCH_REQUIRE_RANGES("patch_batch_extra", B, ch, C, SZ, SY, SX, order);
  const PatchWorkspace s = patch_workspace(B, ch, SZ, SY, SX);
  char shape[64];
  snprintf(shape, sizeof shape, "%d x %d x %d patch", SZ, SY, SX);
  const int rc = aug_check_extra("patch_batch_extra", shape, use, taps_f32, K, SZ < SY ? (SZ < SX ? SZ : SX) : (SY < SX ? SY : SX), ws_bytes, s.total,
                                 "iunet_patch_extra_ws_bytes", "extent");
  if (rc != IUNET_OK) return rc;
  if (use & AUG_ELASTIC)
    IUNET_REQUIRE((long long)B * SY <= 65535, "patch_batch_extra: B * SY = %lld exceeds the grid limit 65535 of the elastic passes", (long long)B * SY);
  PatchExtraParams p;
  p.descs = (const PatchDesc*)descs; p.extras = (const PatchExtraDesc*)extras;
  p.use = use; p.B = B; p.ch = ch; p.C = C; p.SZ = SZ; p.SY = SY; p.SX = SX; p.order = order; p.K = (use & AUG_ELASTIC) ? K : 1;
  p.lut = (const f16*)lut_f16; p.taps = (const float*)taps_f32;
  char* base = (char*)ws;
  p.fa = (float*)(base + s.fa); p.fb = (float*)(base + s.fb); p.img = (float*)(base + s.img); p.hist = (unsigned*)(base + s.hist);
  p.mean = (float*)(base + s.mean);
  p.X = (f16*)X; p.y = (f16*)y; p.w = (f16*)w;
  const hipStream_t st = (hipStream_t)stream;
  const int xt = (SX + AUG_TILE_X - 1) / AUG_TILE_X;
  if (use & AUG_ELASTIC) {
    const long long sY = SX, sZ = (long long)SY * SX;
    hipLaunchKernelGGL(elastic_x_kernel, dim3((SX + PA_XT - 1) / PA_XT, (SY + PA_XR - 1) / PA_XR, B * SZ), dim3(PA_XT, PA_XR), 0, st, p);
    hipLaunchKernelGGL(elastic_axis_kernel, dim3(xt, (SY + AUG_TILE_A - 1) / AUG_TILE_A, B * SZ), dim3(256), 0, st, p, (const float*)p.fa,
                       p.fb, SY, sY, SZ, sZ, 0);
    hipLaunchKernelGGL(elastic_axis_kernel, dim3(xt, (SZ + AUG_TILE_A - 1) / AUG_TILE_A, B * SY), dim3(256), 0, st, p, (const float*)p.fb,
                       p.fa, SZ, sZ, SY, sY, 1);
  }
  if (use & AUG_JITTER) IUNET_CHECK_HIP(hipMemsetAsync(p.hist, 0, 1024 * (size_t)B, st));
  hipLaunchKernelGGL(patch_gather_extra_kernel, dim3((SX + PATCH_TX - 1) / PATCH_TX, (SY + PATCH_TY * PA_GATHER_ROWS - 1) / (PATCH_TY * PA_GATHER_ROWS), B * SZ),
                     dim3(PATCH_TX, PATCH_TY), 0, st, p);
  if (use & AUG_JITTER) hipLaunchKernelGGL(jitter_mean_kernel, dim3(B), dim3(256), 0, st, p);
  if (use & (AUG_JITTER | AUG_BLUR | AUG_NOISE)) {
    const int ztiles = (SZ + PF_Z - 1) / PF_Z;
    hipLaunchKernelGGL(patch_finish_kernel, dim3((SX + PF_X - 1) / PF_X, (SY + PF_Y - 1) / PF_Y, B * ztiles), dim3(256), 0, st, p, ztiles);
  }
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

}  // extern "C"
