// Batch producer on the device: the reference's loader contract as ONE gather launch per batch.
//   interactive_unet/loader.py:32-42    image / mask / weight uint8 -> value / 255 (float64 -> float32), weight repeated over the
//                                       classes, mask and weight zeroed where image[0] == 0
//   interactive_unet/loader.py:125-133  RandomHorizontalFlip, RandomVerticalFlip, RandomRotation(NEAREST), RandomResizedCrop(NEAREST)
//   interactive_unet/loader.py:138-154  the same parameters for the three tensors; float16 out, channels first
// All four transforms are nearest-neighbour index maps, so their composition is one source pixel (or none: the rotation's
// zero padding) per output pixel.  The index arithmetic is torchvision's (not under /root/reference; restated in
// oracle/loader_ref.py, which checks it against torch's own grid_sample / interpolate): crop + interpolate(mode='nearest')
// -> pixel of the rotated image: min(floor(o * (h / out)), h - 1) in float32; rotation: the affine grid g = fma(y, r1, x * r0)
// + r2 (the order torch's CPU bmm accumulates in), ((g + 1) * size - 1) / 2, rint, zero outside; flips last.
// HBM-bound: per output pixel ch + C + 1 source bytes read, (ch + 2 C) halves written.
//
// The three further transforms of the reference's list (loader.py:115-123): ElasticTransform(NEAREST),
// ColorJitter(brightness, contrast) and RandomChoice([GaussianBlur(5), GaussianNoise()]), through iunet_augment_batch_extra.  The
// definition is tests/augment_ref.py: plain float32, every multiply and add rounded on its own (contraction is off for the whole
// file; the affine grid's one fma is spelled out), Philox4x32-10 keyed per sample as the noise source.  The data dependencies make
// it a small pipeline on one stream, no device-to-host copy anywhere:
//   elastic_rows_kernel   (elastic in `use`)  the noise fields' horizontal K-tap pass -> fp32 [B][2][OH][OW]
//   elastic_cols_kernel   (elastic in `use`)  the vertical pass through an LDS tile -> the displaced pixel of every output pixel
//   augment_gather_kernel                     the chain above at the displaced pixel: y, w, the gathered image bytes G
//                                             [B][ch][OH][OW] and (jitter) their 256-bin histogram
//   jitter_table_kernel   (jitter in `use`)   T[b][256]: the exact mean from the histogram, brightness and contrast in drawn order
//   augment_finish_kernel                     X = fp16 of T[G], of its 5 x 5 blur, or of clamp(T[G] + sigma_n z)
// What this pipeline has in common with the 3-D patch producer's (patch_augment.hip) -- Philox, the jitter, the contrast mean, the
// histogram, the two elastic passes, the entry point's checks -- is in augment_common.h.
#include "augment_common.h"

#pragma clang fp contract(off)

namespace {

struct AugDesc {                 // one sample of the batch (mirrored by interactive_unet/loader.py: AugDesc)
  const unsigned char* image;    // uint8 [H][W][ch]
  const unsigned char* mask;     // uint8 [H][W][C]
  const unsigned char* weight;   // uint8 [H][W]
  const float* xg;               // torch.linspace((1 - W) / 2, (W - 1) / 2, W)
  const float* yg;               // torch.linspace((1 - H) / 2, (H - 1) / 2, H)
  int H, W;
  int hflip, vflip;
  int kind;                      // 0 affine grid, 1 identity, 2 rot90 k=2, 3 rot90 k=1, 4 rot90 k=3 (torchvision rotate fast paths)
  int ci, cj, ch, cw;            // crop of the rotated image: top, left, height, width
  float r[6];                    // theta^T / (W/2, H/2): r00 r10 r20 (x) r01 r11 r21 (y)
  int keep_dark;                 // 1: mask / weight are NOT zeroed where the image is 0 (the Suggestor's tensors)
};

struct AugParams {
  const AugDesc* descs;
  int B, ch, C, OH, OW;
  const f16* lut;                // fp16(float32(v / 255)) for v = 0..255
  f16* X; f16* y; f16* w;        // [B][ch][OH][OW], [B][C][OH][OW], [B][C][OH][OW]
};

// the crop / rotation / flip chain at output position (py, px): the source pixel's offset in its [H][W] plane, `ok` false where the
// rotation samples outside (zero padding).  (py, px) is the output pixel itself, or the pixel an elastic map displaced it to.
__device__ __forceinline__ long long aug_source(const AugDesc& d, int OH, int OW, int py, int px, bool& ok) {
  // resized crop: pixel (cy, cx) of the rotated image
  const float sy = (float)d.ch / (float)OH, sx = (float)d.cw / (float)OW;
  const int cy = d.ci + min((int)floorf((float)py * sy), d.ch - 1);
  const int cx = d.cj + min((int)floorf((float)px * sx), d.cw - 1);
  int ry, rx;
  ok = true;
  if (d.kind == 1) { ry = cy; rx = cx; }
  else if (d.kind == 2) { ry = d.H - 1 - cy; rx = d.W - 1 - cx; }
  else if (d.kind == 3) { ry = cx; rx = d.W - 1 - cy; }
  else if (d.kind == 4) { ry = d.H - 1 - cx; rx = cy; }
  else {
    const float X = d.xg[cx], Y = d.yg[cy];
    const float gx = __fmaf_rn(Y, d.r[1], X * d.r[0]) + d.r[2];
    const float gy = __fmaf_rn(Y, d.r[4], X * d.r[3]) + d.r[5];
    const float ix = ((gx + 1.f) * (float)d.W - 1.f) / 2.f;
    const float iy = ((gy + 1.f) * (float)d.H - 1.f) / 2.f;
    const float fx = rintf(ix), fy = rintf(iy);
    ok = fx >= 0.f && fx <= (float)(d.W - 1) && fy >= 0.f && fy <= (float)(d.H - 1);
    rx = ok ? (int)fx : 0; ry = ok ? (int)fy : 0;
  }
  if (d.vflip) ry = d.H - 1 - ry;
  if (d.hflip) rx = d.W - 1 - rx;
  return (long long)ry * d.W + rx;
}

// Output pixel o (its offset in the [OH][OW] plane) of sample b, read at position (py, px) of the chain; ok_in false: (py, px) is
// outside already (displaced out of the output).  y and w are stored here in final form; every image byte (0 outside) goes to
// sink(its offset in [B][ch][OH][OW], byte).  P: the kernel's parameter struct -- ch, C, OH, OW, lut, y, w are read from it.
template <typename P, typename Sink>
__device__ __forceinline__ void aug_gather_pixel(const AugDesc& d, const P& p, int b, int py, int px, bool ok_in, long long o, Sink&& sink) {
  bool ok;
  const long long src = aug_source(d, p.OH, p.OW, py, px, ok);
  ok = ok && ok_in;
  const long long plane = (long long)p.OH * p.OW;
  const f16 zero = p.lut[0];
  bool lit = false;                                   // image[0] != 0 at the source pixel
  for (int c = 0; c < p.ch; ++c) {
    const unsigned char v = ok ? d.image[src * p.ch + c] : (unsigned char)0;
    if (c == 0) lit = ok && (v != 0 || d.keep_dark);
    sink(((long long)b * p.ch + c) * plane + o, v);
  }
  const f16 wv = lit ? p.lut[d.weight[src]] : zero;
  for (int c = 0; c < p.C; ++c) {
    p.y[((long long)b * p.C + c) * plane + o] = lit ? p.lut[d.mask[src * p.C + c]] : zero;
    p.w[((long long)b * p.C + c) * plane + o] = wv;
  }
}

// one lane per output pixel (four pixels per lane with 8-byte stores measured slower: 38 vs 25 us per batch of 8 -- the rows are
// only 512 pixels wide and the rotated gather loses its coalescing)
__global__ __launch_bounds__(256) void augment_batch_kernel(AugParams p) {
  const int ox = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y, b = blockIdx.z;
  if (ox >= p.OW) return;
  const AugDesc d = p.descs[b];
  aug_gather_pixel(d, p, b, oy, ox, true, (long long)oy * p.OW + ox, [&](long long at, unsigned char v) { p.X[at] = p.lut[v]; });
}

// ---- elastic, colour jitter, blur and noise (tests/augment_ref.py) ---------------------------------------------------------------
struct AugExtraDesc {            // one sample's further transforms (mirrored by interactive_unet/loader.py: AugExtraDesc)
  int flags;                     // AUG_ELASTIC | AUG_JITTER where the sample has them
  int kind;                      // 0 neither, 1 blur, 2 noise
  unsigned ekey[2];              // elastic Philox key: low word, high word
  float a2;                      // float32(alpha / 2)
  float brightness, contrast;
  int contrast_first;
  float w2[25];                  // blur: float32(k_i k_j), row-major
  unsigned nkey[2];              // noise Philox key
  float sigma_n;
};

struct AugExtraParams {
  const AugDesc* descs;
  const AugExtraDesc* extras;
  int use, B, ch, C, OH, OW, K;
  const f16* lut;                // fp16(float32(v / 255))
  const float* lut32;            // float32(v / 255)
  const float* taps;             // K float32 taps of the elastic Gaussian
  float* rows;                   // workspace: the noise fields after the horizontal pass, [B][2][OH][OW]
  unsigned* map;                 // workspace: the displaced pixel of every output pixel, [B][OH][OW]
  unsigned char* G;              // workspace: gathered image bytes [B][ch][OH][OW], outside = 0
  unsigned* hist;                // workspace: [B][256], zeroed before the gather
  float* T;                      // workspace: [B][256]
  f16* X; f16* y; f16* w;
};

struct AugWorkspace { long long rows, map, G, hist, T, total; };     // byte offsets of the workspace's parts
inline AugWorkspace aug_workspace(int B, int ch, int OH, int OW) {
  const long long plane = (long long)OH * OW;
  AugWorkspace s;
  s.rows = 0;
  s.map = aug_align256(8 * B * plane);
  s.G = s.map + aug_align256(4 * B * plane);
  s.hist = s.G + aug_align256(B * ch * plane);
  s.T = s.hist + 1024LL * B;
  s.total = s.T + 1024LL * B;
  return s;
}

// Elastic, horizontal pass (augment_common.h: aug_row_pass).  A block: 256 pixels of one row of one elastic sample, both fields;
// counter (x, y, c, 0).
__global__ __launch_bounds__(256) void elastic_rows_kernel(AugExtraParams p) {
  __shared__ float noise[256 + AUG_MAX_TAPS - 1];
  const int x0 = blockIdx.x * 256, y = blockIdx.y, b = blockIdx.z;
  const AugExtraDesc& e = p.extras[b];
  if (!(e.flags & AUG_ELASTIC)) return;              // the same in every lane of the block
  const unsigned k0 = e.ekey[0], k1 = e.ekey[1];
  const int ox = x0 + threadIdx.x;
  for (int c = 0; c < 2; ++c) {
    const float acc = aug_row_pass<256>(noise, threadIdx.x, true, x0, p.OW, (unsigned)y, (unsigned)c, 0u, k0, k1, p.taps, p.K);
    if (ox < p.OW) p.rows[(((long long)b * 2 + c) * p.OH + y) * p.OW + ox] = acc;
    __syncthreads();
  }
}

// Elastic, vertical pass (augment_common.h: aug_tile_pass) and displacement.  A block: a tile of 64 columns x 32 rows of one elastic
// sample, field 0 (displaces x) kept in registers, then field 1 (displaces y).  Out: the pixel each output pixel is displaced to,
// packed ey << 16 | ex, or AUG_OUTSIDE.
constexpr unsigned AUG_OUTSIDE = 0xFFFFFFFFu;    // no pixel packs to this: OH, OW <= 65535
__global__ __launch_bounds__(AUG_TILE_LANES) void elastic_cols_kernel(AugExtraParams p) {
  __shared__ float tile[AUG_TILE_FLOATS];
  const int x0 = blockIdx.x * AUG_TILE_X, y0 = blockIdx.y * AUG_TILE_A, b = blockIdx.z;
  const AugExtraDesc& e = p.extras[b];
  if (!(e.flags & AUG_ELASTIC)) return;              // the same in every lane of the block
  const long long plane = (long long)p.OH * p.OW;
  float dx[AUG_TILE_A / 4];
  for (int c = 0; c < 2; ++c)
    aug_tile_pass(tile, p.rows + ((long long)b * 2 + c) * plane, x0, y0, p.OW, p.OH, p.OW, p.taps, p.K, [&](int q, int oy, int ox, float acc) {
      if (c == 0) dx[q] = acc * e.a2;
      else {
        const float fy = rintf((float)oy + acc * e.a2), fx = rintf((float)ox + dx[q]);
        const bool inside = fy >= 0.f && fy <= (float)(p.OH - 1) && fx >= 0.f && fx <= (float)(p.OW - 1);
        p.map[(long long)b * plane + (long long)oy * p.OW + ox] = inside ? ((unsigned)(int)fy << 16 | (unsigned)(int)fx) : AUG_OUTSIDE;
      }
    });
}

// The gather: aug_gather_pixel behind a prologue.  An elastic sample's lane reads the pixel it is displaced to and evaluates the chain
// there; a pixel displaced out of the output is outside like the rotation's padding.  The image goes out as bytes (the table is not
// known yet); a jitter sample's bytes are counted per block in LDS and merged with integer atomics.  One lane per output pixel as
// above, but a block walks AUG_GATHER_ROWS rows: every block adds up to 256 counts to its sample's 256 words, and with a row a
// block those atomics on 2 048 addresses (batch of 8), not the gather, set the kernel's time.
constexpr int AUG_GATHER_ROWS = 8;
struct AugStoreBytes {           // the gather's sink: the byte to G and into the block's histogram
  unsigned char* G;
  unsigned* hist;                // the block's 256 bins in LDS, or null (a lambda testing `jitter` instead: 106 SGPRs, some spilled)
  __device__ __forceinline__ void operator()(long long at, unsigned char v) const {
    G[at] = v;
    if (hist) atomicAdd(&hist[v], 1u);
  }
};
__global__ __launch_bounds__(256) void augment_gather_kernel(AugExtraParams p) {
  __shared__ unsigned hist[256];
  const int ox = blockIdx.x * 256 + threadIdx.x, b = blockIdx.z;
  const AugDesc d = p.descs[b];
  const AugExtraDesc& e = p.extras[b];
  const bool elastic = p.use & e.flags & AUG_ELASTIC, jitter = p.use & e.flags & AUG_JITTER;
  if (jitter) aug_hist_zero(hist, threadIdx.x);
  const int row0 = blockIdx.y * AUG_GATHER_ROWS, row1 = min(row0 + AUG_GATHER_ROWS, p.OH);
  for (int oy = row0; oy < row1 && ox < p.OW; ++oy) {
    const long long plane = (long long)p.OH * p.OW, o = (long long)oy * p.OW + ox;
    int py = oy, px = ox;
    bool inside = true;
    if (elastic) {
      const unsigned m = p.map[(long long)b * plane + o];
      inside = m != AUG_OUTSIDE;
      py = inside ? (int)(m >> 16) : 0; px = inside ? (int)(m & 0xFFFFu) : 0;
    }
    aug_gather_pixel(d, p, b, py, px, inside, o, AugStoreBytes{p.G, jitter ? hist : nullptr});
  }
  if (jitter) aug_hist_flush(hist, threadIdx.x, p.hist + (long long)b * 256);
}

// T[b][v] of a jitter sample: one block per sample, one lane per byte value: the exact mean (augment_common.h: aug_contrast_mean)
// from lane 0 to every lane, then the jitter of L[v].
__global__ __launch_bounds__(256) void jitter_table_kernel(AugExtraParams p) {
  __shared__ double term[256];
  __shared__ float mean;
  const int b = blockIdx.x, v = threadIdx.x;
  const AugExtraDesc& e = p.extras[b];
  if (!(e.flags & AUG_JITTER)) return;
  const float br = e.brightness, co = e.contrast;
  const bool contrast_first = e.contrast_first != 0;
  const float L = p.lut32[v];
  const float m = aug_contrast_mean(p.hist + (long long)b * 256, v, L, br, contrast_first, (long long)p.ch * p.OH * p.OW, term);
  if (v == 0) mean = m;
  __syncthreads();
  p.T[(long long)b * 256 + v] = aug_jitter(L, br, co, contrast_first, mean);
}

// X from the gathered bytes through the sample's table (in LDS): as it is, blurred 5 x 5 with reflecting borders, or with Gaussian
// noise (Box-Muller on two Philox words; the library's logf / cosf, whose last-ulp differences from a correctly rounded pair are the
// one place the output may leave the definition, by one fp16 step).  One lane per output pixel, every channel.
__global__ __launch_bounds__(256) void augment_finish_kernel(AugExtraParams p) {
  __shared__ float T[256];
  const int ox = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y, b = blockIdx.z;
  const AugExtraDesc& e = p.extras[b];
  const bool jitter = p.use & e.flags & AUG_JITTER;
  T[threadIdx.x] = jitter ? p.T[(long long)b * 256 + threadIdx.x] : p.lut32[threadIdx.x];
  __syncthreads();
  if (ox >= p.OW) return;
  const int kind = (e.kind == 1 && (p.use & AUG_BLUR)) ? 1 : (e.kind == 2 && (p.use & AUG_NOISE)) ? 2 : 0;
  const long long plane = (long long)p.OH * p.OW, o = (long long)oy * p.OW + ox;
  long long rows[5];
  int cols[5];
  if (kind == 1) {
#pragma unroll
    for (int i = 0; i < 5; ++i) { rows[i] = (long long)aug_reflect(oy + i - 2, p.OH) * p.OW; cols[i] = aug_reflect(ox + i - 2, p.OW); }
  }
  for (int c = 0; c < p.ch; ++c) {
    const unsigned char* G = p.G + ((long long)b * p.ch + c) * plane;
    float v;
    if (kind == 1) {
      v = 0.f;
#pragma unroll
      for (int i = 0; i < 5; ++i)
#pragma unroll
        for (int j = 0; j < 5; ++j) v += e.w2[i * 5 + j] * T[G[rows[i] + cols[j]]];
    } else {
      v = T[G[o]];
      if (kind == 2) {
        unsigned w0, w1;
        philox4x32_10((unsigned)ox, (unsigned)oy, (unsigned)c, 1u, e.nkey[0], e.nkey[1], w0, w1);
        v = aug_clamp01(v + e.sigma_n * aug_gauss(w0, w1));
      }
    }
    p.X[((long long)b * p.ch + c) * plane + o] = (f16)v;
  }
}

}  // namespace

extern "C" {

int iunet_augment_desc_bytes(void) { return (int)sizeof(AugDesc); }

int iunet_augment_batch(const void* descs, int B, int ch, int C, int OH, int OW, const void* lut_f16, void* X, void* y, void* w,
                        void* stream) {
  IUNET_REQUIRE(descs && lut_f16 && X && y && w, "augment_batch: null pointer");
  IUNET_REQUIRE(B >= 1 && B <= 65535 && ch >= 1 && ch <= 4 && C >= 1 && C <= 16 && OH >= 1 && OH <= 65535 && OW >= 1,
                "augment_batch: B %d, channels %d, classes %d, output %d x %d", B, ch, C, OH, OW);
  AugParams p;
  p.descs = (const AugDesc*)descs; p.B = B; p.ch = ch; p.C = C; p.OH = OH; p.OW = OW;
  p.lut = (const f16*)lut_f16; p.X = (f16*)X; p.y = (f16*)y; p.w = (f16*)w;
  hipLaunchKernelGGL(augment_batch_kernel, dim3((OW + 255) / 256, OH, B), dim3(256), 0, (hipStream_t)stream, p);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

long long iunet_augment_extra_desc_bytes(void) { return (long long)sizeof(AugExtraDesc); }

long long iunet_augment_extra_ws_bytes(int B, int ch, int OH, int OW) {
  if (!(B >= 1 && B <= 65535 && ch >= 1 && ch <= 4 && OH >= 1 && OH <= 65535 && OW >= 1 && OW <= 65535)) {
    iunet_set_error("augment_extra_ws_bytes: B %d, channels %d, output %d x %d", B, ch, OH, OW);
    return IUNET_ERR_ARG;
  }
  return aug_workspace(B, ch, OH, OW).total;
}

int iunet_augment_batch_extra(const void* descs, const void* extras, int use, int B, int ch, int C, int OH, int OW,
                              const void* lut_f16, const void* lut_f32, const void* taps_f32, int K,
                              void* ws, long long ws_bytes, void* X, void* y, void* w, void* stream) {
  IUNET_REQUIRE(descs && extras && lut_f16 && lut_f32 && ws && X && y && w, "augment_batch_extra: null pointer");
  IUNET_REQUIRE(B >= 1 && B <= 65535 && ch >= 1 && ch <= 4 && C >= 1 && C <= 16 && OH >= 1 && OH <= 65535 && OW >= 1 && OW <= 65535,
                "augment_batch_extra: B %d, channels %d, classes %d, output %d x %d", B, ch, C, OH, OW);
  const AugWorkspace s = aug_workspace(B, ch, OH, OW);
  char shape[64];
  snprintf(shape, sizeof shape, "%d x %d output", OH, OW);
  const int rc = aug_check_extra("augment_batch_extra", shape, use, taps_f32, K, OH < OW ? OH : OW, ws_bytes, s.total, "iunet_augment_extra_ws_bytes", "side");
  if (rc != IUNET_OK) return rc;
  AugExtraParams p;
  p.descs = (const AugDesc*)descs; p.extras = (const AugExtraDesc*)extras;
  p.use = use; p.B = B; p.ch = ch; p.C = C; p.OH = OH; p.OW = OW; p.K = (use & AUG_ELASTIC) ? K : 1;
  p.lut = (const f16*)lut_f16; p.lut32 = (const float*)lut_f32; p.taps = (const float*)taps_f32;
  char* base = (char*)ws;
  p.rows = (float*)(base + s.rows); p.map = (unsigned*)(base + s.map); p.G = (unsigned char*)(base + s.G); p.hist = (unsigned*)(base + s.hist); p.T = (float*)(base + s.T);
  p.X = (f16*)X; p.y = (f16*)y; p.w = (f16*)w;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((OW + 255) / 256, OH, B), block(256);
  if (use & AUG_ELASTIC) {
    hipLaunchKernelGGL(elastic_rows_kernel, grid, block, 0, st, p);
    hipLaunchKernelGGL(elastic_cols_kernel, dim3((OW + AUG_TILE_X - 1) / AUG_TILE_X, (OH + AUG_TILE_A - 1) / AUG_TILE_A, B), block, 0, st, p);
  }
  if (use & AUG_JITTER) IUNET_CHECK_HIP(hipMemsetAsync(p.hist, 0, 1024 * (size_t)B, st));
  hipLaunchKernelGGL(augment_gather_kernel, dim3(grid.x, (OH + AUG_GATHER_ROWS - 1) / AUG_GATHER_ROWS, B), block, 0, st, p);
  if (use & AUG_JITTER) hipLaunchKernelGGL(jitter_table_kernel, dim3(B), block, 0, st, p);
  hipLaunchKernelGGL(augment_finish_kernel, grid, block, 0, st, p);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

}  // extern "C"
