// Symmetry ensemble of the 3-D net (defined bit for bit by tests/tta_ref.py): the 48 symmetries of the cube applied
// to a uint8 block on the way into the forward, and undone on the fp32 probabilities on the way into the ensemble's running sum / min / max.
//
// A symmetry is sym = 8 pi + f: pi indexes the permutations of (0, 1, 2) in lexicographic order, bit a of f flips OUTPUT axis a.  With
// X the untransformed array [D][H][W] and Y the transformed one [m0][m1][m2], m[a] = n[perm[a]], voxel s of X is voxel t of Y with
// t[a] = flip_a ? m[a] - 1 - s[perm[a]] : s[perm[a]].  On the host that becomes one affine map: Y offset = base + s . sy with signed strides
// sy[perm[a]] = +-(stride of Y's axis a) -- the kernels know nothing else of the symmetry.  iunet_sym_block copies X -> Y (1-byte items),
// iunet_sym_accumulate reads Y (q, items of C floats that stay together) and updates sum / mn / mx in X's order, which is contiguous.
//
// perm[2] == 2 (pi 0 and 2): W is innermost on both sides, a row of X is a row of Y, reversed where bit 2 of f is set.  No LDS:
//   bytes   one lane per 16 bytes where W and both addresses are multiples of 16 (a reversed row: the mirrored 16 bytes, byte-swapped in
//           registers), else one lane per byte;
//   floats  one lane per voxel; the C floats of a voxel are one 4 / 8 / 16-byte access where C is 1, 2 or 4 and the buffers are aligned
//           to it, C scalar accesses otherwise.
// the four other permutations: Y's innermost axis runs along X's axis b = perm[2] (0 or 1).  A workgroup stages a tile of (b, W) through
//   LDS: global loads are runs along the source's innermost axis, global stores / updates runs along the destination's.
//   bytes   64 x 64 tile, rows of 68 bytes: lane l reads byte l * 68 + i of the transposed pass, dword l * 17 + i / 4 -- 32 banks per half wave;
//   floats  64 (W) x TB (b) voxels, TB = 32 / 16 / 8 for C <= 2 / <= 4 / <= 16 (16 to 33 KiB), rows of TB * C + 1 floats: the pass over q
//           writes consecutive floats, the pass over X reads float lane * (TB * C + 1) + const -- an odd stride, 32 banks per half wave.
//   Tile edges are ragged (min against the extent); the third axis r is the slowest grid index.
// Every output element is owned by one thread, there are no atomics and no sums across threads: a repeated launch gives the same bits.
// mean = sum * inv_count is ONE fp32 multiply (inv_count comes from the host); spread = max over c of (mx - mn), fp32.
// All flat indices are 64-bit.  Launches are one-dimensional grids of 256 threads, at most 2^24 - 1 workgroups (fewer than 2^32 threads).
#include "common.h"
#include <cstdint>

namespace {

constexpr int SYM_THREADS = 256;
constexpr long long SYM_MAX_BLOCKS = (1ll << 24) - 1;
constexpr int SYM_TILE = 64;                 // edge of the byte tile, and the W extent of the float tile
constexpr int SYM_LD = SYM_TILE + 4;         // bytes of one staged row of the byte tile

const int SYM_PERMS[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

// the rows' view: Y offset of X voxel (z, y, x) = base + z sy0 + y sy1 + x sy2 (sy2 = +-1 where this is used)
struct SymRows {
  int H, W;
  long long sy0, sy1, sy2, base;
};

// the tiles' view: tile axes b (X stride xb, Y stride yb = +-1) and W (X stride 1, Y stride yw), slow axis r
struct SymTiles {
  int nb, nw, tb, tw, TB;                    // extents of b and W, tiles along each, tile extent along b
  long long xb, xr, yb, yr, yw, base;
};

struct SymMap {
  SymRows rows;
  SymTiles tiles;
  bool transposing;
  long long vox, blocks;                     // voxels; workgroups of the launch
};

// TB: tile extent along b (64 for the byte kernel)
void sym_map(SymMap& m, int D, int H, int W, int sym, int TB) {
  const int* perm = SYM_PERMS[sym >> 3];
  const int f = sym & 7, n[3] = {D, H, W};
  const long long mm[3] = {n[perm[0]], n[perm[1]], n[perm[2]]}, ys[3] = {mm[1] * mm[2], mm[2], 1}, xs[3] = {(long long)H * W, W, 1};
  long long sy[3], base = 0;
  for (int a = 0; a < 3; ++a) {
    const bool flip = (f >> a) & 1;
    sy[perm[a]] = flip ? -ys[a] : ys[a];
    if (flip) base += (mm[a] - 1) * ys[a];
  }
  m.vox = (long long)D * H * W;
  m.transposing = perm[2] != 2;
  m.rows = SymRows{H, W, sy[0], sy[1], sy[2], base};
  if (!m.transposing) {
    m.blocks = (m.vox + SYM_THREADS - 1) / SYM_THREADS;
    return;
  }
  const int b = perm[2], r = 1 - b;
  SymTiles& t = m.tiles;
  t.nb = n[b]; t.nw = W; t.TB = TB; t.tb = (n[b] + TB - 1) / TB; t.tw = (W + SYM_TILE - 1) / SYM_TILE;
  t.xb = xs[b]; t.xr = xs[r]; t.yb = sy[b]; t.yr = sy[r]; t.yw = sy[2]; t.base = base;
  m.blocks = (long long)t.tb * t.tw * n[r];
}

__device__ __forceinline__ unsigned int sym_bswap(unsigned int v) { return __builtin_bswap32(v); }

// ---- bytes
template <bool WIDE>
__global__ __launch_bounds__(SYM_THREADS) void sym_rows_u8_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out,
                                                                   SymRows m, long long total) {
  const long long idx = (long long)blockIdx.x * SYM_THREADS + threadIdx.x;
  if (idx >= total) return;
  const int per = WIDE ? m.W >> 4 : m.W;                       // items of one row
  const long long row = idx / per;
  const int cx = (int)(idx - row * per);
  const long long z = row / m.H;
  const int y = (int)(row - z * m.H);
  const long long yrow = m.base + z * m.sy0 + y * m.sy1;
  if (WIDE) {
    const int x = cx * 16;
    const uint4 v = *(const uint4*)(in + row * m.W + x);
    if (m.sy2 > 0) {
      *(uint4*)(out + yrow + x) = v;
    } else {                                                   // bytes x .. x + 15 land on yrow - x - 15 .. yrow - x, in reverse
      uint4 w;
      w.x = sym_bswap(v.w); w.y = sym_bswap(v.z); w.z = sym_bswap(v.y); w.w = sym_bswap(v.x);
      *(uint4*)(out + yrow - x - 15) = w;
    }
  } else {
    out[yrow + cx * m.sy2] = in[idx];
  }
}

__global__ __launch_bounds__(SYM_THREADS) void sym_tiles_u8_kernel(const unsigned char* __restrict__ in, unsigned char* __restrict__ out,
                                                                    SymTiles t) {
  __shared__ unsigned char tile[SYM_TILE * SYM_LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned int blk = blockIdx.x;
  const int iw = (int)(blk % (unsigned)t.tw);
  blk /= (unsigned)t.tw;
  const int ib = (int)(blk % (unsigned)t.tb), r = (int)(blk / (unsigned)t.tb);
  const int w0 = iw * SYM_TILE, b0 = ib * SYM_TILE;
  const int nw = min(SYM_TILE, t.nw - w0), nb = min(SYM_TILE, t.nb - b0);
  const unsigned char* src = in + ((long long)r * t.xr + (long long)b0 * t.xb + w0);
#pragma unroll 4
  for (int j = wave; j < nb; j += 4)
    if (lane < nw) tile[j * SYM_LD + lane] = src[(long long)j * t.xb + lane];
  __syncthreads();
  unsigned char* dst = out + (t.base + (long long)r * t.yr + (long long)b0 * t.yb + (long long)w0 * t.yw);
#pragma unroll 4
  for (int i = wave; i < nw; i += 4)
    if (lane < nb) dst[(long long)lane * t.yb + (long long)i * t.yw] = tile[lane * SYM_LD + i];
}

// ---- floats
struct AccParams {
  const float* q;
  float *sum, *mn, *mx, *mean, *spread;      // (mean may be sum: no __restrict__ here)
  int C, first, last;
  float inv;
};

template <int N> struct alignas(4 * N) FV { float v[N]; };

// One voxel of the ensemble: its member values src(0 .. C - 1) into sum / mn / mx at voxel `vox` of X; mean and spread on the last call.
// CV = C in {1, 2, 4}: the voxel's floats are one access per array; CV = 0: C scalar accesses.
template <int CV, typename Src>
__device__ __forceinline__ void acc_voxel(const AccParams& p, long long vox, Src src) {
#pragma clang fp contract(off)
  if constexpr (CV > 0) {
    FV<CV> v, s, lo, hi;
#pragma unroll
    for (int c = 0; c < CV; ++c) v.v[c] = src(c);
    s = v; lo = v; hi = v;
    if (!p.first) {
      const FV<CV> ts = ((const FV<CV>*)p.sum)[vox];
      FV<CV> tl = v, th = v;
      if (p.mn) { tl = ((const FV<CV>*)p.mn)[vox]; th = ((const FV<CV>*)p.mx)[vox]; }
#pragma unroll
      for (int c = 0; c < CV; ++c) { s.v[c] = ts.v[c] + v.v[c]; lo.v[c] = fminf(tl.v[c], v.v[c]); hi.v[c] = fmaxf(th.v[c], v.v[c]); }
    }
    ((FV<CV>*)p.sum)[vox] = s;
    if (p.mn) { ((FV<CV>*)p.mn)[vox] = lo; ((FV<CV>*)p.mx)[vox] = hi; }
    if (p.last) {
      FV<CV> m;
#pragma unroll
      for (int c = 0; c < CV; ++c) m.v[c] = s.v[c] * p.inv;
      ((FV<CV>*)p.mean)[vox] = m;                              // after the store of sum: where mean is sum, the mean stays
      if (p.spread) {
        float sp = hi.v[0] - lo.v[0];
#pragma unroll
        for (int c = 1; c < CV; ++c) sp = fmaxf(sp, hi.v[c] - lo.v[c]);
        p.spread[vox] = sp;
      }
    }
  } else {
    const long long e0 = vox * p.C;
    float sp = 0.f;
    for (int c = 0; c < p.C; ++c) {
      const float v = src(c);
      float s = v, lo = v, hi = v;
      if (!p.first) {
        s = p.sum[e0 + c] + v;
        if (p.mn) { lo = fminf(p.mn[e0 + c], v); hi = fmaxf(p.mx[e0 + c], v); }
      }
      p.sum[e0 + c] = s;
      if (p.mn) { p.mn[e0 + c] = lo; p.mx[e0 + c] = hi; }
      if (p.last) p.mean[e0 + c] = s * p.inv;
      const float d = hi - lo;
      sp = c == 0 ? d : fmaxf(sp, d);
    }
    if (p.last && p.spread) p.spread[vox] = sp;
  }
}

template <int CV>
__global__ __launch_bounds__(SYM_THREADS) void sym_acc_rows_kernel(AccParams p, SymRows m, long long total) {
  const long long idx = (long long)blockIdx.x * SYM_THREADS + threadIdx.x;
  if (idx >= total) return;
  const long long row = idx / m.W;
  const int x = (int)(idx - row * m.W);
  const long long z = row / m.H;
  const int y = (int)(row - z * m.H);
  const long long yv = m.base + z * m.sy0 + y * m.sy1 + x * m.sy2;
  if constexpr (CV > 0) {
    const FV<CV> v = ((const FV<CV>*)p.q)[yv];
    acc_voxel<CV>(p, idx, [&](int c) { return v.v[c]; });
  } else {
    const float* s = p.q + yv * p.C;
    acc_voxel<0>(p, idx, [&](int c) { return s[c]; });
  }
}

template <int CV>
__global__ __launch_bounds__(SYM_THREADS) void sym_acc_tiles_kernel(AccParams p, SymTiles t) {
  extern __shared__ float acc_tile[];                          // [SYM_TILE][TB * C + 1]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C = CV > 0 ? CV : p.C, RS = t.TB * C + 1;
  unsigned int blk = blockIdx.x;
  const int iw = (int)(blk % (unsigned)t.tw);
  blk /= (unsigned)t.tw;
  const int ib = (int)(blk % (unsigned)t.tb), r = (int)(blk / (unsigned)t.tb);
  const int w0 = iw * SYM_TILE, b0 = ib * t.TB;
  const int nw = min(SYM_TILE, t.nw - w0), nb = min(t.TB, t.nb - b0);
  // the pass over q: row i of the tile (one W position) is the run of nb * C floats that starts at the voxel of the lowest address
  const long long y0 = t.base + (long long)r * t.yr + (long long)w0 * t.yw + (t.yb > 0 ? (long long)b0 : -(long long)(b0 + nb - 1));
  for (int g = lane; g < nb * C; g += 64) {
    const int jv = g / C, c = g - jv * C;
    const int slot = (t.yb > 0 ? jv : nb - 1 - jv) * C + c;
#pragma unroll 4
    for (int i = wave; i < nw; i += 4) acc_tile[i * RS + slot] = p.q[(y0 + (long long)i * t.yw) * C + g];
  }
  __syncthreads();
  // the pass over X: lane = W position, a wave per b position
  const long long x0 = (long long)r * t.xr + (long long)b0 * t.xb + w0;
  for (int j = wave; j < nb; j += 4)
    if (lane < nw) acc_voxel<CV>(p, x0 + (long long)j * t.xb + lane, [&](int c) { return acc_tile[lane * RS + j * C + c]; });
}

template <int CV>
void sym_acc_launch(const AccParams& p, const SymMap& m, hipStream_t stream) {
  if (m.transposing) {
    const int lds = SYM_TILE * (m.tiles.TB * p.C + 1) * (int)sizeof(float);
    hipLaunchKernelGGL(sym_acc_tiles_kernel<CV>, dim3((unsigned)m.blocks), dim3(SYM_THREADS), lds, stream, p, m.tiles);
  } else {
    hipLaunchKernelGGL(sym_acc_rows_kernel<CV>, dim3((unsigned)m.blocks), dim3(SYM_THREADS), 0, stream, p, m.rows, m.vox);
  }
}

inline bool sym_volume_ok(int D, int H, int W) {
  return D > 0 && H > 0 && W > 0 && (long long)D * H < (1ll << 42) && (long long)D * H <= ((1ll << 42) - 1) / W;
}

inline bool sym_aligned(const void* p, int bytes) { return ((uintptr_t)p & (uintptr_t)(bytes - 1)) == 0; }

}  // namespace

extern "C" {

// in: uint8 [D][H][W]; out: uint8 [m0][m1][m2], m[a] = (D, H, W)[perm[a]]; both on the device, not overlapping.
int iunet_sym_block(const void* in, int D, int H, int W, int sym, void* out, void* stream) {
  IUNET_REQUIRE(in && out, "sym_block: null pointer");
  IUNET_REQUIRE(sym_volume_ok(D, H, W), "sym_block: volume %d x %d x %d", D, H, W);
  IUNET_REQUIRE(sym >= 0 && sym < 48, "sym_block: symmetry code %d outside 0..47", sym);
  SymMap m;
  sym_map(m, D, H, W, sym, SYM_TILE);
  IUNET_REQUIRE(m.blocks <= SYM_MAX_BLOCKS, "sym_block: block %d x %d x %d under symmetry %d exceeds the grid (%lld workgroups, %lld allowed)",
                D, H, W, sym, m.blocks, SYM_MAX_BLOCKS);
  const unsigned char* src = (const unsigned char*)in;
  unsigned char* dst = (unsigned char*)out;
  if (m.transposing) {
    hipLaunchKernelGGL(sym_tiles_u8_kernel, dim3((unsigned)m.blocks), dim3(SYM_THREADS), 0, (hipStream_t)stream, src, dst, m.tiles);
  } else if (W % 16 == 0 && sym_aligned(in, 16) && sym_aligned(out, 16)) {
    const long long chunks = m.vox / 16;
    hipLaunchKernelGGL(sym_rows_u8_kernel<true>, dim3((unsigned)((chunks + SYM_THREADS - 1) / SYM_THREADS)), dim3(SYM_THREADS), 0,
                       (hipStream_t)stream, src, dst, m.rows, chunks);
  } else {
    hipLaunchKernelGGL(sym_rows_u8_kernel<false>, dim3((unsigned)m.blocks), dim3(SYM_THREADS), 0, (hipStream_t)stream, src, dst, m.rows, m.vox);
  }
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

// q: fp32 [m0][m1][m2][C]; sum, mn, mx, mean: fp32 [D][H][W][C]; spread: fp32 [D][H][W]; all on the device.
int iunet_sym_accumulate(const void* q, int D, int H, int W, int C, int sym, int index, int count, float inv_count, void* sum, void* mn,
                         void* mx, void* mean, void* spread, void* stream) {
  const bool last = index == count - 1;
  IUNET_REQUIRE(q && sum && (mean || !last), "sym_accumulate: null pointer (q, sum, and mean on the last call)");
  IUNET_REQUIRE((mn && mx && spread) || (!mn && !mx && !spread), "sym_accumulate: mn, mx and spread go together, all or none");
  IUNET_REQUIRE(sym_volume_ok(D, H, W), "sym_accumulate: volume %d x %d x %d", D, H, W);
  IUNET_REQUIRE(C >= 1 && C <= 16, "sym_accumulate: %d classes outside 1..16", C);
  IUNET_REQUIRE(sym >= 0 && sym < 48, "sym_accumulate: symmetry code %d outside 0..47", sym);
  IUNET_REQUIRE(count >= 1 && count <= 48, "sym_accumulate: member count %d outside 1..48", count);
  IUNET_REQUIRE(index >= 0 && index < count, "sym_accumulate: member index %d outside [0, %d)", index, count);
  SymMap m;
  sym_map(m, D, H, W, sym, C <= 2 ? 32 : C <= 4 ? 16 : 8);
  IUNET_REQUIRE(m.blocks <= SYM_MAX_BLOCKS, "sym_accumulate: block %d x %d x %d under symmetry %d exceeds the grid (%lld workgroups, %lld allowed)",
                D, H, W, sym, m.blocks, SYM_MAX_BLOCKS);
  AccParams p;
  p.q = (const float*)q; p.sum = (float*)sum; p.mn = (float*)mn; p.mx = (float*)mx; p.mean = (float*)mean; p.spread = (float*)spread;
  p.C = C; p.first = index == 0; p.last = last; p.inv = inv_count;
  const int vb = 4 * C;
  const bool vec = (C == 1 || C == 2 || C == 4) && sym_aligned(q, vb) && sym_aligned(sum, vb) && sym_aligned(mn, vb) && sym_aligned(mx, vb) &&
                   sym_aligned(mean, vb);
  if (!vec) sym_acc_launch<0>(p, m, (hipStream_t)stream);
  else if (C == 1) sym_acc_launch<1>(p, m, (hipStream_t)stream);
  else if (C == 2) sym_acc_launch<2>(p, m, (hipStream_t)stream);
  else sym_acc_launch<4>(p, m, (hipStream_t)stream);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

}  // extern "C"
