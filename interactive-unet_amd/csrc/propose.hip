// Where to annotate next (defined bit for bit by tests/propose_ref.py): the uncertainty of a resident predicted
// volume, its brick sums, and the uncertainty summed over candidate planes.
//
// Uncertainty byte of a voxel with predicted bytes q[0 .. C-1]: b1 the largest, b2 the second largest with multiplicity,
// u = 255 - (b1 - b2) if b1 > 0 else 0; u = 0 where a weight byte is > 0 (annotated) or image channel 0 is 0 (the loader's dark rule).
// Integer arithmetic only.
//
// uncertainty_kernel: one workgroup owns the bricks (bz, by, a run of xs voxels along x), xs a power of two in 16 .. 256 and a multiple
// of the brick, so a brick's sum is finished on chip: no atomics, no second launch.  It walks the brick row's g * g volume rows in
// batches of about 16 KiB.  A batch's row segments (xs * C contiguous bytes of pred, xs * wch of weight, xs * ich of image) are staged
// in LDS by 16-byte loads on the 16-byte grid of the global address, at the LDS offset with the address's low four bits, so the LDS
// stores are aligned too.  A row of the [Z][Y][X][C] volume starts at any byte: where the rows are not whole 16-byte slots, the slots
// that straddle a segment's ends are copied bytewise (the scalar head and tail).  Then thread t takes voxel t % xs of row t / xs
// (+ 256 / xs per step): the same x in every step, so its sum belongs to one brick; 64 consecutive lanes write 64 consecutive bytes of u.
// The sums meet in LDS at the end.  The pass lives on the bytes it keeps in flight: a thread issues four loads before it stores them,
// reads four rows' bytes from LDS before it uses them, and the host sizes xs so that the grid fills the chip.
//
// plane_scores_kernel: sample (i, j) of plane p at c = (a r_i + b r_j) + o per axis (plane_point, volume_rules.h); inside iff
// 0 <= c <= dim - 1 on all axes (coord_inside), then it reads voxel floor(c + 0.5) (coord_nearest) -- the order-0 sample of
// slab_gather_kernel (slab.hip) at r_k = 0, with its lane mapping: 64 consecutive j per wave, a wave per row, four steps of four rows per workgroup.  (sum u, count inside) is
// reduced in the wave, then across the four waves, and written as one int pair per workgroup; plane_scores_finish_kernel sums a
// plane's pairs into int64.  Integer sums: any order gives the same bits.
#include "common.h"
#include "volume_rules.h"
#include <cstdint>

namespace {

constexpr int UNC_THREADS = 256;
constexpr int UNC_LDS = 16384;         // bytes of one staged batch (a batch of fewer rows than the threads take in one step is rounded up)
constexpr int UNC_STAGE = 4;           // 16-byte slots a thread loads before it stores them
constexpr int UNC_ROWS = 4;            // rows a thread computes per step
constexpr int UNC_BLOCKS = 2048;       // workgroups wanted in flight: 8 on each of 256 CUs

struct UncParams {
  const unsigned char *pred, *weight, *image;
  unsigned char* u;
  unsigned int* bricks;
  int Z, Y, X, C, wch, ich, g, g_log2;
  int xs, xs_log2, runs, Yb, Xb;
  int rb;                              // rows of one staged batch, a multiple of the 256 / xs rows the threads take in one step
  int ls_p, ls_w, ls_i;                // LDS bytes of one staged row: align16(xs * bytes per voxel) + 16
  unsigned int magic_p, magic_w, magic_i;   // ceil(2^32 / (ls / 16)): q / (ls / 16) = umulhi(q, magic) for the q < 2^12 of a batch
};

__host__ __device__ inline int unc_row_lds(int xs, int cb) { return ((xs * cb + 15) & ~15) + 16; }

// Row rr of the workgroup's brick row is (z0 + rr / g, y0 + rr % g): the g x g grid of a whole brick, rows past the volume's y extent
// skipped (rows past its z extent lie behind the loop bounds).  The row's first voxel:
__device__ __forceinline__ long long unc_row_voxel(const UncParams& p, int z0, int y0, int x0, int rr) {
  return ((long long)(z0 + (rr >> p.g_log2)) * p.Y + (y0 + (rr & (p.g - 1)))) * p.X + x0;
}

// rows rr0 .. of the batch: bytes [row voxel * cb, + nx * cb) of src -> lds[r * ls + (address & 15) + byte].  Slot s of a row is the
// 16 bytes at segment offset 16 s - (address & 15): aligned in memory and in LDS.
//   aligned (the volume starts on a 16-byte address and both the volume's and the segment's row bytes are multiples of 16): every slot is
//   whole or empty.  A thread loads UNC_STAGE slots, then stores them: the loads are in flight together (a slot outside the batch loads
//   the volume's first 16 bytes and stores them in a dump slot behind the batches: one basic block).
//   otherwise: slot by slot; the slots that straddle a segment's ends are copied bytewise (the scalar head and tail).
__device__ __forceinline__ void unc_stage(const UncParams& p, const unsigned char* __restrict__ src, int cb, int ls, unsigned int magic,
                                          unsigned char* lds, unsigned char* dump, int z0, int y0, int x0, int nx, int rr0, int nrows) {
  const unsigned int spr = (unsigned int)ls >> 4, total = (unsigned int)p.rb * spr;
  const int len = nx * cb;
  if ((((uintptr_t)src | (uintptr_t)((long long)p.X * cb) | (uintptr_t)len) & 15) == 0) {
#pragma unroll 1
    for (unsigned int q0 = threadIdx.x; q0 < total; q0 += UNC_STAGE * UNC_THREADS) {
      uint4 val[UNC_STAGE];
      unsigned char* to[UNC_STAGE];
#pragma unroll
      for (int k = 0; k < UNC_STAGE; ++k) {
        const unsigned int q = q0 + k * UNC_THREADS;
        const int r = (int)__umulhi(q, magic), s = (int)(q - (unsigned int)r * spr), rr = rr0 + r;
        const bool ok = q < total && rr < nrows && y0 + (rr & (p.g - 1)) < p.Y && 16 * s < len;
        to[k] = ok ? lds + r * ls + 16 * s : dump;
        val[k] = *(const uint4*)(src + (ok ? unc_row_voxel(p, z0, y0, x0, rr) * cb + 16 * s : 0));
      }
#pragma unroll
      for (int k = 0; k < UNC_STAGE; ++k) *(uint4*)to[k] = val[k];
    }
    return;
  }
#pragma unroll 1
  for (unsigned int q = threadIdx.x; q < total; q += UNC_THREADS) {
    const int r = (int)__umulhi(q, magic), s = (int)(q - (unsigned int)r * spr), rr = rr0 + r;
    if (rr >= nrows) break;
    if (y0 + (rr & (p.g - 1)) >= p.Y) continue;
    const unsigned char* row = src + unc_row_voxel(p, z0, y0, x0, rr) * cb;
    const int pad = (int)((uintptr_t)row & 15);
    const int lo = max(16 * s - pad, 0), hi = min(16 * s - pad + 16, len);
    unsigned char* dst = lds + r * ls + pad + lo;
    if (hi - lo == 16) {
      *(uint4*)dst = *(const uint4*)(row + lo);
    } else {
      for (int b = lo; b < hi; ++b) dst[b - lo] = row[b];
    }
  }
}

// C2: two classes; W, I: a weight / an image volume is given (compile-time, so the four rows a thread takes per unrolled step form one
// basic block and their LDS reads are in flight together)
template <bool C2, bool W, bool I>
__global__ __launch_bounds__(UNC_THREADS) void uncertainty_kernel(UncParams p) {
  extern __shared__ __align__(16) unsigned char unc_lds[];
  __shared__ unsigned int red[UNC_THREADS];
  const int tid = threadIdx.x;
  unsigned int blk = blockIdx.x;
  const int run = (int)(blk % (unsigned)p.runs);
  blk /= (unsigned)p.runs;
  const int by = (int)(blk % (unsigned)p.Yb), bz = (int)(blk / (unsigned)p.Yb);
  const int z0 = bz * p.g, y0 = by * p.g, x0 = run * p.xs;
  const int nx = min(p.xs, p.X - x0), nrows = min(p.g, p.Z - z0) << p.g_log2, rstep = UNC_THREADS >> p.xs_log2;
  unsigned char* lp = unc_lds;
  unsigned char* lw = lp + p.rb * p.ls_p;
  unsigned char* li = lw + p.rb * p.ls_w;
  unsigned char* dump = li + p.rb * p.ls_i;                             // 16 bytes nobody reads
  const int v = tid & (p.xs - 1), r0 = tid >> p.xs_log2;
  unsigned int acc = 0;
  for (int rr0 = 0; rr0 < nrows; rr0 += p.rb) {
    unc_stage(p, p.pred, p.C, p.ls_p, p.magic_p, lp, dump, z0, y0, x0, nx, rr0, nrows);
    if (W) unc_stage(p, p.weight, p.wch, p.ls_w, p.magic_w, lw, dump, z0, y0, x0, nx, rr0, nrows);
    if (I) unc_stage(p, p.image, p.ich, p.ls_i, p.magic_i, li, dump, z0, y0, x0, nx, rr0, nrows);
    __syncthreads();
    // UNC_ROWS rows per step, as one basic block whose LDS reads are in flight together: a row or voxel outside the volume (or behind
    // the batch: its reads go to the batch's last row) is computed like the others and only its result is dropped
#pragma unroll 1
    for (int rs = r0; rs < p.rb; rs += UNC_ROWS * rstep) {
      int uk[UNC_ROWS];
      long long at[UNC_ROWS];
#pragma unroll
      for (int k = 0; k < UNC_ROWS; ++k) {
        const int r = min(rs + k * rstep, p.rb - 1), rr = rr0 + r;
        const bool ok = rs + k * rstep < p.rb && v < nx && rr < nrows && y0 + (rr & (p.g - 1)) < p.Y;
        const long long vox = unc_row_voxel(p, z0, y0, x0, rr);
        const unsigned char* q = lp + r * p.ls_p + (int)(((uintptr_t)p.pred + (uintptr_t)(vox * p.C)) & 15) + v * p.C;
        const int q0 = q[0], q1 = q[1];
        int b1 = max(q0, q1), b2 = min(q0, q1);
        if (!C2) {
          for (int c = 2; c < p.C; ++c) {
            const int t = q[c];
            b2 = max(b2, min(b1, t));
            b1 = max(b1, t);
          }
        }
        int u = b1 > 0 ? 255 - (b1 - b2) : 0;
        if (W) {
          const unsigned char* w = lw + r * p.ls_w + (int)(((uintptr_t)p.weight + (uintptr_t)(vox * p.wch)) & 15) + v * p.wch;
          u = (w[0] | w[p.wch - 1]) ? 0 : u;
        }
        if (I) u = li[r * p.ls_i + (int)(((uintptr_t)p.image + (uintptr_t)(vox * p.ich)) & 15) + v * p.ich] ? u : 0;
        uk[k] = ok ? u : 0;
        at[k] = ok ? vox + v : -1;
        acc += (unsigned int)uk[k];
      }
      if (p.u) {
#pragma unroll
        for (int k = 0; k < UNC_ROWS; ++k)
          if (at[k] >= 0) p.u[at[k]] = (unsigned char)uk[k];
      }
    }
    __syncthreads();
  }
  if (!p.bricks) return;
  red[tid] = acc;
  __syncthreads();
  const int b = tid, bx = run * (p.xs >> p.g_log2) + b;
  if (b < (p.xs >> p.g_log2) && bx < p.Xb) {
    unsigned int s = 0;
    for (int k = 0; k < rstep; ++k)
      for (int i = 0; i < p.g; ++i) s += red[k * p.xs + b * p.g + i];
    p.bricks[((long long)bz * p.Yb + by) * p.Xb + bx] = s;
  }
}

template <bool C2, bool W>
void uncertainty_launch(const UncParams& p, unsigned int blocks, int lds, hipStream_t stream) {
  if (p.image) hipLaunchKernelGGL((uncertainty_kernel<C2, W, true>), dim3(blocks), dim3(UNC_THREADS), lds, stream, p);
  else hipLaunchKernelGGL((uncertainty_kernel<C2, W, false>), dim3(blocks), dim3(UNC_THREADS), lds, stream, p);
}

constexpr int SCORE_ROWS = 16;         // rows of a plane one workgroup takes: four steps of four waves

struct ScoreParams {
  const unsigned char* u;
  int dim[3];
  const double* geoms;
  int sw, start;
  int2* ws;
};

__host__ __device__ inline long long score_blocks(int sw) { return (long long)((sw + 63) / 64) * ((sw + SCORE_ROWS - 1) / SCORE_ROWS); }

__global__ __launch_bounds__(256) void plane_scores_kernel(ScoreParams p) {
  __shared__ int part[4][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + lane;
  const double* g = p.geoms + 9 * (long long)blockIdx.z;
  const double rj = (double)(p.start + j);
  const long long sy = p.dim[2], sz = (long long)p.dim[1] * p.dim[2];
  int sum = 0, cnt = 0;
  for (int r = 0; r < SCORE_ROWS / 4; ++r) {
    const int i = blockIdx.y * SCORE_ROWS + r * 4 + wave;
    if (i >= p.sw || j >= p.sw) continue;
    const double ri = (double)(p.start + i);
    double c[3];
    bool inside = true;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      c[x] = plane_point(g[x], g[3 + x], g[6 + x], ri, rj);
      inside = inside && coord_inside(c[x], p.dim[x]);
    }
    if (inside) {
      const long long z = (long long)coord_nearest(c[0]), y = (long long)coord_nearest(c[1]), x = (long long)coord_nearest(c[2]);
      sum += p.u[z * sz + y * sy + x];
      cnt += 1;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    sum += __shfl_down(sum, off, 64);
    cnt += __shfl_down(cnt, off, 64);
  }
  if (lane == 0) { part[wave][0] = sum; part[wave][1] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0)
    p.ws[((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] =
        make_int2(part[0][0] + part[1][0] + part[2][0] + part[3][0], part[0][1] + part[1][1] + part[2][1] + part[3][1]);
}

__global__ __launch_bounds__(64) void plane_scores_finish_kernel(const int2* ws, int nblk, long long* out) {
  const int2* row = ws + (long long)blockIdx.x * nblk;
  long long s = 0, c = 0;
  for (int k = threadIdx.x; k < nblk; k += 64) { const int2 t = row[k]; s += t.x; c += t.y; }
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_down(s, off, 64);
    c += __shfl_down(c, off, 64);
  }
  if (threadIdx.x == 0) { out[2 * (long long)blockIdx.x] = s; out[2 * (long long)blockIdx.x + 1] = c; }
}

}  // namespace

extern "C" {

// pred: uint8 [Z][Y][X][C]; weight: NULL or uint8 [Z][Y][X][wch]; image: NULL or uint8 [Z][Y][X][ich]; u: uint8 [Z][Y][X] or NULL;
// bricks: uint32 [ceil(Z / brick)][ceil(Y / brick)][ceil(X / brick)] or NULL; all on the device.
int iunet_uncertainty_volume(const void* pred, int Z, int Y, int X, int C, const void* weight, int wch, const void* image, int ich,
                             int brick, void* u, void* bricks, void* stream) {
  IUNET_REQUIRE(pred && (u || bricks), "uncertainty_volume: null pointer (pred, and one of u / bricks)");
  IUNET_REQUIRE(C >= 2 && C <= 16, "uncertainty_volume: %d classes outside 2..16", C);
  IUNET_REQUIRE(!weight || wch == 1 || wch == 2, "uncertainty_volume: %d weight channels (1 or 2)", wch);
  IUNET_REQUIRE(!image || (ich >= 1 && ich <= 4), "uncertainty_volume: %d image channels outside 1..4", ich);
  IUNET_REQUIRE(brick == 4 || brick == 8 || brick == 16 || brick == 32, "uncertainty_volume: brick size %d (4, 8, 16 or 32)", brick);
  IUNET_REQUIRE(volume_ok(Z, Y, X, VOLUME_MAX_SAMPLED), "uncertainty_volume: volume %d x %d x %d", Z, Y, X);
  UncParams p;
  p.pred = (const unsigned char*)pred; p.weight = (const unsigned char*)weight; p.image = (const unsigned char*)image;
  p.u = (unsigned char*)u; p.bricks = (unsigned int*)bricks;
  p.Z = Z; p.Y = Y; p.X = X; p.C = C; p.wch = weight ? wch : 0; p.ich = image ? ich : 0; p.g = brick;
  p.g_log2 = brick == 4 ? 2 : brick == 8 ? 3 : brick == 16 ? 4 : 5;
  // xs: the smallest power of two that holds the row, 16 .. 256 and at least a brick; halved down to 64 (and a brick) while the grid has
  // fewer than UNC_BLOCKS workgroups -- the pass lives on the bytes in flight, one batch per resident workgroup
  p.xs_log2 = 4;
  while ((1 << p.xs_log2) < brick || ((1 << p.xs_log2) < 256 && (1 << p.xs_log2) < X)) ++p.xs_log2;
  const long long brick_rows = (long long)((Z + brick - 1) / brick) * ((Y + brick - 1) / brick);
  while (p.xs_log2 > 6 && (1 << (p.xs_log2 - 1)) >= brick && brick_rows * ((X + (1 << p.xs_log2) - 1) >> p.xs_log2) < UNC_BLOCKS) --p.xs_log2;
  p.xs = 1 << p.xs_log2;
  p.runs = (X + p.xs - 1) / p.xs; p.Yb = (Y + brick - 1) / brick; p.Xb = (X + brick - 1) / brick;
  const long long blocks = brick_rows * p.runs;
  IUNET_REQUIRE(blocks <= 0x7fffffffll, "uncertainty_volume: volume %d x %d x %d at brick %d exceeds the grid", Z, Y, X, brick);
  p.ls_p = unc_row_lds(p.xs, C); p.ls_w = weight ? unc_row_lds(p.xs, wch) : 0; p.ls_i = image ? unc_row_lds(p.xs, ich) : 0;
  auto magic = [](int ls) { return ls ? (unsigned int)(((1ull << 32) + (unsigned)(ls >> 4) - 1) / (unsigned)(ls >> 4)) : 0u; };   // ls / 16 >= 2
  p.magic_p = magic(p.ls_p); p.magic_w = magic(p.ls_w); p.magic_i = magic(p.ls_i);
  const int rstep = UNC_THREADS >> p.xs_log2, ls = p.ls_p + p.ls_w + p.ls_i;
  p.rb = UNC_LDS / ls / rstep * rstep;
  if (p.rb < rstep) p.rb = rstep;
  const int batches = (brick * brick + p.rb - 1) / p.rb;                 // of a whole brick row; evened out: 64 rows go as 22 + 22 + 20, not 31 + 31 + 2
  p.rb = ((brick * brick + batches - 1) / batches + rstep - 1) / rstep * rstep;
  const int lds = p.rb * ls + 16;                                           // at most UNC_LDS, or one step's rows: 16 x (16 x 22 + 48) bytes
  if (C == 2) {
    if (weight) uncertainty_launch<true, true>(p, (unsigned)blocks, lds, (hipStream_t)stream);
    else uncertainty_launch<true, false>(p, (unsigned)blocks, lds, (hipStream_t)stream);
  } else {
    if (weight) uncertainty_launch<false, true>(p, (unsigned)blocks, lds, (hipStream_t)stream);
    else uncertainty_launch<false, false>(p, (unsigned)blocks, lds, (hipStream_t)stream);
  }
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

// bytes of iunet_plane_scores' workspace: one (sum, count) int pair per workgroup; 0 where P or sw is out of range
long long iunet_plane_scores_ws_bytes(int P, int sw) {
  if (P < 1 || P > 65535 || sw < 1 || sw > 4096) return 0;
  return (long long)P * score_blocks(sw) * (long long)sizeof(int2);
}

// u: uint8 [Z][Y][X]; geoms: P x 9 doubles (a[3], b[3], origin[3]) ON THE DEVICE; out: int64 [P][2] = (score, inside); all on the device.
int iunet_plane_scores(const void* u, int Z, int Y, int X, const void* geoms, int P, int sw, int start, void* ws, long long ws_bytes,
                       void* out, void* stream) {
  IUNET_REQUIRE(u && geoms && ws && out, "plane_scores: null pointer");
  IUNET_REQUIRE(volume_ok(Z, Y, X, VOLUME_MAX_SAMPLED), "plane_scores: volume %d x %d x %d", Z, Y, X);
  IUNET_REQUIRE(P >= 1 && P <= 65535, "plane_scores: %d planes outside 1..65535", P);
  IUNET_REQUIRE(sw >= 1 && sw <= 4096, "plane_scores: slice width %d outside 1..4096", sw);
  IUNET_REQUIRE(ws_bytes >= iunet_plane_scores_ws_bytes(P, sw), "plane_scores: workspace of %lld bytes, %lld needed", ws_bytes,
                iunet_plane_scores_ws_bytes(P, sw));
  ScoreParams p;
  p.u = (const unsigned char*)u; p.dim[0] = Z; p.dim[1] = Y; p.dim[2] = X;
  p.geoms = (const double*)geoms; p.sw = sw; p.start = start; p.ws = (int2*)ws;
  hipLaunchKernelGGL(plane_scores_kernel, dim3((sw + 63) / 64, (sw + SCORE_ROWS - 1) / SCORE_ROWS, P), dim3(256), 0, (hipStream_t)stream, p);
  IUNET_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(plane_scores_finish_kernel, dim3(P), dim3(64), 0, (hipStream_t)stream, (const int2*)ws, (int)score_blocks(sw),
                     (long long*)out);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

}  // extern "C"
