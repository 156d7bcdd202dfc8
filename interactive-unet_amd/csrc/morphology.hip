// Exact Euclidean distance transform of a resident volume and what is built on it: dilation, erosion, opening and closing by a ball
// (defined bit for bit by tests/morphology_ref.py).  Integers only, no atomics, every element has one owner: the
// same bits on every launch.  The squared distance separates into three passes, each its own launch; launch boundaries are the only
// global synchronisation, no thread ever waits for another (no lock, flag, ticket or spin).
//
//   row_kernel      pass X, a workgroup per row (several rows above ED_MAX_GRID: a trip count fixed at launch).  Class per voxel (argmax
//                   for C >= 2) or the threshold of an earlier distance map, membership, and the seeds of 64 voxels as one ballot word in
//                   LDS -- the wave first.  Then across waves: the last seed position at or before each word (a max-scan) and the first
//                   at or after it (a min-scan), Hillis-Steele over the row's <= 725 words, ceil(log2(words)) steps fixed at launch.  A
//                   voxel finds its nearest seed to the left and right in its own word by clz / ffs, else in the scanned neighbours, and
//                   writes g^2, or INF in a row without a seed.  Rows longer than the workgroup go in chunks of 256, a fixed trip count.
//   column_kernel   passes Y and Z, one thread per column, adjacent threads adjacent x: the exact lower envelope D(u) = min_i f(i) + (u - i)^2
//                   by Meijster's two scans.  The forward scan has a trip count fixed at launch (the column's length, eight entries loaded
//                   ahead as one block); its inner loop pops the stack of envelope parabolas, which holds at most one entry per column
//                   entry passed, so it strictly consumes a bounded stack.  The backward scan has the same fixed trip count.  Entries with
//                   f = INF never enter the envelope (the sums below would overflow).  The stack (site uint16, start uint16, f int32 = one 8-byte
//                   entry per voxel, laid out [k][column] like the volume) lives in the workspace: the pass runs in place on d2 -- the
//                   forward scan reads the whole column before the backward scan writes it, and the backward scan reads f from the stack.
//   <.., true>      the feature transform: the same passes carrying one more value, idx, the raster index of the nearest
//                   seed.  The row pass records which of its two candidates won (the left on a tie).  A column pass writes, beside d2[u],
//                   idx_out[u] = idx_in[site] of the parabola that governs u, read once per parabola as the backward scan reaches it; idx_in
//                   is the map the pass before wrote and idx_out another one (the caller's and a spare in the workspace, alternating),
//                   so no entry is read after this pass has overwritten it.  The <.., false> instantiations are the kernels as they were.
//   the select      one streaming pass, volume_select_kernel (volume_rules.h) with SelectPick: out = value where the distance passes the
//                   threshold (and the class is `only`), else cls.
//
// Ranges.  Every axis <= 46341 and (Z-1)^2 + (Y-1)^2 + (X-1)^2 <= 2^31 - 2, so a finite f(i) + (u - i)^2 is a true squared distance
// inside the volume or the sum of one (< 2^31) and a square (< 2^31): below 2^32, compared as unsigned.  The numerator of
// Sep(i, u) = (u^2 - i^2 + f(u) - f(i)) div 2 (u - i) is formed in 64 bits; where it is used the stack's top is no worse than u at its own
// start t >= 0, so the crossing lies at or after t: the numerator is >= 0, and it is <= u^2 + f(u) <= 2^31 - 2.  All linear indices are
// 64-bit: d2 passes 2^32 bytes at 2^30 voxels.
#include "common.h"
#include "volume_rules.h"
#include <cstdint>

namespace {

constexpr int ED_THREADS = 256, ED_WAVES = ED_THREADS / 64;
constexpr int ED_INF = 0x7fffffff;
constexpr int ED_MAX_AXIS = 46341;                                  // 46340^2 < 2^31 - 1 <= 46341^2
constexpr long long ED_MAX_SQ = 0x7ffffffell;                       // the largest finite squared distance: 2^31 - 2
constexpr long long ED_MAX_VOX = 0x7fffffffll;
constexpr int ED_WORDS = (ED_MAX_AXIS + 63) / 64;                   // ballot words of the longest row: 725
constexpr int ED_WORDS_PER_THREAD = (ED_WORDS + ED_THREADS - 1) / ED_THREADS;
constexpr int ED_NONE = 1 << 30;                                    // no seed on this side
constexpr long long ED_MAX_GRID = 1ll << 20;                        // more rows / column groups than this: a workgroup takes several
constexpr int ED_AHEAD = 8;                                         // column entries loaded ahead of the forward scan
constexpr int ED_CHUNK = 4096;                                      // voxels of one workgroup of the streaming pass: <= 2^19 workgroups

static_assert(ED_WORDS_PER_THREAD * ED_THREADS >= ED_WORDS && ED_MAX_AXIS <= 65535, "the scan covers the longest row; positions fit uint16");

struct RowParams {
  const unsigned char* src;    // CT != 3
  const int* prev;             // CT == 3: the distance map whose threshold gives the seeds
  int* d2;                     // NULL: the class-map pass alone
  unsigned char* cls;          // optional output (CT != 3)
  int X, C, target, invert, r2, above;
  int words;                   // ceil(X / 64)
  long long rows;
  int* idx;                    // F: the raster index of the row's nearest seed (the left one of two equally near), -1 in a row without one
};

// CT: 1 a class map, 2 two classes, 0 any number of classes, 3 a distance map
template <int CT>
__device__ __forceinline__ bool voxel_seed(const RowParams& p, long long v) {
  if (CT == 3) {
    const int d = p.prev[v];
    return p.above ? d > p.r2 : d <= p.r2;
  }
  const TopByte t = volume_top_byte<CT>(p.src, v, p.C);  // volume_rules.h
  if (p.cls) p.cls[v] = (unsigned char)t.at;
  // all bytes 0: never predicted, class map 0 (t.at == 0 there), member of no class
  return (t.best > 0 && t.at == p.target) != (p.invert != 0);
}

// F: the feature transform -- the pass also records which seed is the nearest
template <int CT, bool F>
__global__ __launch_bounds__(ED_THREADS) void row_kernel(RowParams p) {
  __shared__ unsigned long long bits[ED_WORDS];
  __shared__ int L[ED_WORDS], R[ED_WORDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunks = (p.X + ED_THREADS - 1) / ED_THREADS;
  // trip count fixed at launch; uniform over the workgroup (the barriers below)
  for (long long row = blockIdx.x; row < p.rows; row += gridDim.x) {
    const long long base = row * p.X;
    for (int k = 0; k < chunks; ++k) {                   // fixed trip count
      const int x = k * ED_THREADS + threadIdx.x;
      const bool seed = x < p.X && voxel_seed<CT>(p, base + x);
      const unsigned long long m = __ballot(seed);
      const int w = k * ED_WAVES + wave;
      if (lane == 0 && w < p.words) {
        bits[w] = m;
        L[w] = m ? w * 64 + 63 - __clzll((long long)m) : -1;
        R[w] = m ? w * 64 + __ffsll((long long)m) - 1 : ED_NONE;
      }
    }
    if (p.d2 == nullptr) continue;                       // uniform: the class-map pass alone, no barrier was met
    __syncthreads();
    for (int off = 1; off < p.words; off <<= 1) {        // ceil(log2(words)) steps: fixed at launch, uniform
      int l[ED_WORDS_PER_THREAD], r[ED_WORDS_PER_THREAD];
#pragma unroll
      for (int j = 0; j < ED_WORDS_PER_THREAD; ++j) {
        const int w = threadIdx.x + j * ED_THREADS;
        if (w < p.words) {
          l[j] = w >= off ? max(L[w], L[w - off]) : L[w];
          r[j] = w + off < p.words ? min(R[w], R[w + off]) : R[w];
        }
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < ED_WORDS_PER_THREAD; ++j) {
        const int w = threadIdx.x + j * ED_THREADS;
        if (w < p.words) { L[w] = l[j]; R[w] = r[j]; }
      }
      __syncthreads();
    }
    const bool none = L[p.words - 1] < 0;                // a row without a seed
    for (int k = 0; k < chunks; ++k) {                   // fixed trip count
      const int x = k * ED_THREADS + threadIdx.x;
      if (x >= p.X) break;
      int out = ED_INF, at = -1;
      if (!none) {
        const int w = x >> 6, b = x & 63;
        const unsigned long long m = bits[w];
        const unsigned long long lo = m & ((2ull << b) - 1ull), hi = m & ~((1ull << b) - 1ull);
        const int left = lo ? w * 64 + 63 - __clzll((long long)lo) : (w > 0 ? L[w - 1] : -1);
        const int right = hi ? w * 64 + __ffsll((long long)hi) - 1 : (w + 1 < p.words ? R[w + 1] : ED_NONE);
        const int gl = left < 0 ? ED_NONE : x - left, gr = right == ED_NONE ? ED_NONE : right - x;
        const int g = min(gl, gr);                       // <= 46340: one side has a seed
        out = g * g;
        if (F) at = (int)(base + (gl <= gr ? left : right));   // the left seed on a tie: the smaller raster index; below 2^31 - 1
      }
      p.d2[base + x] = out;
      if (F) p.idx[base + x] = at;
    }
    __syncthreads();                                     // the next row overwrites the tables
  }
}

struct ColParams {
  int* d2;
  uint2* stack;                // a column's envelope: x = the parabola's site | the first entry it governs << 16, y = f at the site
  long long ncols;             // columns of this pass
  long long stride;            // between the entries of a column
  long long plane;             // inner pass (Y): Y X; a column is (z, x) = (c / X, c % X)
  int X, n, inner;
  const int* idx_in;           // F: the pass before's nearest seed of every entry (-1 where f = INF) ...
  int* idx_out;                // ... and this pass's: another buffer, so no entry is read after this pass has written it
};

// F: the feature transform -- the backward scan also writes the governing site's seed, idx_out[u] = idx_in[site].  The envelope keeps the
// smaller site on every tie (a later site governs from 1 + Sep on: only where it is strictly better; the top is popped only when it is
// strictly worse), so of equally near seeds the one in the smaller plane / row wins: the smallest raster index.
template <bool F>
__global__ __launch_bounds__(ED_THREADS) void column_kernel(ColParams p) {
  // trip count fixed at launch (no barrier in here: it need not be uniform)
  for (long long c = (long long)blockIdx.x * ED_THREADS + threadIdx.x; c < p.ncols; c += (long long)gridDim.x * ED_THREADS) {
    const long long first = p.inner ? (c / p.X) * p.plane + c % p.X : c;
    int* col = p.d2 + first;
    uint2* mine = p.stack + c;                           // entry k of this column's stack: mine[k ncols]
    int q = -1, ts = 0, tt = 0;                          // the stack's height - 1 and its top, kept in registers
    unsigned int tf = 0;
    for (int u0 = 0; u0 < p.n; u0 += ED_AHEAD) {         // fixed trip count
      int f[ED_AHEAD];
#pragma unroll
      for (int j = 0; j < ED_AHEAD; ++j) f[j] = u0 + j < p.n ? col[(long long)(u0 + j) * p.stride] : ED_INF;
#pragma unroll
      for (int j = 0; j < ED_AHEAD; ++j) {
        const int u = u0 + j, fu = f[j];
        if (fu == ED_INF) continue;                      // no seed in this row (or past the column's end): never in the envelope
        // pops while the top is worse than u already where the top begins.  terminates: q strictly falls and stops at -1
        while (q >= 0) {
          const unsigned int a = (unsigned int)((tt - ts) * (tt - ts)) + tf, b = (unsigned int)((tt - u) * (tt - u)) + (unsigned int)fu;
          if (a <= b) break;
          --q;
          if (q >= 0) {
            const uint2 e = mine[q * p.ncols];
            ts = (int)(e.x & 0xffffu); tt = (int)(e.x >> 16); tf = e.y;
          }
        }
        bool push = true;
        int from = 0;
        if (q >= 0) {
          const long long num = (long long)u * u - (long long)ts * ts + (long long)fu - (long long)tf;     // 0 .. 2^31 - 2 (header)
          from = 1 + (int)((unsigned int)num / (unsigned int)(2 * (u - ts)));
          push = from < p.n;
        }
        if (push) {
          ++q;
          ts = u; tt = from; tf = (unsigned int)fu;
          mine[q * p.ncols] = make_uint2((unsigned int)ts | ((unsigned int)tt << 16), tf);
        }
      }
    }
    if (q < 0) {                                         // a column without a seed: INF already
      if (F) for (int u = 0; u < p.n; ++u) p.idx_out[first + (long long)u * p.stride] = -1;      // fixed trip count
      continue;
    }
    int at = 0;
    if (F) at = p.idx_in[first + (long long)ts * p.stride];
    for (int u = p.n - 1; u >= 0; --u) {                 // fixed trip count; the bottom entry begins at 0, so q >= 0 down to u == 0
      col[(long long)u * p.stride] = (u - ts) * (u - ts) + (int)tf;
      if (F) p.idx_out[first + (long long)u * p.stride] = at;
      if (u == tt && q > 0) {
        --q;
        const uint2 e = mine[q * p.ncols];
        ts = (int)(e.x & 0xffffu); tt = (int)(e.x >> 16); tf = e.y;
        if (F) at = p.idx_in[first + (long long)ts * p.stride];
      }
    }
  }
}

// the select's rule for volume_select_kernel: `value` where the distance passes the threshold (and the class is `only`), else the class
struct SelectPick {
  int r2, above, only, value;
  __device__ __forceinline__ unsigned char operator()(int d, unsigned char c) const {
    const bool cond = above ? d > r2 : d <= r2;
    return (cond && (only < 0 || c == only)) ? (unsigned char)value : c;
  }
};

inline bool ed_volume_ok(int Z, int Y, int X) {
  if (!volume_ok(Z, Y, X, ED_MAX_VOX) || Z > ED_MAX_AXIS || Y > ED_MAX_AXIS || X > ED_MAX_AXIS) return false;
  return (long long)(Z - 1) * (Z - 1) + (long long)(Y - 1) * (Y - 1) + (long long)(X - 1) * (X - 1) <= ED_MAX_SQ;
}

// The feature transform's idx alternates between the caller's map and a spare one in the workspace, pass by pass; the row pass begins in
// the one from which the column passes that will run (an axis of one entry has none) end in the caller's.
inline int* ed_row_idx(int* idx, int* spare, int Z, int Y) { return ((Y > 1) != (Z > 1)) ? spare : idx; }

// passes Y and Z in place on d2; an axis of one entry is its own envelope.  idx: NULL, or the feature transform's map (ed_row_idx)
int ed_columns(int* d2, int Z, int Y, int X, void* ws, hipStream_t st, int* idx = nullptr, int* spare = nullptr) {
  ColParams c;
  c.d2 = d2;
  c.stack = (uint2*)ws;
  c.X = X;
  c.plane = (long long)Y * X;
  c.idx_in = nullptr; c.idx_out = idx ? ed_row_idx(idx, spare, Z, Y) : nullptr;
  void (*column)(ColParams) = idx ? column_kernel<true> : column_kernel<false>;
  if (Y > 1) {
    c.ncols = (long long)Z * X; c.stride = X; c.n = Y; c.inner = 1;
    c.idx_in = c.idx_out; c.idx_out = c.idx_in == idx ? spare : idx;
    hipLaunchKernelGGL(column, dim3(volume_grid((c.ncols + ED_THREADS - 1) / ED_THREADS, ED_MAX_GRID)), dim3(ED_THREADS), 0, st, c);
    IUNET_CHECK_HIP(hipGetLastError());
  }
  if (Z > 1) {
    c.ncols = c.plane; c.stride = c.plane; c.n = Z; c.inner = 0;
    c.idx_in = c.idx_out; c.idx_out = c.idx_in == idx ? spare : idx;
    hipLaunchKernelGGL(column, dim3(volume_grid((c.ncols + ED_THREADS - 1) / ED_THREADS, ED_MAX_GRID)), dim3(ED_THREADS), 0, st, c);
    IUNET_CHECK_HIP(hipGetLastError());
  }
  return IUNET_OK;
}

}  // namespace

extern "C" {

// the workspace: the columns' stacks, 8 bytes per voxel, a multiple of 16 bytes
long long iunet_edt_ws_bytes(int Z, int Y, int X) {
  if (!ed_volume_ok(Z, Y, X)) return 0;
  const long long N = (long long)Z * Y * X;
  return volume_align16(8 * N);
}

int iunet_edt_sq(const void* src, int Z, int Y, int X, int C, int target, int invert,
                 void* d2, void* cls, void* ws, long long ws_bytes, void* stream) {
  IUNET_REQUIRE(src && (d2 || cls), "edt_sq: null pointer (src; d2 and cls both)");
  VOLUME_REQUIRE_DIMS("edt_sq", Z, Y, X);
  IUNET_REQUIRE(ed_volume_ok(Z, Y, X), "edt_sq: volume %d x %d x %d: more than 2^31 - 1 voxels or a squared diagonal above 2^31 - 2", Z, Y, X);
  IUNET_REQUIRE(C >= 1 && C <= 16, "edt_sq: %d classes outside 1..16", C);
  IUNET_REQUIRE(target >= 0 && target <= 255, "edt_sq: target %d outside 0..255", target);
  IUNET_REQUIRE(invert == 0 || invert == 1, "edt_sq: invert %d (0 or 1)", invert);
  if (d2) {
    IUNET_REQUIRE(ws, "edt_sq: null pointer (ws)");
    IUNET_REQUIRE(ws_bytes >= iunet_edt_ws_bytes(Z, Y, X), "edt_sq: workspace of %lld bytes, %lld needed", ws_bytes, iunet_edt_ws_bytes(Z, Y, X));
    IUNET_REQUIRE((((uintptr_t)d2 | (uintptr_t)ws) & 3) == 0, "edt_sq: d2 and the workspace must be 4-byte aligned");
  }
  hipStream_t st = (hipStream_t)stream;
  RowParams p;
  p.src = (const unsigned char*)src; p.prev = nullptr; p.d2 = (int*)d2; p.cls = (unsigned char*)cls;
  p.X = X; p.C = C; p.target = target; p.invert = invert; p.r2 = 0; p.above = 0;
  p.words = (X + 63) / 64;
  p.rows = (long long)Z * Y;
  p.idx = nullptr;
  void (*row[3])(RowParams) = {row_kernel<0, false>, row_kernel<1, false>, row_kernel<2, false>};
  hipLaunchKernelGGL(row[C <= 2 ? C : 0], dim3(volume_grid(p.rows, ED_MAX_GRID)), dim3(ED_THREADS), 0, st, p);
  IUNET_CHECK_HIP(hipGetLastError());
  return d2 ? ed_columns((int*)d2, Z, Y, X, ws, st) : IUNET_OK;
}

int iunet_edt_sq_mask(const void* prev, int Z, int Y, int X, int r2, int above,
                      void* d2, void* ws, long long ws_bytes, void* stream) {
  IUNET_REQUIRE(prev && d2 && ws, "edt_sq_mask: null pointer (prev, d2, ws)");
  VOLUME_REQUIRE_DIMS("edt_sq_mask", Z, Y, X);
  IUNET_REQUIRE(ed_volume_ok(Z, Y, X), "edt_sq_mask: volume %d x %d x %d: more than 2^31 - 1 voxels or a squared diagonal above 2^31 - 2", Z, Y, X);
  IUNET_REQUIRE(r2 >= 0 && r2 <= ED_MAX_SQ, "edt_sq_mask: threshold r2 %d outside 0..2^31 - 2", r2);
  IUNET_REQUIRE(above == 0 || above == 1, "edt_sq_mask: above %d (0 or 1)", above);
  IUNET_REQUIRE(ws_bytes >= iunet_edt_ws_bytes(Z, Y, X), "edt_sq_mask: workspace of %lld bytes, %lld needed", ws_bytes, iunet_edt_ws_bytes(Z, Y, X));
  IUNET_REQUIRE((((uintptr_t)prev | (uintptr_t)d2 | (uintptr_t)ws) & 3) == 0, "edt_sq_mask: prev, d2 and the workspace must be 4-byte aligned");
  const long long N = (long long)Z * Y * X;
  IUNET_REQUIRE((uintptr_t)prev + 4 * (uintptr_t)N <= (uintptr_t)d2 || (uintptr_t)d2 + 4 * (uintptr_t)N <= (uintptr_t)prev,
                "edt_sq_mask: d2 and prev overlap");
  hipStream_t st = (hipStream_t)stream;
  RowParams p;
  p.src = nullptr; p.prev = (const int*)prev; p.d2 = (int*)d2; p.cls = nullptr;
  p.X = X; p.C = 1; p.target = 0; p.invert = 0; p.r2 = r2; p.above = above;
  p.words = (X + 63) / 64;
  p.rows = (long long)Z * Y;
  p.idx = nullptr;
  hipLaunchKernelGGL((row_kernel<3, false>), dim3(volume_grid(p.rows, ED_MAX_GRID)), dim3(ED_THREADS), 0, st, p);
  IUNET_CHECK_HIP(hipGetLastError());
  return ed_columns((int*)d2, Z, Y, X, ws, st);
}

// the feature transform's workspace: the columns' stacks, then the spare idx map: 12 bytes per voxel, each part a multiple of 16 bytes
long long iunet_edt_feature_ws_bytes(int Z, int Y, int X) {
  if (!ed_volume_ok(Z, Y, X)) return 0;
  const long long N = (long long)Z * Y * X;
  return volume_align16(8 * N) + volume_align16(4 * N);
}

int iunet_edt_feature(const void* src, int Z, int Y, int X, int C, int target, int invert,
                      void* d2, void* idx, void* cls, void* ws, long long ws_bytes, void* stream) {
  IUNET_REQUIRE(src && d2 && idx && ws, "edt_feature: null pointer (src, d2, idx, ws)");
  VOLUME_REQUIRE_DIMS("edt_feature", Z, Y, X);
  IUNET_REQUIRE(ed_volume_ok(Z, Y, X), "edt_feature: volume %d x %d x %d: more than 2^31 - 1 voxels or a squared diagonal above 2^31 - 2", Z, Y, X);
  IUNET_REQUIRE(C >= 1 && C <= 16, "edt_feature: %d classes outside 1..16", C);
  IUNET_REQUIRE(target >= 0 && target <= 255, "edt_feature: target %d outside 0..255", target);
  IUNET_REQUIRE(invert == 0 || invert == 1, "edt_feature: invert %d (0 or 1)", invert);
  IUNET_REQUIRE(ws_bytes >= iunet_edt_feature_ws_bytes(Z, Y, X), "edt_feature: workspace of %lld bytes, %lld needed", ws_bytes,
                iunet_edt_feature_ws_bytes(Z, Y, X));
  IUNET_REQUIRE((((uintptr_t)d2 | (uintptr_t)idx | (uintptr_t)ws) & 3) == 0, "edt_feature: d2, idx and the workspace must be 4-byte aligned");
  const long long N = (long long)Z * Y * X;
  IUNET_REQUIRE((uintptr_t)idx + 4 * (uintptr_t)N <= (uintptr_t)d2 || (uintptr_t)d2 + 4 * (uintptr_t)N <= (uintptr_t)idx,
                "edt_feature: d2 and idx overlap");
  hipStream_t st = (hipStream_t)stream;
  int* spare = (int*)((char*)ws + volume_align16(8 * N));
  RowParams p;
  p.src = (const unsigned char*)src; p.prev = nullptr; p.d2 = (int*)d2; p.cls = (unsigned char*)cls;
  p.X = X; p.C = C; p.target = target; p.invert = invert; p.r2 = 0; p.above = 0;
  p.words = (X + 63) / 64;
  p.rows = (long long)Z * Y;
  p.idx = ed_row_idx((int*)idx, spare, Z, Y);
  void (*row[3])(RowParams) = {row_kernel<0, true>, row_kernel<1, true>, row_kernel<2, true>};
  hipLaunchKernelGGL(row[C <= 2 ? C : 0], dim3(volume_grid(p.rows, ED_MAX_GRID)), dim3(ED_THREADS), 0, st, p);
  IUNET_CHECK_HIP(hipGetLastError());
  return ed_columns((int*)d2, Z, Y, X, ws, st, (int*)idx, spare);
}

int iunet_edt_feature_mask(const void* prev, int Z, int Y, int X, int r2, int above,
                           void* d2, void* idx, void* ws, long long ws_bytes, void* stream) {
  IUNET_REQUIRE(prev && d2 && idx && ws, "edt_feature_mask: null pointer (prev, d2, idx, ws)");
  VOLUME_REQUIRE_DIMS("edt_feature_mask", Z, Y, X);
  IUNET_REQUIRE(ed_volume_ok(Z, Y, X), "edt_feature_mask: volume %d x %d x %d: more than 2^31 - 1 voxels or a squared diagonal above 2^31 - 2", Z, Y, X);
  IUNET_REQUIRE(r2 >= 0 && r2 <= ED_MAX_SQ, "edt_feature_mask: threshold r2 %d outside 0..2^31 - 2", r2);
  IUNET_REQUIRE(above == 0 || above == 1, "edt_feature_mask: above %d (0 or 1)", above);
  IUNET_REQUIRE(ws_bytes >= iunet_edt_feature_ws_bytes(Z, Y, X), "edt_feature_mask: workspace of %lld bytes, %lld needed", ws_bytes,
                iunet_edt_feature_ws_bytes(Z, Y, X));
  IUNET_REQUIRE((((uintptr_t)prev | (uintptr_t)d2 | (uintptr_t)idx | (uintptr_t)ws) & 3) == 0,
                "edt_feature_mask: prev, d2, idx and the workspace must be 4-byte aligned");
  const long long N = (long long)Z * Y * X;
  const uintptr_t a = (uintptr_t)prev, b = (uintptr_t)d2, c = (uintptr_t)idx, len = 4 * (uintptr_t)N;
  IUNET_REQUIRE((a + len <= b || b + len <= a) && (a + len <= c || c + len <= a) && (b + len <= c || c + len <= b),
                "edt_feature_mask: prev, d2 and idx overlap");
  hipStream_t st = (hipStream_t)stream;
  int* spare = (int*)((char*)ws + volume_align16(8 * N));
  RowParams p;
  p.src = nullptr; p.prev = (const int*)prev; p.d2 = (int*)d2; p.cls = nullptr;
  p.X = X; p.C = 1; p.target = 0; p.invert = 0; p.r2 = r2; p.above = above;
  p.words = (X + 63) / 64;
  p.rows = (long long)Z * Y;
  p.idx = ed_row_idx((int*)idx, spare, Z, Y);
  hipLaunchKernelGGL((row_kernel<3, true>), dim3(volume_grid(p.rows, ED_MAX_GRID)), dim3(ED_THREADS), 0, st, p);
  IUNET_CHECK_HIP(hipGetLastError());
  return ed_columns((int*)d2, Z, Y, X, ws, st, (int*)idx, spare);
}

int iunet_edt_select(const void* d2, const void* cls, int Z, int Y, int X, int r2, int above, int only, int value,
                     void* out, void* stream) {
  IUNET_REQUIRE(d2 && cls && out, "edt_select: null pointer");
  VOLUME_REQUIRE_DIMS("edt_select", Z, Y, X);
  IUNET_REQUIRE(ed_volume_ok(Z, Y, X), "edt_select: volume %d x %d x %d: more than 2^31 - 1 voxels or a squared diagonal above 2^31 - 2", Z, Y, X);
  IUNET_REQUIRE(r2 >= 0 && r2 <= ED_MAX_SQ, "edt_select: threshold r2 %d outside 0..2^31 - 2", r2);
  IUNET_REQUIRE(above == 0 || above == 1, "edt_select: above %d (0 or 1)", above);
  IUNET_REQUIRE(only >= -1 && only <= 255, "edt_select: only %d outside -1..255", only);
  IUNET_REQUIRE(value >= 0 && value <= 255, "edt_select: value %d outside 0..255", value);
  IUNET_REQUIRE(((uintptr_t)d2 & 3) == 0, "edt_select: d2 must be 4-byte aligned");
  const long long N = (long long)Z * Y * X;
  volume_select_launch<ED_CHUNK, ED_THREADS>(d2, cls, SelectPick{r2, above, only, value}, out, N, (hipStream_t)stream);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

}  // extern "C"
