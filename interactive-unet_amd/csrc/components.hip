// Connected components of a resident volume (defined bit for bit by tests/components_ref.py): label, measure,
// filter.  Integers only; the only atomics are integer minima and sums, so every launch gives the same bits.
//
// A node is a voxel's raster index v = (z Y + y) X + x; P[v] holds parent + 1, 0 for a voxel of no component.  From its first write on
// P[v] <= v + 1: a parent is never behind its child, so every walk towards a root descends, and a root (P[v] == v + 1) is the smallest
// index of its tree.  The passes are separate launches and launch boundaries are the only global synchronisation: no thread ever waits
// for another (no lock, flag, ticket or spin), and every loop has a trip count fixed at launch or strictly decreases an integer.
//
//   tile_kernel     a workgroup owns a tile of CC_TZ x CC_TY x CC_TX voxels, a wave a row of CC_TX = 64 along x.  Class per voxel (argmax
//                   for C >= 2); the row's x-runs are resolved by one ballot (a voxel starts at its run's first voxel), then the runs are
//                   united with the rows behind them by union-find with atomicMin in LDS, only where a pair of runs is met the first
//                   time.  Writes P[v] = the tile-local first voxel + 1, cls and (C >= 2) the key map.  No traffic between workgroups.
//   seam_kernel     the tile pass's grid; the tile's keys and labels and a one-voxel halo are staged in LDS, then voxels on tile faces only:
//                   for each neighbour of the forward half of the structure in ANOTHER tile with the same class, the atomicMin union on P
//                   in global memory (Komura; Playne & Hawick).  P is read by agent-scope relaxed atomic loads and written by agent-scope
//                   atomicMin only; the union is correct for any earlier value of a parent (section 22).
//   flatten_kernel  labels[v] = root + 1; counts the roots of each run of CC_CHUNK voxels.
//   scan_kernel     one workgroup: exclusive scan of the <= 2^19 counts, and K.
//   rank_kernel     a root writes its rank + 1 (roots in raster order = components in order of first voxel) into its own P entry.
//   apply_kernel    labels[v] = P[labels[v] - 1].
//   table kernels   sizes by atomicAdd and first by atomicMin, one pair per (workgroup, label): equal labels next to each other are
//                   summed in the wave by ballot, then in the workgroup in a table in LDS.
//   the filter      one streaming pass: volume_select_kernel (volume_rules.h) with FilterPick.
#include "common.h"
#include "volume_rules.h"
#include <cstdint>

namespace {

constexpr int CC_TZ = 4, CC_TY = 16, CC_TX = 64;     // the tile (interactive_unet/components.py: TILE); CC_TX is the wave
constexpr int CC_ROWS = CC_TZ * CC_TY, CC_TV = CC_ROWS * CC_TX;
constexpr int CC_THREADS = 256, CC_WAVES = CC_THREADS / 64;
constexpr int CC_CHUNK = 4096, CC_STEPS = CC_CHUNK / CC_THREADS;   // voxels of one workgroup of the streaming passes: <= 2^19 workgroups
constexpr long long CC_MAX_VOX = 0x7fffffffll;
constexpr long long CC_MAX_TILE_GRID = 1ll << 20;                  // more tiles than this: a workgroup takes several (fixed trip count)
constexpr int CC_SCAN_THREADS = 1024;

static_assert(CC_TX == 64 && CC_ROWS % CC_WAVES == 0 && CC_TV <= 32768, "a wave per row; tile-local indices fit the LDS table");

struct CcParams {
  const unsigned char* src;
  int* P;
  unsigned char* cls;          // optional output
  unsigned char* key;          // C >= 2: class, or 255 for a voxel of no component (C == 1: src is the key map, none = background)
  int Z, Y, X, C, level, background;
  int nty, ntx;
  long long ntiles;
};

__device__ __forceinline__ int lds_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// terminates: L[x] <= x, the walk goes on only to a strictly smaller index.  On the way every node is handed to its grandparent
// (atomicMin: a parent only falls, and stays an ancestor), which shortens the walks that follow.
__device__ __forceinline__ int lds_find(int* L, int x) {
  int cur = lds_load(L + x);
  if (cur >= x) return x;
  for (;;) {
    const int next = lds_load(L + cur);
    if (next >= cur) return cur;
    atomicMin(L + x, next);
    x = cur;
    cur = next;
  }
}

// terminates: every turn ends or replaces the larger root a by a strictly smaller index (old < a), b never grows: a + b decreases
__device__ __forceinline__ void lds_unite(int* L, int a, int b) {
  for (;;) {
    a = lds_find(L, a);
    b = lds_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(L + a, b);
    if (old >= a) return;          // a was a root: linked
    a = old;                       // a had a parent already (still its ancestor, or replaced by b): unite that one with b
  }
}

// the voxel's class (volume_top_byte, volume_rules.h); a voxel of no component: -1 for a class map, -1 - class for a predicted volume
template <int CT>
__device__ __forceinline__ int voxel_class(const CcParams& p, long long v) {
  const TopByte t = volume_top_byte<CT>(p.src, v, p.C);
  if (CT == 1) return t.at == p.background ? -1 : t.at;
  return (t.best == 0 || t.at == p.background) ? -1 - t.at : t.at;
}

// CT: 1 a class map, 2 two classes, 0 any number; LV: the structure's rank (1, 2, 3 = connectivity 6, 18, 26), so that the offsets it
// leaves out cost nothing
template <int CT, int LV>
__global__ __launch_bounds__(CC_THREADS) void tile_kernel(CcParams p) {
  __shared__ int L[CC_TV];
  __shared__ short cl[CC_TV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // trip count fixed at launch; uniform over the workgroup (the barriers below)
  for (long long t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
    const int tx = (int)(t % p.ntx), ty = (int)((t / p.ntx) % p.nty), tz = (int)(t / ((long long)p.ntx * p.nty));
    const int z0 = tz * CC_TZ, y0 = ty * CC_TY, x0 = tx * CC_TX;
    for (int k = 0; k < CC_ROWS / CC_WAVES; ++k) {       // the wave's 16 rows: a constant trip count, here and below
      const int r = wave + k * CC_WAVES, z = z0 + r / CC_TY, y = y0 + r % CC_TY, x = x0 + lane;
      const bool in = z < p.Z && y < p.Y && x < p.X;
      int c = -1;
      if (in) {
        const long long v = ((long long)z * p.Y + y) * p.X + x;
        c = voxel_class<CT>(p, v);
        const int shown = c < 0 ? (CT == 1 ? p.background : -1 - c) : c;
        if (p.cls) p.cls[v] = (unsigned char)shown;
        if (CT != 1) p.key[v] = (unsigned char)(c < 0 ? 255 : c);
        c = c < 0 ? -1 : c;
      }
      // the row's x-runs by one ballot: a voxel starts at the first voxel of its run
      const int prev = __shfl_up(c, 1, 64);
      const unsigned long long heads = __ballot(lane == 0 || c != prev);
      const int start = 63 - __clzll(heads & ((2ull << lane) - 1ull));
      cl[r * CC_TX + lane] = (short)c;
      L[r * CC_TX + lane] = r * CC_TX + start;
    }
    __syncthreads();
    for (int k = 0; k < CC_ROWS / CC_WAVES; ++k) {
      const int r = wave + k * CC_WAVES, lz = r / CC_TY, ly = r % CC_TY, i = r * CC_TX + lane;
      const int c = cl[i];
      if (c < 0) continue;
      const bool run_l = lane > 0 && cl[i - 1] == c;
#pragma unroll
      for (int h = 0; h < 4; ++h) {                      // the rows behind: (dz, dy) = (0, -1), (-1, 0), (-1, -1), (-1, +1)
        const int dz = h == 0 ? 0 : -1, dy = h == 0 ? -1 : h == 1 ? 0 : h == 2 ? -1 : 1;
        if (lz + dz < 0 || ly + dy < 0 || ly + dy >= CC_TY) continue;
        const int rr = r + dz * CC_TY + dy;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          if ((dz != 0) + (dy != 0) + (dx != 0) > LV) continue;
          const int xx = lane + dx;
          if (xx < 0 || xx >= CC_TX) continue;
          const int j = rr * CC_TX + xx;
          if (cl[j] != c) continue;
          if (run_l && xx > 0 && cl[j - 1] == c) continue;      // the pair of runs was met one voxel to the left
          lds_unite(L, i, j);
        }
      }
    }
    __syncthreads();
    for (int k = 0; k < CC_ROWS / CC_WAVES; ++k) {
      const int r = wave + k * CC_WAVES, z = z0 + r / CC_TY, y = y0 + r % CC_TY, x = x0 + lane;
      if (!(z < p.Z && y < p.Y && x < p.X)) continue;
      const int i = r * CC_TX + lane;
      int out = 0;
      if (cl[i] >= 0) {
        const int root = lds_find(L, i), rr = root / CC_TX;
        out = (int)(((long long)(z0 + rr / CC_TY) * p.Y + (y0 + rr % CC_TY)) * p.X + (x0 + root % CC_TX)) + 1;
      }
      p.P[((long long)z * p.Y + y) * p.X + x] = out;
    }
    __syncthreads();                                     // the next tile overwrites the tables
  }
}

__device__ __forceinline__ int glb_parent(const int* P, int x) {
  return __hip_atomic_load(P + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - 1;
}

// terminates: a parent is <= its child; the walk goes on only to a strictly smaller index.  Any earlier value of a parent is an ancestor.
// On the way every node is handed to its grandparent by atomicMin (the parent it loses stays connected through its own parent link).
__device__ __forceinline__ int glb_find(int* P, int x) {
  int cur = glb_parent(P, x);
  if (cur >= x || cur < 0) return x;
  for (;;) {
    const int next = glb_parent(P, cur);
    if (next >= cur || next < 0) return cur;
    atomicMin(P + x, next + 1);
    x = cur;
    cur = next;
  }
}

// terminates: as lds_unite -- the atomicMin loop ends when the value it replaced was a root, else goes on with a strictly smaller a
__device__ __forceinline__ void glb_unite(int* P, int a, int b) {
  for (;;) {
    a = glb_find(P, a);
    b = glb_find(P, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(P + a, b + 1) - 1;         // agent scope
    if (old >= a || old < 0) return;
    a = old;
  }
}

struct SeamParams {
  const unsigned char* key;
  int* P;
  int Z, Y, X, none;
  int nty, ntx;
  long long ntiles;
};

// The tile pass's grid and lane mapping.  The tile's keys and tile-pass labels and a one-voxel halo (+z, both y, both x) are staged in
// LDS first (key -1 for a voxel of no component or outside the volume): every test below reads LDS, only the unions go to global
// memory.  Rows on the tile's high-z face and on its two y faces take part whole, of the others the voxels on the two x faces.  A pair
// (v, n) is united through its tile-local first voxels, and only where the pair one voxel to the left or one row up -- the same two
// tiles, the same offset -- does not name the same two: a blob that crosses a face costs one union per offset, not one per voxel.
template <int LV>
__global__ __launch_bounds__(CC_THREADS) void seam_kernel(SeamParams p) {
  constexpr int HY = CC_TY + 2, HX = CC_TX + 2, HV = (CC_TZ + 1) * HY * HX;
  __shared__ int pp[HV];
  __shared__ short kk[HV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // trip count fixed at launch; uniform over the workgroup (the barriers below)
  for (long long t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
    const int tx = (int)(t % p.ntx), ty = (int)((t / p.ntx) % p.nty), tz = (int)(t / ((long long)p.ntx * p.nty));
    const int z0 = tz * CC_TZ, y0 = ty * CC_TY, x0 = tx * CC_TX;
    // eight voxels per thread and step, as one basic block whose loads are in flight together: a voxel outside the volume (or behind
    // the table) loads voxel 0 and only its result is dropped
    for (int i0 = threadIdx.x; i0 < HV; i0 += 8 * CC_THREADS) {
      int cs[8], ls[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = i0 + j * CC_THREADS;
        const int z = z0 + i / (HY * HX), y = y0 + i / HX % HY - 1, x = x0 + i % HX - 1;
        const bool in = i < HV && z < p.Z && y >= 0 && y < p.Y && x >= 0 && x < p.X;
        const long long v = in ? ((long long)z * p.Y + y) * p.X + x : 0;
        const int c = p.key[v];
        // any earlier value of a label names an ancestor (a union of this launch may have lowered it already)
        const int l = glb_parent(p.P, (int)v) + 1;
        cs[j] = (in && c != p.none) ? c : -1;
        ls[j] = (in && c != p.none) ? l : 0;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = i0 + j * CC_THREADS;
        if (i < HV) { kk[i] = (short)cs[j]; pp[i] = ls[j]; }
      }
    }
    __syncthreads();
    for (int k = 0; k < CC_ROWS / CC_WAVES; ++k) {
      const int r = wave + k * CC_WAVES, lz = r / CC_TY, ly = r % CC_TY, lx = lane;
      if (lz != CC_TZ - 1 && ly != 0 && ly != CC_TY - 1 && lx != 0 && lx != CC_TX - 1) continue;
      const int at = (lz * HY + ly + 1) * HX + lx + 1;
      const int c = kk[at], mine = pp[at];
      if (c < 0) continue;
#pragma unroll
      for (int o = 14; o < 27; ++o) {                    // the forward half of the 3 x 3 x 3 structure
        const int dz = o / 9 - 1, dy = o / 3 % 3 - 1, dx = o % 3 - 1;
        if ((dz != 0) + (dy != 0) + (dx != 0) > LV) continue;
        if (lz + dz < CC_TZ && ly + dy >= 0 && ly + dy < CC_TY && lx + dx >= 0 && lx + dx < CC_TX) continue;   // the same tile
        const int an = at + (dz * HY + dy) * HX + dx;
        if (kk[an] != c) continue;
        const int other = pp[an];
        // one to the left / one row up: v' in v's tile, n' in n's tile, so their thread meets the same offset across the same seam
        if (lx > 0 && ((lx + dx) & (CC_TX - 1)) != 0 && pp[at - 1] == mine && pp[an - 1] == other) continue;
        if (ly > 0 && ((ly + dy) & (CC_TY - 1)) != 0 && pp[at - HX] == mine && pp[an - HX] == other) continue;
        glb_unite(p.P, mine - 1, other - 1);
      }
    }
    __syncthreads();                                     // the next tile overwrites the tables
  }
}

__global__ __launch_bounds__(CC_THREADS) void flatten_kernel(const int* P, int* labels, int* counts, long long N) {
  __shared__ int part[CC_WAVES];
  const long long base = (long long)blockIdx.x * CC_CHUNK;
  int roots = 0;
  for (int s = 0; s < CC_STEPS; ++s) {                   // fixed trip count
    const long long v = base + s * CC_THREADS + threadIdx.x;
    if (v >= N) break;
    int x = (int)v, out = 0;
    if (P[v] != 0) {
      for (;;) {                                         // terminates: goes on only to a strictly smaller index
        const int q = P[x] - 1;
        if (q >= x || q < 0) break;
        x = q;
      }
      out = x + 1;
      roots += x == (int)v;
    }
    labels[v] = out;
  }
  for (int off = 32; off > 0; off >>= 1) roots += __shfl_down(roots, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = roots;
  __syncthreads();
  if (threadIdx.x == 0) {
    int sum = 0;
    for (int w = 0; w < CC_WAVES; ++w) sum += part[w];
    counts[blockIdx.x] = sum;
  }
}

// counts[b] -> the number of roots before workgroup b's voxels; *count = K.  One workgroup; every loop's trip count is fixed at launch.
__global__ __launch_bounds__(CC_SCAN_THREADS) void scan_kernel(int* counts, int nb, int* count) {
  __shared__ int sums[CC_SCAN_THREADS];
  const int per = (nb + CC_SCAN_THREADS - 1) / CC_SCAN_THREADS, lo = threadIdx.x * per, hi = min(lo + per, nb);
  int sum = 0;
  for (int k = lo; k < hi; ++k) sum += counts[k];
  sums[threadIdx.x] = sum;
  __syncthreads();
  for (int off = 1; off < CC_SCAN_THREADS; off <<= 1) {
    const int add = threadIdx.x >= off ? sums[threadIdx.x - off] : 0;
    __syncthreads();
    sums[threadIdx.x] += add;
    __syncthreads();
  }
  int run = sums[threadIdx.x] - sum;
  for (int k = lo; k < hi; ++k) {
    const int c = counts[k];
    counts[k] = run;
    run += c;
  }
  if (threadIdx.x == CC_SCAN_THREADS - 1) *count = sums[threadIdx.x];
}

__global__ __launch_bounds__(CC_THREADS) void rank_kernel(const int* labels, const int* offsets, int* P, long long N) {
  __shared__ int part[CC_WAVES];
  const long long base = (long long)blockIdx.x * CC_CHUNK;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int run = offsets[blockIdx.x];
  for (int s = 0; s < CC_STEPS; ++s) {                   // fixed trip count, uniform over the workgroup
    const long long v = base + s * CC_THREADS + threadIdx.x;
    const bool root = v < N && labels[v] == (int)v + 1;
    const unsigned long long m = __ballot(root);
    if (lane == 0) part[wave] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < CC_WAVES; ++w) {
      before += w < wave ? part[w] : 0;
      all += part[w];
    }
    if (root) P[v] = run + before + __popcll(m & ((1ull << lane) - 1ull)) + 1;
    run += all;
    __syncthreads();
  }
}

__global__ __launch_bounds__(CC_THREADS) void apply_kernel(int* labels, const int* P, long long N) {
  const long long base = (long long)blockIdx.x * CC_CHUNK;
  for (int s = 0; s < CC_STEPS; ++s) {                   // fixed trip count
    const long long v = base + s * CC_THREADS + threadIdx.x;
    if (v >= N) break;
    const int l = labels[v];
    if (l > 0) labels[v] = P[l - 1];
  }
}

__global__ __launch_bounds__(CC_THREADS) void table_init_kernel(int* sizes, int* first, unsigned char* classes, int K) {
  const long long k = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (k > K) return;
  sizes[k] = 0;
  first[k] = k == 0 ? -1 : 0x7fffffff;
  classes[k] = 0;
}

constexpr int CC_HASH = 1024, CC_HASH_LOG2 = 10, CC_PROBES = 8;     // the workgroup's table of (label, voxels, first voxel)
constexpr int CC_TABLE_GRID = 2048;                                 // workgroups of the table pass: 8 on each of 256 CUs

__device__ __forceinline__ void table_emit(int* sizes, int* first, int label, int n, int at) {
  atomicAdd(sizes + label, n);
  // first only falls: a candidate that does not beat a value read earlier does not beat the present one
  if (at < __hip_atomic_load(first + label, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(first + label, at);
}

// Adds a run of one label to the workgroup's table: linear probing, at most CC_PROBES slots (a fixed trip count; the compare-and-swap
// answers at once, nobody waits for a slot), else straight to global memory.
__device__ __forceinline__ void table_add(int* hk, int* hn, int* hf, int* sizes, int* first, int label, int n, int at) {
  unsigned int h = ((unsigned int)label * 2654435761u) >> (32 - CC_HASH_LOG2);
  for (int t = 0; t < CC_PROBES; ++t) {
    const int old = atomicCAS(hk + h, 0, label);
    if (old == 0 || old == label) {
      atomicAdd(hn + h, n);
      atomicMin(hf + h, at);
      return;
    }
    h = (h + 1) & (CC_HASH - 1);
  }
  table_emit(sizes, first, label, n, at);
}

// A workgroup takes `per` consecutive runs of CC_CHUNK voxels, a wave 64 consecutive voxels per step.  Equal labels next to each other in
// the wave are summed by one ballot; the runs' first lanes add them to the workgroup's table in LDS; at the end one atomic pair per
// (workgroup, label) goes to global memory -- not one per voxel, and not one per run: the giant component of a noisy volume has
// millions of runs.
__global__ __launch_bounds__(CC_THREADS) void table_kernel(const int* labels, int K, int* sizes, int* first, long long N, int per) {
  __shared__ int hk[CC_HASH], hn[CC_HASH], hf[CC_HASH];
  const int lane = threadIdx.x & 63;
  for (int h = threadIdx.x; h < CC_HASH; h += CC_THREADS) { hk[h] = 0; hn[h] = 0; hf[h] = 0x7fffffff; }
  __syncthreads();
  const long long begin = (long long)blockIdx.x * per * CC_CHUNK;
  for (int s = 0; s < per * CC_STEPS; ++s) {              // fixed trip count
    const long long v0 = begin + (long long)s * CC_THREADS + (threadIdx.x - lane), v = v0 + lane;
    if (v0 >= N) break;                                   // uniform over the wave
    int l = v < N ? labels[v] : 0;
    l = (l < 0 || l > K) ? 0 : l;                         // a label outside the table is nobody's
    const int prev = __shfl_up(l, 1, 64);
    const unsigned long long heads = __ballot(lane == 0 || l != prev);
    const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
    const int len = after ? __ffsll((long long)after) : 64 - lane;       // of the run that starts at this lane
    if (((heads >> lane) & 1) && l > 0) table_add(hk, hn, hf, sizes, first, l, len, (int)v);
  }
  __syncthreads();
  for (int h = threadIdx.x; h < CC_HASH; h += CC_THREADS)
    if (hk[h] != 0) table_emit(sizes, first, hk[h], hn[h], hf[h]);
}

__global__ __launch_bounds__(CC_THREADS) void table_classes_kernel(const unsigned char* cls, const int* first, unsigned char* classes, int K,
                                                                   long long N) {
  const long long k = (long long)blockIdx.x * CC_THREADS + threadIdx.x + 1;
  if (k > K) return;
  const int at = first[k];
  classes[k] = (at >= 0 && at < N) ? cls[at] : 0;
}

// the filter's rule for volume_select_kernel: the voxels of a component that is not kept take `fill`
struct FilterPick {
  const unsigned char* keep;
  int K, fill;
  __device__ __forceinline__ unsigned char operator()(int l, unsigned char c) const {
    return (l > 0 && l <= K && !keep[l]) ? (unsigned char)fill : c;
  }
};

inline long long cc_chunks(long long N) { return (N + CC_CHUNK - 1) / CC_CHUNK; }

}  // namespace

extern "C" {

// the workspace: P int32 [N] | key uint8 [N] | counts int32 [ceil(N / CC_CHUNK)], each part a multiple of 16 bytes
long long iunet_cc_ws_bytes(int Z, int Y, int X) {
  if (!volume_ok(Z, Y, X, CC_MAX_VOX)) return 0;
  const long long N = (long long)Z * Y * X;
  return volume_align16(4 * N) + volume_align16(N) + volume_align16(4 * cc_chunks(N));
}

int iunet_cc_label(const void* src, int Z, int Y, int X, int C, int connectivity, int background,
                   void* labels, void* cls, void* count, void* ws, long long ws_bytes, void* stream) {
  IUNET_REQUIRE(src && labels && count && ws, "cc_label: null pointer (src, labels, count, ws)");
  VOLUME_REQUIRE_DIMS("cc_label", Z, Y, X);
  IUNET_REQUIRE(volume_ok(Z, Y, X, CC_MAX_VOX), "cc_label: volume %d x %d x %d: more than 2^31 - 1 voxels", Z, Y, X);
  IUNET_REQUIRE(C >= 1 && C <= 16, "cc_label: %d classes outside 1..16", C);
  IUNET_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, "cc_label: connectivity %d (6, 18 or 26)", connectivity);
  IUNET_REQUIRE(background >= -1 && background <= 255, "cc_label: background %d outside -1..255", background);
  IUNET_REQUIRE(ws_bytes >= iunet_cc_ws_bytes(Z, Y, X), "cc_label: workspace of %lld bytes, %lld needed", ws_bytes, iunet_cc_ws_bytes(Z, Y, X));
  IUNET_REQUIRE((((uintptr_t)labels | (uintptr_t)count | (uintptr_t)ws) & 3) == 0, "cc_label: labels, count and the workspace must be 4-byte aligned");
  const long long N = (long long)Z * Y * X;
  hipStream_t st = (hipStream_t)stream;
  CcParams p;
  p.src = (const unsigned char*)src; p.P = (int*)ws; p.cls = (unsigned char*)cls;
  p.key = (unsigned char*)ws + volume_align16(4 * N);
  int* counts = (int*)((unsigned char*)ws + volume_align16(4 * N) + volume_align16(N));
  p.Z = Z; p.Y = Y; p.X = X; p.C = C; p.level = connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3; p.background = background;
  p.nty = (Y + CC_TY - 1) / CC_TY; p.ntx = (X + CC_TX - 1) / CC_TX;
  p.ntiles = (long long)((Z + CC_TZ - 1) / CC_TZ) * p.nty * p.ntx;
  const unsigned int tgrid = volume_grid(p.ntiles, CC_MAX_TILE_GRID);
  void (*tile[3][3])(CcParams) = {{tile_kernel<0, 1>, tile_kernel<0, 2>, tile_kernel<0, 3>},
                                  {tile_kernel<1, 1>, tile_kernel<1, 2>, tile_kernel<1, 3>},
                                  {tile_kernel<2, 1>, tile_kernel<2, 2>, tile_kernel<2, 3>}};
  hipLaunchKernelGGL(tile[C <= 2 ? C : 0][p.level - 1], dim3(tgrid), dim3(CC_THREADS), 0, st, p);
  IUNET_CHECK_HIP(hipGetLastError());
  const unsigned int chunks = (unsigned int)cc_chunks(N);               // <= 2^19
  SeamParams s;
  s.key = C == 1 ? (const unsigned char*)src : p.key; s.P = p.P; s.Z = Z; s.Y = Y; s.X = X;
  s.none = C == 1 ? background : 255; s.nty = p.nty; s.ntx = p.ntx; s.ntiles = p.ntiles;
  void (*seam[3])(SeamParams) = {seam_kernel<1>, seam_kernel<2>, seam_kernel<3>};
  hipLaunchKernelGGL(seam[p.level - 1], dim3(tgrid), dim3(CC_THREADS), 0, st, s);
  IUNET_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(flatten_kernel, dim3(chunks), dim3(CC_THREADS), 0, st, (const int*)p.P, (int*)labels, counts, N);
  IUNET_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(CC_SCAN_THREADS), 0, st, counts, (int)chunks, (int*)count);
  IUNET_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(rank_kernel, dim3(chunks), dim3(CC_THREADS), 0, st, (const int*)labels, (const int*)counts, p.P, N);
  IUNET_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(apply_kernel, dim3(chunks), dim3(CC_THREADS), 0, st, (int*)labels, (const int*)p.P, N);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_cc_table(const void* labels, const void* cls, int Z, int Y, int X, int K,
                   void* sizes, void* classes, void* first, void* stream) {
  IUNET_REQUIRE(labels && cls && sizes && classes && first, "cc_table: null pointer");
  VOLUME_REQUIRE_DIMS("cc_table", Z, Y, X);
  IUNET_REQUIRE(volume_ok(Z, Y, X, CC_MAX_VOX), "cc_table: volume %d x %d x %d: more than 2^31 - 1 voxels", Z, Y, X);
  IUNET_REQUIRE(K >= 0 && K <= (long long)Z * Y * X, "cc_table: %d components outside 0..the number of voxels", K);
  IUNET_REQUIRE((((uintptr_t)labels | (uintptr_t)sizes | (uintptr_t)first) & 3) == 0, "cc_table: labels, sizes and first must be 4-byte aligned");
  const long long N = (long long)Z * Y * X;
  hipStream_t st = (hipStream_t)stream;
  const unsigned int kgrid = (unsigned int)(((long long)K + CC_THREADS) / CC_THREADS);      // K + 1 entries: <= 2^23 workgroups
  hipLaunchKernelGGL(table_init_kernel, dim3(kgrid), dim3(CC_THREADS), 0, st, (int*)sizes, (int*)first, (unsigned char*)classes, K);
  IUNET_CHECK_HIP(hipGetLastError());
  const long long chunks = cc_chunks(N);
  const int per = (int)((chunks + CC_TABLE_GRID - 1) / CC_TABLE_GRID);                      // <= 2^8
  hipLaunchKernelGGL(table_kernel, dim3((unsigned int)((chunks + per - 1) / per)), dim3(CC_THREADS), 0, st, (const int*)labels, K, (int*)sizes,
                     (int*)first, N, per);
  IUNET_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(table_classes_kernel, dim3(kgrid), dim3(CC_THREADS), 0, st, (const unsigned char*)cls, (const int*)first,
                     (unsigned char*)classes, K, N);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_cc_filter(const void* labels, const void* cls, int Z, int Y, int X, int K, const void* keep, int fill,
                    void* out, void* stream) {
  IUNET_REQUIRE(labels && cls && keep && out, "cc_filter: null pointer");
  VOLUME_REQUIRE_DIMS("cc_filter", Z, Y, X);
  IUNET_REQUIRE(volume_ok(Z, Y, X, CC_MAX_VOX), "cc_filter: volume %d x %d x %d: more than 2^31 - 1 voxels", Z, Y, X);
  IUNET_REQUIRE(K >= 0 && K <= (long long)Z * Y * X, "cc_filter: %d components outside 0..the number of voxels", K);
  IUNET_REQUIRE(fill >= 0 && fill <= 255, "cc_filter: fill %d outside 0..255", fill);
  IUNET_REQUIRE(((uintptr_t)labels & 3) == 0, "cc_filter: labels must be 4-byte aligned");
  const long long N = (long long)Z * Y * X;
  volume_select_launch<CC_CHUNK, CC_THREADS>(labels, cls, FilterPick{(const unsigned char*)keep, K, fill}, out, N, (hipStream_t)stream);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

}  // extern "C"
