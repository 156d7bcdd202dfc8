// Geodesic seeded growth through a resident volume (defined bit for bit by tests/geodesic_ref.py): integer seed
// labels grow through a domain A along the shortest path INSIDE A, under a step metric (w1, w2, w3) for face, edge and vertex steps.
//
// State: one 64-bit key per voxel, the distance g in the high word and the label in the low word, so that the order of the integers is
// the lexicographic order of (g, label).  Off A: all ones.  In A and not reached: (INF, 0), INF = 2^31 - 1.  The result is the one fixed
// point of key[v] = min(key[v], min over neighbours u in A with g[u] < INF of key[u] + (w(u, v) << 32)) below the initial state, and it
// is reached under ANY order of relaxations, stale reads included (section 27): a key only falls, every value it takes is the weight and
// label of a real path, and no state above the fixed point is stable.  A key is read and written as ONE 8-byte access everywhere (a pair
// torn across two 4-byte accesses could lie below the true value and would never be repaired); between workgroups by agent-scope relaxed
// atomic loads and stores.  Launch boundaries are the only global synchronisation: no thread waits for another workgroup (no lock, flag
// wait, ticket or spin), and every loop has a trip count fixed at compile or launch time.
//
//   init_kernel     streaming: the keys from src (class rule, volume_rules.h) or from an int32 domain map, and from seeds; sets every
//                   tile flag.
//   relax_kernel    a workgroup owns a tile of GE_TZ x GE_TY x GE_TX voxels, a wave a row of 64 along x.  It stages the tile and a
//                   one-voxel halo as keys in LDS, sweeps there (read the neighbours, barrier, write if lower, barrier) at most GE_SWEEPS
//                   times, writes back the interior keys that fell and sets flags_out[tile] if any did.  A tile whose own and 26
//                   neighbouring flags_in entries are all 0 leaves after those loads with flags_out = 0: nothing it could read has
//                   changed since it last found nothing to do.  The two flag arrays alternate per round (a launch).
//   finish_kernel   streaming: labels, optionally g, optionally offset + fallback[v] on the voxels of A no seed reached.
//
// The streaming passes as assign_kernel (instances.hip): IN_CHUNK-style chunks, four voxels a thread with 16-byte accesses where every
// map is aligned for them, else one.  64-bit linear indices.
#include "common.h"
#include "volume_rules.h"
#include <cstdint>

namespace {

typedef unsigned long long u64;

constexpr int GE_TZ = 8, GE_TY = 8, GE_TX = 64;                     // the tile; GE_TX is the wave
constexpr int GE_HZ = GE_TZ + 2, GE_HY = GE_TY + 2, GE_HX = GE_TX + 2, GE_HV = GE_HZ * GE_HY * GE_HX;     // with the halo: 52 800 bytes
constexpr int GE_THREADS = 256, GE_WAVES = GE_THREADS / 64, GE_ROWS = GE_TZ * GE_TY, GE_PER = GE_ROWS / GE_WAVES;
constexpr int GE_SWEEPS = 32;                                       // sweeps of a tile in one round: a compile-time cap
constexpr int GE_CHUNK = 4096;                                      // voxels of one workgroup's step of the streaming passes
constexpr long long GE_MAX_GRID = 1ll << 20;
constexpr long long GE_MAX_VOX = 0x7fffffffll;
constexpr long long GE_MAX_DIST = 0x7ffffffell;                     // the largest finite distance: 2^31 - 2
constexpr int GE_MAX_ROUNDS = 1024;                                 // launches of one call
constexpr u64 GE_OFF = ~0ull, GE_UNREACHED = 0x7fffffffull << 32;

static_assert(GE_TX == 64 && GE_ROWS % GE_WAVES == 0 && GE_HV * 8 <= 65536, "a wave per row; the staged tile fits the static LDS limit");

__device__ __forceinline__ u64 key_load(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void key_store(u64* p, u64 k) { __hip_atomic_store(p, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- init ----
struct InitParams {
  const unsigned char* src;
  const int *dom, *seeds;
  u64* key;
  int *flags_a, *flags_b;
  int C, target;
  long long N, chunks, ntiles;
};

__device__ __forceinline__ u64 init_key(bool member, int seed) { return !member ? GE_OFF : seed > 0 ? (u64)(unsigned int)seed : GE_UNREACHED; }

// CT: 1 a class map, 2 two classes, 0 any number of classes, 3 an int32 domain map
template <int CT>
__device__ __forceinline__ bool init_member(const InitParams& p, long long v) {
  if (CT == 3) return p.dom[v] > 0;
  const TopByte t = volume_top_byte<CT>(p.src, v, p.C);
  return t.best > 0 && t.at == p.target;             // all bytes 0: never predicted, member of no class
}

template <int CT, int V>
__global__ __launch_bounds__(GE_THREADS) void init_kernel(InitParams p) {
  for (long long chunk = blockIdx.x; chunk < p.chunks; chunk += gridDim.x) {      // trip count fixed at launch
    for (int s = 0; s < GE_CHUNK / GE_THREADS / V; ++s) {
      const long long v = chunk * GE_CHUNK + ((long long)s * GE_THREADS + threadIdx.x) * V;
      if (v >= p.N) break;
      if (V == 4 && v + 4 <= p.N) {
        const int4 sd = *(const int4*)(p.seeds + v);
        bool m[4];
        if (CT == 1) {
          const uchar4 c = *(const uchar4*)(p.src + v);
          m[0] = c.x == p.target; m[1] = c.y == p.target; m[2] = c.z == p.target; m[3] = c.w == p.target;
        } else if (CT == 3) {
          const int4 d = *(const int4*)(p.dom + v);
          m[0] = d.x > 0; m[1] = d.y > 0; m[2] = d.z > 0; m[3] = d.w > 0;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) m[j] = init_member<CT>(p, v + j);
        }
        *(ulonglong2*)(p.key + v) = make_ulonglong2(init_key(m[0], sd.x), init_key(m[1], sd.y));
        *(ulonglong2*)(p.key + v + 2) = make_ulonglong2(init_key(m[2], sd.z), init_key(m[3], sd.w));
      } else {
        for (int j = 0; j < V && v + j < p.N; ++j) p.key[v + j] = init_key(init_member<CT>(p, v + j), p.seeds[v + j]);
      }
    }
  }
  // the first round has every flag set
  for (long long i = (long long)blockIdx.x * GE_THREADS + threadIdx.x; i < p.ntiles; i += (long long)gridDim.x * GE_THREADS) {
    p.flags_a[i] = 1;
    p.flags_b[i] = 1;
  }
}

// ---- relax ----
struct RelaxParams {
  u64* key;
  const int* flags_in;
  int* flags_out;
  int* count;                  // the last round of a call: the tiles that changed are counted here (zeroed before); else NULL
  int Z, Y, X, ntz, nty, ntx;
  long long ntiles;
  u64 w[3];                    // the step weights, already in the high word; 0: no such step
};

// LV: the highest neighbour rank the metric uses (1 face, 2 edge, 3 vertex), so that the offsets it leaves out cost nothing
template <int LV>
__global__ __launch_bounds__(GE_THREADS) void relax_kernel(RelaxParams p) {
  __shared__ u64 K[GE_HV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // trip count fixed at launch; uniform over the workgroup (the barriers below)
  for (long long t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
    const int tx = (int)(t % p.ntx), ty = (int)((t / p.ntx) % p.nty), tz = (int)(t / ((long long)p.ntx * p.nty));
    int flag = 0;
    if (threadIdx.x < 27) {
      const int nz = tz + (int)threadIdx.x / 9 - 1, ny = ty + ((int)threadIdx.x / 3) % 3 - 1, nx = tx + (int)threadIdx.x % 3 - 1;
      if (nz >= 0 && nz < p.ntz && ny >= 0 && ny < p.nty && nx >= 0 && nx < p.ntx) flag = p.flags_in[((long long)nz * p.nty + ny) * p.ntx + nx];
    }
    if (!__syncthreads_or(flag)) {                       // nothing this tile reads has changed since it last found nothing to do
      if (threadIdx.x == 0) p.flags_out[t] = 0;
      continue;
    }
    const int z0 = tz * GE_TZ, y0 = ty * GE_TY, x0 = tx * GE_TX;
    for (int i = threadIdx.x; i < GE_HV; i += GE_THREADS) {          // the tile and its halo; outside the volume: off A
      const int z = z0 + i / (GE_HX * GE_HY) - 1, y = y0 + (i / GE_HX) % GE_HY - 1, x = x0 + i % GE_HX - 1;
      u64 k = GE_OFF;
      if (z >= 0 && z < p.Z && y >= 0 && y < p.Y && x >= 0 && x < p.X) k = key_load(p.key + ((long long)z * p.Y + y) * p.X + x);
      K[i] = k;
    }
    __syncthreads();
    u64 orig[GE_PER], cur[GE_PER], nw[GE_PER];
#pragma unroll
    for (int k = 0; k < GE_PER; ++k) {                   // the wave's 16 rows: a constant trip count, here and below
      const int r = wave + k * GE_WAVES;
      orig[k] = cur[k] = K[((r / GE_TY + 1) * GE_HY + r % GE_TY + 1) * GE_HX + lane + 1];
    }
    for (int s = 0; s < GE_SWEEPS; ++s) {
      int lower = 0;
#pragma unroll
      for (int k = 0; k < GE_PER; ++k) {
        const int r = wave + k * GE_WAVES, li = ((r / GE_TY + 1) * GE_HY + r % GE_TY + 1) * GE_HX + lane + 1;
        u64 best = cur[k];
        if (best != GE_OFF) {
#pragma unroll
          for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
              for (int dx = -1; dx <= 1; ++dx) {
                const int rank = (dz != 0) + (dy != 0) + (dx != 0);
                if (rank == 0 || rank > LV) continue;
                if (LV == 3 && rank == 2 && p.w[1] == 0) continue;        // (w1, 0, w3): uniform
                const u64 u = K[li + (dz * GE_HY + dy) * GE_HX + dx];
                const u64 c = u < GE_UNREACHED ? u + p.w[rank - 1] : GE_OFF;      // g[u] + w <= 2^31 - 2: the entry point's limit
                best = c < best ? c : best;
              }
        }
        nw[k] = best;
        lower |= best < cur[k];
      }
      if (!__syncthreads_or(lower)) break;               // every read of this sweep is done; uniform
#pragma unroll
      for (int k = 0; k < GE_PER; ++k) {
        if (nw[k] < cur[k]) {
          const int r = wave + k * GE_WAVES;
          K[((r / GE_TY + 1) * GE_HY + r % GE_TY + 1) * GE_HX + lane + 1] = cur[k] = nw[k];
        }
      }
      __syncthreads();
    }
    int changed = 0;
#pragma unroll
    for (int k = 0; k < GE_PER; ++k) {
      if (cur[k] != orig[k]) {                           // only a voxel of A inside the volume ever changes
        const int r = wave + k * GE_WAVES;
        key_store(p.key + ((long long)(z0 + r / GE_TY) * p.Y + (y0 + r % GE_TY)) * p.X + (x0 + lane), cur[k]);
        changed = 1;
      }
    }
    changed = __syncthreads_or(changed);                 // also: the next tile overwrites K
    if (threadIdx.x == 0) {
      p.flags_out[t] = changed;
      if (changed && p.count) atomicAdd(p.count, 1);     // an integer sum: the same on every launch that makes the same changes
    }
  }
}

// ---- finish ----
struct FinishParams {
  const u64* key;
  int *labels, *g;
  const int* fallback;
  int offset;
  long long N, chunks;
};

__device__ __forceinline__ int finish_label(const FinishParams& p, u64 k, int fb) {
  if (k < GE_UNREACHED) return (int)(unsigned int)k;
  return (k == GE_UNREACHED && p.fallback) ? p.offset + fb : 0;
}
__device__ __forceinline__ int finish_g(u64 k) { return k < GE_UNREACHED ? (int)(k >> 32) : 0x7fffffff; }

template <int V>
__global__ __launch_bounds__(GE_THREADS) void finish_kernel(FinishParams p) {
  for (long long chunk = blockIdx.x; chunk < p.chunks; chunk += gridDim.x) {      // trip count fixed at launch
    for (int s = 0; s < GE_CHUNK / GE_THREADS / V; ++s) {
      const long long v = chunk * GE_CHUNK + ((long long)s * GE_THREADS + threadIdx.x) * V;
      if (v >= p.N) break;
      if (V == 4 && v + 4 <= p.N) {
        const ulonglong2 a = *(const ulonglong2*)(p.key + v), b = *(const ulonglong2*)(p.key + v + 2);
        int4 fb = make_int4(0, 0, 0, 0);
        if (p.fallback) fb = *(const int4*)(p.fallback + v);
        *(int4*)(p.labels + v) = make_int4(finish_label(p, a.x, fb.x), finish_label(p, a.y, fb.y), finish_label(p, b.x, fb.z), finish_label(p, b.y, fb.w));
        if (p.g) *(int4*)(p.g + v) = make_int4(finish_g(a.x), finish_g(a.y), finish_g(b.x), finish_g(b.y));
      } else {
        for (int j = 0; j < V && v + j < p.N; ++j) {
          const u64 k = p.key[v + j];
          p.labels[v + j] = finish_label(p, k, p.fallback ? p.fallback[v + j] : 0);
          if (p.g) p.g[v + j] = finish_g(k);
        }
      }
    }
  }
}

// ---- host ----
struct GeoLayout { long long N, ntiles, key_bytes, flag_bytes; int ntz, nty, ntx; };
inline GeoLayout geo_layout(int Z, int Y, int X) {
  GeoLayout l;
  l.N = (long long)Z * Y * X;
  l.ntz = (Z - 1) / GE_TZ + 1; l.nty = (Y - 1) / GE_TY + 1; l.ntx = (X - 1) / GE_TX + 1;      // Z + GE_TZ - 1 could pass 2^31 - 1
  l.ntiles = (long long)l.ntz * l.nty * l.ntx;
  l.key_bytes = volume_align16(8 * l.N); l.flag_bytes = volume_align16(4 * l.ntiles);
  return l;
}

inline bool geo_apart(const void* a, long long alen, const void* b, long long blen) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x + (uintptr_t)alen <= y || y + (uintptr_t)blen <= x;
}

int geo_init(int ct, const void* src, const void* dom, int Z, int Y, int X, int C, int target, const void* seeds, void* ws,
             hipStream_t st) {
  const GeoLayout l = geo_layout(Z, Y, X);
  InitParams p;
  p.src = (const unsigned char*)src; p.dom = (const int*)dom; p.seeds = (const int*)seeds; p.key = (u64*)ws;
  p.flags_a = (int*)((unsigned char*)ws + l.key_bytes); p.flags_b = (int*)((unsigned char*)ws + l.key_bytes + l.flag_bytes);
  p.C = C; p.target = target; p.N = l.N; p.chunks = (l.N + GE_CHUNK - 1) / GE_CHUNK; p.ntiles = l.ntiles;
  const bool wide = ((uintptr_t)seeds & 15) == 0 && ((uintptr_t)dom & 15) == 0 && (ct != 1 || ((uintptr_t)src & 3) == 0);
  void (*kernel[4][2])(InitParams) = {{init_kernel<0, 1>, init_kernel<0, 4>}, {init_kernel<1, 1>, init_kernel<1, 4>},
                                      {init_kernel<2, 1>, init_kernel<2, 4>}, {init_kernel<3, 1>, init_kernel<3, 4>}};
  hipLaunchKernelGGL(kernel[ct][wide], dim3(volume_grid(p.chunks, GE_MAX_GRID)), dim3(GE_THREADS), 0, st, p);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

}  // namespace

// the checks iunet_geo_init and iunet_geo_init_mask share
#define GEO_REQUIRE_VOLUME(who, Z, Y, X)                                                                                     \
  VOLUME_REQUIRE_DIMS(who, Z, Y, X);                                                                                         \
  IUNET_REQUIRE(volume_ok(Z, Y, X, GE_MAX_VOX), who ": volume %d x %d x %d: more than 2^31 - 1 voxels", Z, Y, X)
#define GEO_REQUIRE_WS(who, ws, ws_bytes, Z, Y, X)                                                                           \
  IUNET_REQUIRE(ws_bytes >= iunet_geo_ws_bytes(Z, Y, X), who ": workspace of %lld bytes, %lld needed", (long long)ws_bytes,  \
                iunet_geo_ws_bytes(Z, Y, X));                                                                                \
  IUNET_REQUIRE(((uintptr_t)ws & 15) == 0, who ": the workspace must be 16-byte aligned")

extern "C" {

// the workspace: key uint64 [N] | flags int32 [tiles] | flags int32 [tiles], each part a multiple of 16 bytes
long long iunet_geo_ws_bytes(int Z, int Y, int X) {
  if (!volume_ok(Z, Y, X, GE_MAX_VOX)) return 0;
  const GeoLayout l = geo_layout(Z, Y, X);
  return l.key_bytes + 2 * l.flag_bytes;
}

int iunet_geo_init(const void* src, int Z, int Y, int X, int C, int target, const void* seeds, void* ws, long long ws_bytes, void* stream) {
  IUNET_REQUIRE(src && seeds && ws, "geo_init: null pointer (src, seeds, ws)");
  GEO_REQUIRE_VOLUME("geo_init", Z, Y, X);
  IUNET_REQUIRE(C >= 1 && C <= 16, "geo_init: %d classes outside 1..16", C);
  IUNET_REQUIRE(target >= 0 && target <= 255, "geo_init: target %d outside 0..255", target);
  GEO_REQUIRE_WS("geo_init", ws, ws_bytes, Z, Y, X);
  IUNET_REQUIRE(((uintptr_t)seeds & 3) == 0, "geo_init: seeds must be 4-byte aligned");
  return geo_init(C <= 2 ? C : 0, src, nullptr, Z, Y, X, C, target, seeds, ws, (hipStream_t)stream);
}

int iunet_geo_init_mask(const void* dom, int Z, int Y, int X, const void* seeds, void* ws, long long ws_bytes, void* stream) {
  IUNET_REQUIRE(dom && seeds && ws, "geo_init_mask: null pointer (dom, seeds, ws)");
  GEO_REQUIRE_VOLUME("geo_init_mask", Z, Y, X);
  GEO_REQUIRE_WS("geo_init_mask", ws, ws_bytes, Z, Y, X);
  IUNET_REQUIRE((((uintptr_t)dom | (uintptr_t)seeds) & 3) == 0, "geo_init_mask: dom and seeds must be 4-byte aligned");
  return geo_init(3, nullptr, dom, Z, Y, X, 1, 0, seeds, ws, (hipStream_t)stream);
}

int iunet_geo_relax(void* ws, long long ws_bytes, int Z, int Y, int X, int w1, int w2, int w3, int rounds, void* changed, void* stream) {
  IUNET_REQUIRE(ws && changed, "geo_relax: null pointer (ws, changed)");
  GEO_REQUIRE_VOLUME("geo_relax", Z, Y, X);
  IUNET_REQUIRE(w1 >= 1 && w1 <= 255 && w2 >= 0 && w2 <= 255 && w3 >= 0 && w3 <= 255,
                "geo_relax: weights (%d, %d, %d): w1 in 1..255, w2 and w3 in 0..255", w1, w2, w3);
  const int wmax = w1 > w2 ? (w1 > w3 ? w1 : w3) : (w2 > w3 ? w2 : w3);
  IUNET_REQUIRE((long long)Z * Y * X <= GE_MAX_DIST / wmax, "geo_relax: volume %d x %d x %d at weight %d: a distance could pass 2^31 - 2 (overflow)",
                Z, Y, X, wmax);
  IUNET_REQUIRE(rounds >= 1 && rounds <= GE_MAX_ROUNDS, "geo_relax: %d rounds outside 1..%d", rounds, GE_MAX_ROUNDS);
  GEO_REQUIRE_WS("geo_relax", ws, ws_bytes, Z, Y, X);
  IUNET_REQUIRE(((uintptr_t)changed & 3) == 0, "geo_relax: changed must be 4-byte aligned");
  IUNET_REQUIRE(geo_apart(changed, 4, ws, iunet_geo_ws_bytes(Z, Y, X)), "geo_relax: changed may not overlap the workspace");
  const GeoLayout l = geo_layout(Z, Y, X);
  hipStream_t st = (hipStream_t)stream;
  int* flags[2] = {(int*)((unsigned char*)ws + l.key_bytes), (int*)((unsigned char*)ws + l.key_bytes + l.flag_bytes)};
  RelaxParams p;
  p.key = (u64*)ws; p.Z = Z; p.Y = Y; p.X = X; p.ntz = l.ntz; p.nty = l.nty; p.ntx = l.ntx; p.ntiles = l.ntiles;
  p.w[0] = (u64)w1 << 32; p.w[1] = (u64)w2 << 32; p.w[2] = (u64)w3 << 32;
  void (*kernel)(RelaxParams) = w3 ? relax_kernel<3> : w2 ? relax_kernel<2> : relax_kernel<1>;
  IUNET_CHECK_HIP(hipMemsetAsync(changed, 0, 4, st));
  for (int r = 0; r < rounds; ++r) {
    p.flags_in = flags[r & 1]; p.flags_out = flags[(r + 1) & 1];
    p.count = r == rounds - 1 ? (int*)changed : nullptr;
    hipLaunchKernelGGL(kernel, dim3(volume_grid(l.ntiles, GE_MAX_GRID)), dim3(GE_THREADS), 0, st, p);
    IUNET_CHECK_HIP(hipGetLastError());
  }
  // both arrays leave with the last round's flags: the next call starts from the first again
  IUNET_CHECK_HIP(hipMemcpyAsync(flags[(rounds + 1) & 1], flags[rounds & 1], (size_t)(4 * l.ntiles), hipMemcpyDeviceToDevice, st));
  return IUNET_OK;
}

int iunet_geo_finish(const void* ws, long long ws_bytes, int Z, int Y, int X, void* labels, void* g, const void* fallback, int offset, void* stream) {
  IUNET_REQUIRE(ws && labels, "geo_finish: null pointer (ws, labels)");
  GEO_REQUIRE_VOLUME("geo_finish", Z, Y, X);
  IUNET_REQUIRE(offset >= 0, "geo_finish: offset %d below 0", offset);
  GEO_REQUIRE_WS("geo_finish", ws, ws_bytes, Z, Y, X);
  IUNET_REQUIRE((((uintptr_t)labels | (uintptr_t)g | (uintptr_t)fallback) & 3) == 0, "geo_finish: labels, g and fallback must be 4-byte aligned");
  const long long N = (long long)Z * Y * X, need = iunet_geo_ws_bytes(Z, Y, X);
  IUNET_REQUIRE(geo_apart(labels, 4 * N, ws, need) && (!g || geo_apart(g, 4 * N, ws, need)) && (!g || geo_apart(g, 4 * N, labels, 4 * N)) &&
                (!fallback || (geo_apart(labels, 4 * N, fallback, 4 * N) && (!g || geo_apart(g, 4 * N, fallback, 4 * N)))),
                "geo_finish: labels and g may overlap neither each other, the workspace nor fallback");
  FinishParams p;
  p.key = (const u64*)ws; p.labels = (int*)labels; p.g = (int*)g; p.fallback = (const int*)fallback; p.offset = offset;
  p.N = N; p.chunks = (N + GE_CHUNK - 1) / GE_CHUNK;
  const bool wide = (((uintptr_t)labels | (uintptr_t)g | (uintptr_t)fallback) & 15) == 0;
  hipLaunchKernelGGL(wide ? finish_kernel<4> : finish_kernel<1>, dim3(volume_grid(p.chunks, GE_MAX_GRID)), dim3(GE_THREADS), 0, (hipStream_t)stream, p);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

}  // extern "C"
