// Grayscale morphological reconstruction of a resident int32 volume (defined bit for bit by tests/reconstruct_ref.py):
// by dilation, R is the one fixed point of r[v] = min(mask[v], max(r[v], max over the neighbours u inside the volume of r[u])) above
// r0[v] = min(sat(marker[v] - h), mask[v]); by erosion the dual, min and max exchanged and sat(marker[v] + h).  On it: h-maxima, regional
// and extended maxima, and the markers that split touching objects by the dynamic of their distance map's peaks.
//
// State: one int32 per voxel, r itself.  The fixed point is reached under ANY order of updates, stale reads included (section 28): a value
// only rises (erosion: falls), every value a voxel ever holds is the minimum along a real path from a voxel's r0, so none passes R, and a
// state at rest that does not pass R is R.  A value is one 4-byte word, so no read can tear; between workgroups r goes by agent-scope
// relaxed atomic loads and stores (a plain load may be served from a stale L1 line of another launch).  Launch boundaries are the only
// global synchronisation: no thread waits for another workgroup (no lock, flag wait, ticket or spin), and every loop has a trip count
// fixed at compile or launch time.
//
//   rec_init_kernel       streaming: r0 from marker, mask and h; sets every tile flag.
//   rec_relax_kernel      a workgroup owns a tile of RC_TZ x RC_TY x RC_TX voxels, a wave a row of 64 along x, a thread 16 voxels whose mask
//                         values it keeps in registers.  It stages the tile of r and a one-voxel halo in LDS (outside the volume: -2^31, for
//                         erosion 2^31 - 1), sweeps there (read the neighbours, barrier, write what changed, barrier) at most RC_SWEEPS times,
//                         writes back the interior voxels that changed and sets flags_out[tile] if any did.  A tile whose own and 26
//                         neighbouring flags_in entries are all 0 leaves after those loads with flags_out = 0.  The two flag arrays alternate
//                         per round (a launch).  The tile loop is geodesic.hip's relax_kernel with another state and rule.
//   rec_landscape_kernel  streaming: f = isqrt(scale^2 d2) where d2 > 0, `off` elsewhere; in place or not.
//   rec_select_kernel     streaming: out uint8 = (a - b >= t, the difference in 64 bits) ? value : 0.
//
// The streaming passes as init_kernel (geodesic.hip): chunks, four voxels a thread with 16-byte accesses where every map is aligned for
// them, else one.  64-bit linear indices.
#include "common.h"
#include "volume_rules.h"
#include <cstdint>

namespace {

constexpr int RC_TZ = 8, RC_TY = 8, RC_TX = 64;                     // the tile; RC_TX is the wave
constexpr int RC_HZ = RC_TZ + 2, RC_HY = RC_TY + 2, RC_HX = RC_TX + 2, RC_HV = RC_HZ * RC_HY * RC_HX;     // with the halo: 26 400 bytes
constexpr int RC_THREADS = 256, RC_WAVES = RC_THREADS / 64, RC_ROWS = RC_TZ * RC_TY, RC_PER = RC_ROWS / RC_WAVES;
constexpr int RC_SWEEPS = 32;                                       // sweeps of a tile in one round: a compile-time cap
constexpr int RC_CHUNK = 4096;                                      // voxels of one workgroup's step of the streaming passes
constexpr long long RC_MAX_GRID = 1ll << 20;
constexpr long long RC_MAX_VOX = 0x7fffffffll;
constexpr int RC_MAX_ROUNDS = 1024;                                 // launches of one call
constexpr int RC_LOW = -0x7fffffff - 1, RC_HIGH = 0x7fffffff;

static_assert(RC_TX == 64 && RC_ROWS % RC_WAVES == 0 && RC_HV * 4 <= 65536, "a wave per row; the staged tile fits the static LDS limit");

__device__ __forceinline__ int word_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void word_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ERO 0: by dilation -- values rise towards the mask from below; ERO 1: by erosion, the dual
template <int ERO> __device__ __forceinline__ int rec_pad() { return ERO ? RC_HIGH : RC_LOW; }                        // offers nothing
template <int ERO> __device__ __forceinline__ int rec_spread(int a, int b) { return ERO ? (a < b ? a : b) : (a > b ? a : b); }
template <int ERO> __device__ __forceinline__ int rec_bound(int a, int m) { return ERO ? (a > m ? a : m) : (a < m ? a : m); }
__device__ __forceinline__ int rec_sat(long long v) { return v < RC_LOW ? RC_LOW : v > RC_HIGH ? RC_HIGH : (int)v; }
template <int ERO> __device__ __forceinline__ int rec_first(int marker, int mask, int h) {
  return rec_bound<ERO>(rec_sat(ERO ? (long long)marker + h : (long long)marker - h), mask);
}

// ---- init ----
struct RecInitParams {
  const int *marker, *mask;
  int* r;
  int *flags_a, *flags_b;
  int h;
  long long N, chunks, ntiles;
};

template <int ERO, int V>
__global__ __launch_bounds__(RC_THREADS) void rec_init_kernel(RecInitParams p) {
  for (long long chunk = blockIdx.x; chunk < p.chunks; chunk += gridDim.x) {      // trip count fixed at launch
    for (int s = 0; s < RC_CHUNK / RC_THREADS / V; ++s) {
      const long long v = chunk * RC_CHUNK + ((long long)s * RC_THREADS + threadIdx.x) * V;
      if (v >= p.N) break;
      if (V == 4 && v + 4 <= p.N) {
        const int4 k = *(const int4*)(p.marker + v), m = *(const int4*)(p.mask + v);
        *(int4*)(p.r + v) = make_int4(rec_first<ERO>(k.x, m.x, p.h), rec_first<ERO>(k.y, m.y, p.h), rec_first<ERO>(k.z, m.z, p.h),
                                      rec_first<ERO>(k.w, m.w, p.h));
      } else {
        for (int j = 0; j < V && v + j < p.N; ++j) p.r[v + j] = rec_first<ERO>(p.marker[v + j], p.mask[v + j], p.h);
      }
    }
  }
  // the first round has every flag set
  for (long long i = (long long)blockIdx.x * RC_THREADS + threadIdx.x; i < p.ntiles; i += (long long)gridDim.x * RC_THREADS) {
    p.flags_a[i] = 1;
    p.flags_b[i] = 1;
  }
}

// ---- relax ----
struct RecRelaxParams {
  int* r;
  const int* mask;
  const int* flags_in;
  int* flags_out;
  int* count;                  // the last round of a call: the tiles that changed are counted here (zeroed before); else NULL
  int Z, Y, X, ntz, nty, ntx;
  long long ntiles;
};

// LV: the highest neighbour rank of the connectivity (1 face, 2 edge, 3 vertex), so that the offsets it leaves out cost nothing
template <int LV, int ERO>
__global__ __launch_bounds__(RC_THREADS) void rec_relax_kernel(RecRelaxParams p) {
  __shared__ int R[RC_HV];
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
    const int z0 = tz * RC_TZ, y0 = ty * RC_TY, x0 = tx * RC_TX;
    for (int i = threadIdx.x; i < RC_HV; i += RC_THREADS) {          // the tile and its halo; outside the volume: a value that offers nothing
      // 64-bit: behind the last tile of a dimension of 2^31 - 1 the halo's coordinate is 2^31
      const long long z = (long long)z0 + i / (RC_HX * RC_HY) - 1, y = (long long)y0 + (i / RC_HX) % RC_HY - 1, x = (long long)x0 + i % RC_HX - 1;
      int v = rec_pad<ERO>();
      if (z >= 0 && z < p.Z && y >= 0 && y < p.Y && x >= 0 && x < p.X) v = word_load(p.r + (z * p.Y + y) * p.X + x);
      R[i] = v;
    }
    int m[RC_PER], orig[RC_PER], cur[RC_PER], nw[RC_PER];
#pragma unroll
    for (int k = 0; k < RC_PER; ++k) {                   // the thread's 16 mask values: a constant trip count, here and below
      const int r = wave + k * RC_WAVES, z = z0 + r / RC_TY, y = y0 + r % RC_TY, x = x0 + lane;
      // a voxel of the tile outside the volume: bounded by the pad, it keeps the pad and is never written
      m[k] = (z < p.Z && y < p.Y && x < p.X) ? p.mask[((long long)z * p.Y + y) * p.X + x] : rec_pad<ERO>();
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RC_PER; ++k) {
      const int r = wave + k * RC_WAVES;
      orig[k] = cur[k] = R[((r / RC_TY + 1) * RC_HY + r % RC_TY + 1) * RC_HX + lane + 1];
    }
    for (int s = 0; s < RC_SWEEPS; ++s) {
      int moved = 0;
#pragma unroll
      for (int k = 0; k < RC_PER; ++k) {
        const int r = wave + k * RC_WAVES, li = ((r / RC_TY + 1) * RC_HY + r % RC_TY + 1) * RC_HX + lane + 1;
        int best = cur[k];
#pragma unroll
        for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
          for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
              const int rank = (dz != 0) + (dy != 0) + (dx != 0);
              if (rank == 0 || rank > LV) continue;
              best = rec_spread<ERO>(best, R[li + (dz * RC_HY + dy) * RC_HX + dx]);
            }
        nw[k] = rec_bound<ERO>(best, m[k]);
        moved |= nw[k] != cur[k];
      }
      if (!__syncthreads_or(moved)) break;               // every read of this sweep is done; uniform
#pragma unroll
      for (int k = 0; k < RC_PER; ++k) {
        if (nw[k] != cur[k]) {
          const int r = wave + k * RC_WAVES;
          R[((r / RC_TY + 1) * RC_HY + r % RC_TY + 1) * RC_HX + lane + 1] = cur[k] = nw[k];
        }
      }
      __syncthreads();
    }
    int changed = 0;
#pragma unroll
    for (int k = 0; k < RC_PER; ++k) {
      if (cur[k] != orig[k]) {                           // only a voxel inside the volume ever changes
        const int r = wave + k * RC_WAVES;
        word_store(p.r + ((long long)(z0 + r / RC_TY) * p.Y + (y0 + r % RC_TY)) * p.X + (x0 + lane), cur[k]);
        changed = 1;
      }
    }
    changed = __syncthreads_or(changed);                 // also: the next tile overwrites R
    if (threadIdx.x == 0) {
      p.flags_out[t] = changed;
      if (changed && p.count) atomicAdd(p.count, 1);     // an integer sum: the same on every launch that makes the same changes
    }
  }
}

// ---- landscape and select ----
// floor(sqrt(p)), 0 <= p < 2^47: the double holds p exactly and its square root is within one of the floor
__device__ __forceinline__ int rec_isqrt(long long p) {
  long long s = (long long)sqrt((double)p);
  s -= s * s > p;
  s += (s + 1) * (s + 1) <= p;
  return (int)s;
}
__device__ __forceinline__ int rec_height(int d2, long long scale_sq, int off) { return d2 > 0 ? rec_isqrt(scale_sq * d2) : off; }

template <int V>
__global__ __launch_bounds__(RC_THREADS) void rec_landscape_kernel(const int* d2, int* f, long long scale_sq, int off, long long N, long long chunks) {
  for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {        // trip count fixed at launch
    for (int s = 0; s < RC_CHUNK / RC_THREADS / V; ++s) {
      const long long v = chunk * RC_CHUNK + ((long long)s * RC_THREADS + threadIdx.x) * V;
      if (v >= N) break;
      if (V == 4 && v + 4 <= N) {
        const int4 d = *(const int4*)(d2 + v);
        *(int4*)(f + v) = make_int4(rec_height(d.x, scale_sq, off), rec_height(d.y, scale_sq, off), rec_height(d.z, scale_sq, off),
                                    rec_height(d.w, scale_sq, off));
      } else {
        for (int j = 0; j < V && v + j < N; ++j) f[v + j] = rec_height(d2[v + j], scale_sq, off);
      }
    }
  }
}

__device__ __forceinline__ unsigned char rec_pick(int a, int b, int t, int value) { return (long long)a - b >= t ? (unsigned char)value : 0; }

template <int V>
__global__ __launch_bounds__(RC_THREADS) void rec_select_kernel(const int* a, const int* b, int t, int value, unsigned char* out, long long N,
                                                                long long chunks) {
  for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {        // trip count fixed at launch
    for (int s = 0; s < RC_CHUNK / RC_THREADS / V; ++s) {
      const long long v = chunk * RC_CHUNK + ((long long)s * RC_THREADS + threadIdx.x) * V;
      if (v >= N) break;
      if (V == 4 && v + 4 <= N) {
        const int4 x = *(const int4*)(a + v), y = *(const int4*)(b + v);
        *(uchar4*)(out + v) = make_uchar4(rec_pick(x.x, y.x, t, value), rec_pick(x.y, y.y, t, value), rec_pick(x.z, y.z, t, value),
                                          rec_pick(x.w, y.w, t, value));
      } else {
        for (int j = 0; j < V && v + j < N; ++j) out[v + j] = rec_pick(a[v + j], b[v + j], t, value);
      }
    }
  }
}

// ---- host ----
struct RecLayout { long long N, ntiles, flag_bytes; int ntz, nty, ntx; };
inline RecLayout rec_layout(int Z, int Y, int X) {
  RecLayout l;
  l.N = (long long)Z * Y * X;
  l.ntz = (Z - 1) / RC_TZ + 1; l.nty = (Y - 1) / RC_TY + 1; l.ntx = (X - 1) / RC_TX + 1;      // Z + RC_TZ - 1 could pass 2^31 - 1
  l.ntiles = (long long)l.ntz * l.nty * l.ntx;
  l.flag_bytes = volume_align16(4 * l.ntiles);
  return l;
}

inline bool rec_apart(const void* a, long long alen, const void* b, long long blen) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x + (uintptr_t)alen <= y || y + (uintptr_t)blen <= x;
}

}  // namespace

#define REC_REQUIRE_VOLUME(who, Z, Y, X)                                                                                     \
  VOLUME_REQUIRE_DIMS(who, Z, Y, X);                                                                                         \
  IUNET_REQUIRE(volume_ok(Z, Y, X, RC_MAX_VOX), who ": volume %d x %d x %d: more than 2^31 - 1 voxels", Z, Y, X)
#define REC_REQUIRE_WS(who, ws, ws_bytes, Z, Y, X)                                                                           \
  IUNET_REQUIRE(ws_bytes >= iunet_rec_ws_bytes(Z, Y, X), who ": workspace of %lld bytes, %lld needed", (long long)ws_bytes,  \
                iunet_rec_ws_bytes(Z, Y, X));                                                                                \
  IUNET_REQUIRE(((uintptr_t)ws & 15) == 0, who ": the workspace must be 16-byte aligned")

extern "C" {

// the workspace: flags int32 [tiles] | flags int32 [tiles], each a multiple of 16 bytes
long long iunet_rec_ws_bytes(int Z, int Y, int X) {
  if (!volume_ok(Z, Y, X, RC_MAX_VOX)) return 0;
  return 2 * rec_layout(Z, Y, X).flag_bytes;
}

int iunet_rec_landscape(const void* d2, int Z, int Y, int X, int scale, int off, void* f, void* stream) {
  IUNET_REQUIRE(d2 && f, "rec_landscape: null pointer (d2, f)");
  REC_REQUIRE_VOLUME("rec_landscape", Z, Y, X);
  IUNET_REQUIRE(scale >= 1 && scale <= 256, "rec_landscape: scale %d outside 1..256", scale);
  IUNET_REQUIRE((((uintptr_t)d2 | (uintptr_t)f) & 3) == 0, "rec_landscape: d2 and f must be 4-byte aligned");
  const long long N = (long long)Z * Y * X, chunks = (N + RC_CHUNK - 1) / RC_CHUNK;
  IUNET_REQUIRE(f == d2 || rec_apart(f, 4 * N, d2, 4 * N), "rec_landscape: f is d2 itself or may not overlap it");
  const bool wide = (((uintptr_t)d2 | (uintptr_t)f) & 15) == 0;
  hipLaunchKernelGGL(wide ? rec_landscape_kernel<4> : rec_landscape_kernel<1>, dim3(volume_grid(chunks, RC_MAX_GRID)), dim3(RC_THREADS), 0,
                     (hipStream_t)stream, (const int*)d2, (int*)f, (long long)scale * scale, off, N, chunks);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_rec_init(const void* marker, const void* mask, int Z, int Y, int X, int h, int erosion, void* r, void* ws, long long ws_bytes,
                   void* stream) {
  IUNET_REQUIRE(marker && mask && r && ws, "rec_init: null pointer (marker, mask, r, ws)");
  REC_REQUIRE_VOLUME("rec_init", Z, Y, X);
  IUNET_REQUIRE(h >= 0, "rec_init: h %d below 0", h);
  IUNET_REQUIRE(erosion == 0 || erosion == 1, "rec_init: erosion %d: 0 (by dilation) or 1", erosion);
  REC_REQUIRE_WS("rec_init", ws, ws_bytes, Z, Y, X);
  IUNET_REQUIRE((((uintptr_t)marker | (uintptr_t)mask | (uintptr_t)r) & 3) == 0, "rec_init: marker, mask and r must be 4-byte aligned");
  const RecLayout l = rec_layout(Z, Y, X);
  IUNET_REQUIRE(rec_apart(r, 4 * l.N, marker, 4 * l.N) && rec_apart(r, 4 * l.N, mask, 4 * l.N) && rec_apart(r, 4 * l.N, ws, 2 * l.flag_bytes),
                "rec_init: r may overlap neither marker, mask nor the workspace");
  RecInitParams p;
  p.marker = (const int*)marker; p.mask = (const int*)mask; p.r = (int*)r;
  p.flags_a = (int*)ws; p.flags_b = (int*)((unsigned char*)ws + l.flag_bytes);
  p.h = h; p.N = l.N; p.chunks = (l.N + RC_CHUNK - 1) / RC_CHUNK; p.ntiles = l.ntiles;
  const bool wide = (((uintptr_t)marker | (uintptr_t)mask | (uintptr_t)r) & 15) == 0;
  void (*kernel[2][2])(RecInitParams) = {{rec_init_kernel<0, 1>, rec_init_kernel<0, 4>}, {rec_init_kernel<1, 1>, rec_init_kernel<1, 4>}};
  hipLaunchKernelGGL(kernel[erosion][wide], dim3(volume_grid(p.chunks, RC_MAX_GRID)), dim3(RC_THREADS), 0, (hipStream_t)stream, p);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_rec_relax(void* r, const void* mask, int Z, int Y, int X, int connectivity, int erosion, int rounds, void* changed, void* ws,
                    long long ws_bytes, void* stream) {
  IUNET_REQUIRE(r && mask && changed && ws, "rec_relax: null pointer (r, mask, changed, ws)");
  REC_REQUIRE_VOLUME("rec_relax", Z, Y, X);
  IUNET_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, "rec_relax: connectivity %d: 6, 18 or 26", connectivity);
  IUNET_REQUIRE(erosion == 0 || erosion == 1, "rec_relax: erosion %d: 0 (by dilation) or 1", erosion);
  IUNET_REQUIRE(rounds >= 1 && rounds <= RC_MAX_ROUNDS, "rec_relax: %d rounds outside 1..%d", rounds, RC_MAX_ROUNDS);
  REC_REQUIRE_WS("rec_relax", ws, ws_bytes, Z, Y, X);
  IUNET_REQUIRE((((uintptr_t)r | (uintptr_t)mask | (uintptr_t)changed) & 3) == 0, "rec_relax: r, mask and changed must be 4-byte aligned");
  const RecLayout l = rec_layout(Z, Y, X);
  IUNET_REQUIRE(rec_apart(r, 4 * l.N, mask, 4 * l.N) && rec_apart(r, 4 * l.N, ws, 2 * l.flag_bytes) && rec_apart(changed, 4, ws, 2 * l.flag_bytes) &&
                rec_apart(changed, 4, r, 4 * l.N),
                "rec_relax: r may overlap neither mask nor the workspace, changed neither r nor the workspace");
  hipStream_t st = (hipStream_t)stream;
  int* flags[2] = {(int*)ws, (int*)((unsigned char*)ws + l.flag_bytes)};
  RecRelaxParams p;
  p.r = (int*)r; p.mask = (const int*)mask; p.Z = Z; p.Y = Y; p.X = X; p.ntz = l.ntz; p.nty = l.nty; p.ntx = l.ntx; p.ntiles = l.ntiles;
  void (*kernels[3][2])(RecRelaxParams) = {{rec_relax_kernel<1, 0>, rec_relax_kernel<1, 1>}, {rec_relax_kernel<2, 0>, rec_relax_kernel<2, 1>},
                                           {rec_relax_kernel<3, 0>, rec_relax_kernel<3, 1>}};
  void (*kernel)(RecRelaxParams) = kernels[connectivity == 6 ? 0 : connectivity == 18 ? 1 : 2][erosion];
  IUNET_CHECK_HIP(hipMemsetAsync(changed, 0, 4, st));
  for (int k = 0; k < rounds; ++k) {
    p.flags_in = flags[k & 1]; p.flags_out = flags[(k + 1) & 1];
    p.count = k == rounds - 1 ? (int*)changed : nullptr;
    hipLaunchKernelGGL(kernel, dim3(volume_grid(l.ntiles, RC_MAX_GRID)), dim3(RC_THREADS), 0, st, p);
    IUNET_CHECK_HIP(hipGetLastError());
  }
  // both arrays leave with the last round's flags: the next call starts from the first again
  IUNET_CHECK_HIP(hipMemcpyAsync(flags[(rounds + 1) & 1], flags[rounds & 1], (size_t)(4 * l.ntiles), hipMemcpyDeviceToDevice, st));
  return IUNET_OK;
}

int iunet_rec_select(const void* a, const void* b, int Z, int Y, int X, int t, int value, void* out, void* stream) {
  IUNET_REQUIRE(a && b && out, "rec_select: null pointer (a, b, out)");
  REC_REQUIRE_VOLUME("rec_select", Z, Y, X);
  IUNET_REQUIRE(value >= 0 && value <= 255, "rec_select: value %d outside 0..255", value);
  IUNET_REQUIRE((((uintptr_t)a | (uintptr_t)b) & 3) == 0, "rec_select: a and b must be 4-byte aligned");
  const long long N = (long long)Z * Y * X, chunks = (N + RC_CHUNK - 1) / RC_CHUNK;
  IUNET_REQUIRE(rec_apart(out, N, a, 4 * N) && rec_apart(out, N, b, 4 * N), "rec_select: out may overlap neither a nor b");
  const bool wide = (((uintptr_t)a | (uintptr_t)b) & 15) == 0 && ((uintptr_t)out & 3) == 0;
  hipLaunchKernelGGL(wide ? rec_select_kernel<4> : rec_select_kernel<1>, dim3(volume_grid(chunks, RC_MAX_GRID)), dim3(RC_THREADS), 0,
                     (hipStream_t)stream, (const int*)a, (const int*)b, t, value, (unsigned char*)out, N, chunks);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

}  // extern "C"
