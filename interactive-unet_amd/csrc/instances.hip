// Instance labels from the nearest-seed feature transform of a resident volume (defined bit for bit by
// tests/instances_ref.py): the two streaming passes that follow iunet_edt_feature / iunet_edt_feature_mask (morphology.hip).
//
//   assign_kernel   out[v] = the label of v's nearest seed, seed_labels[idx[v]], where that seed is within r2 (and, with a group map, lies in
//                   v's own group); else 0 (or offset + group[v]: the remainder of v's group).  Reads idx, d2 (and group) and writes out in
//                   order; the two gathers through idx, seed_labels[idx[v]] and group[idx[v]], are data-dependent 4-byte reads.
//   remap_kernel    labels[v] = map[labels[v]] in place; a label outside 0 .. K stays.
//
// Both in the manner of volume_select_kernel (volume_rules.h): a workgroup takes IN_CHUNK voxels at a time (a trip count fixed at launch),
// a thread four per step with 16-byte accesses where every map is 16-byte aligned, else one; the last voxels of a volume that is no
// multiple of 4 go one by one.  One owner per element, no atomics, 64-bit linear indices: the same bits on every launch.
#include "common.h"
#include "volume_rules.h"
#include <cstdint>

namespace {

constexpr int IN_THREADS = 256;
constexpr int IN_CHUNK = 4096;                                      // voxels of one workgroup's step: <= 2^19 chunks
constexpr long long IN_MAX_GRID = 1ll << 20;
constexpr long long IN_MAX_VOX = 0x7fffffffll;
constexpr long long IN_MAX_SQ = 0x7ffffffell;                       // the largest finite squared distance: 2^31 - 2

struct AssignParams {
  const int *idx, *d2, *seed_labels, *group;
  int* out;
  int offset, r2;
  long long N, chunks;
};

// G: with a group map
template <bool G>
__device__ __forceinline__ int assign_one(const AssignParams& p, int i, int d, int g) {
  if (G && g == 0) return 0;
  const bool reached = i >= 0 && i < p.N && d <= p.r2;               // an idx outside the volume is no seed: nothing is read through it
  if (!G) return reached ? p.seed_labels[i] : 0;
  return (reached && p.group[i] == g) ? p.seed_labels[i] : p.offset + g;
}

template <int V, bool G>
__global__ __launch_bounds__(IN_THREADS) void assign_kernel(AssignParams p) {
  for (long long chunk = blockIdx.x; chunk < p.chunks; chunk += gridDim.x) {      // trip count fixed at launch
    for (int s = 0; s < IN_CHUNK / IN_THREADS / V; ++s) {
      const long long v = chunk * IN_CHUNK + ((long long)s * IN_THREADS + threadIdx.x) * V;
      if (v >= p.N) break;
      if (V == 4 && v + 4 <= p.N) {
        const int4 i = *(const int4*)(p.idx + v), d = *(const int4*)(p.d2 + v);
        int4 g = make_int4(0, 0, 0, 0);
        if (G) g = *(const int4*)(p.group + v);
        int4 o;
        o.x = assign_one<G>(p, i.x, d.x, g.x); o.y = assign_one<G>(p, i.y, d.y, g.y);
        o.z = assign_one<G>(p, i.z, d.z, g.z); o.w = assign_one<G>(p, i.w, d.w, g.w);
        *(int4*)(p.out + v) = o;
      } else {
        for (int j = 0; j < V && v + j < p.N; ++j) p.out[v + j] = assign_one<G>(p, p.idx[v + j], p.d2[v + j], G ? p.group[v + j] : 0);
      }
    }
  }
}

__device__ __forceinline__ int remap_one(const int* map, int K, int l) { return (l >= 0 && l <= K) ? map[l] : l; }

template <int V>
__global__ __launch_bounds__(IN_THREADS) void remap_kernel(int* labels, const int* map, int K, long long N, long long chunks) {
  for (long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {        // trip count fixed at launch
    for (int s = 0; s < IN_CHUNK / IN_THREADS / V; ++s) {
      const long long v = chunk * IN_CHUNK + ((long long)s * IN_THREADS + threadIdx.x) * V;
      if (v >= N) break;
      if (V == 4 && v + 4 <= N) {
        int4 l = *(const int4*)(labels + v);
        l.x = remap_one(map, K, l.x); l.y = remap_one(map, K, l.y); l.z = remap_one(map, K, l.z); l.w = remap_one(map, K, l.w);
        *(int4*)(labels + v) = l;
      } else {
        for (int j = 0; j < V && v + j < N; ++j) labels[v + j] = remap_one(map, K, labels[v + j]);
      }
    }
  }
}

inline bool in_apart(const void* a, const void* b, long long N) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, len = 4 * (uintptr_t)N;
  return x + len <= y || y + len <= x;
}

}  // namespace

extern "C" {

int iunet_edt_assign(const void* idx, const void* d2, const void* seed_labels, const void* group, int offset,
                     int Z, int Y, int X, int r2, void* out, void* stream) {
  IUNET_REQUIRE(idx && d2 && seed_labels && out, "edt_assign: null pointer (idx, d2, seed_labels, out)");
  VOLUME_REQUIRE_DIMS("edt_assign", Z, Y, X);
  IUNET_REQUIRE(volume_ok(Z, Y, X, IN_MAX_VOX), "edt_assign: volume %d x %d x %d: more than 2^31 - 1 voxels", Z, Y, X);
  IUNET_REQUIRE(r2 >= 0 && r2 <= IN_MAX_SQ, "edt_assign: bound r2 %d outside 0..2^31 - 2", r2);
  IUNET_REQUIRE(offset >= 0, "edt_assign: offset %d below 0", offset);
  IUNET_REQUIRE((((uintptr_t)idx | (uintptr_t)d2 | (uintptr_t)seed_labels | (uintptr_t)group | (uintptr_t)out) & 3) == 0,
                "edt_assign: idx, d2, seed_labels, group and out must be 4-byte aligned");
  const long long N = (long long)Z * Y * X;
  IUNET_REQUIRE(in_apart(out, idx, N) && in_apart(out, seed_labels, N) && (!group || in_apart(out, group, N)),
                "edt_assign: out may overlap none of idx, seed_labels and group");
  AssignParams p;
  p.idx = (const int*)idx; p.d2 = (const int*)d2; p.seed_labels = (const int*)seed_labels; p.group = (const int*)group; p.out = (int*)out;
  p.offset = offset; p.r2 = r2; p.N = N; p.chunks = (N + IN_CHUNK - 1) / IN_CHUNK;
  const bool wide = (((uintptr_t)idx | (uintptr_t)d2 | (uintptr_t)group | (uintptr_t)out) & 15) == 0;
  void (*kernel)(AssignParams) = group ? (wide ? assign_kernel<4, true> : assign_kernel<1, true>)
                                       : (wide ? assign_kernel<4, false> : assign_kernel<1, false>);
  hipLaunchKernelGGL(kernel, dim3(volume_grid(p.chunks, IN_MAX_GRID)), dim3(IN_THREADS), 0, (hipStream_t)stream, p);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

int iunet_label_remap(void* labels, int Z, int Y, int X, int K, const void* map, void* stream) {
  IUNET_REQUIRE(labels && map, "label_remap: null pointer (labels, map)");
  VOLUME_REQUIRE_DIMS("label_remap", Z, Y, X);
  IUNET_REQUIRE(volume_ok(Z, Y, X, IN_MAX_VOX), "label_remap: volume %d x %d x %d: more than 2^31 - 1 voxels", Z, Y, X);
  IUNET_REQUIRE(K >= 0, "label_remap: %d labels below 0", K);
  IUNET_REQUIRE((((uintptr_t)labels | (uintptr_t)map) & 3) == 0, "label_remap: labels and map must be 4-byte aligned");
  const long long N = (long long)Z * Y * X, chunks = (N + IN_CHUNK - 1) / IN_CHUNK;
  const bool wide = ((uintptr_t)labels & 15) == 0;
  hipLaunchKernelGGL(wide ? remap_kernel<4> : remap_kernel<1>, dim3(volume_grid(chunks, IN_MAX_GRID)), dim3(IN_THREADS), 0,
                     (hipStream_t)stream, (int*)labels, (const int*)map, K, N, chunks);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

}  // extern "C"
