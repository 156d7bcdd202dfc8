// The rules the resident-volume kernels share, each written once: slicer.hip, slab.hip, propose.hip, components.hip
// and morphology.hip include them; tests/slab_ref.py, propose_ref.py, components_ref.py and morphology_ref.py restate them.  The float
// bodies are each under their own `fp contract(off)` (the pragma is lexical): float64, every product and sum rounded on its own, in the
// order written -- numpy's evaluation, no fma.
#pragma once
#include "common.h"

// a sample's coordinate along one axis: of a plane, c = (a r_i + b r_j) + o; of a slab, c = ((a r_i + b r_j) + n r_k) + o
__device__ __forceinline__ double plane_point(double a, double b, double o, double ri, double rj) {
#pragma clang fp contract(off)
  const double t1 = a * ri, t2 = b * rj;
  return (t1 + t2) + o;
}
__device__ __forceinline__ double slab_point(double a, double b, double n, double o, double ri, double rj, double rk) {
#pragma clang fp contract(off)
  const double t1 = a * ri, t2 = b * rj, t3 = n * rk;
  return ((t1 + t2) + t3) + o;
}

// scipy.ndimage.map_coordinates(mode='constant', cval=0): a coordinate outside [0, dim - 1] gives 0 (no interpolation against the padding)
__device__ __forceinline__ bool coord_inside(double c, int dim) { return c >= 0.0 && c <= (double)(dim - 1); }

// order 0: voxel floor(c + 0.5).  Still a double: integral and, behind coord_inside, in 0 .. dim - 1, so the caller's cast to its index
// type is exact
__device__ __forceinline__ double coord_nearest(double c) {
#pragma clang fp contract(off)
  return floor(c + 0.5);
}

__device__ __forceinline__ int volume_mirror(int idx, int len) {
  if (len <= 1) return 0;
  const int s2 = 2 * len - 2;
  if (idx < 0) { idx = s2 * (-idx / s2) + idx; return idx <= 1 - len ? idx + s2 : -idx; }
  if (idx >= len) { idx -= s2 * (idx / s2); if (idx >= len) idx = s2 - idx; }
  return idx;
}

// order 1: weights w0 = 1 - frac, w1 = 1 - w0, neighbour indices mirrored at the box's edge (weight 0 there), t = sum over (dz, dy, dx) of
// ((v * wz) * wy) * wx in that order, result trunc(t + 0.5) clamped to 255.  base: voxel (0, 0, 0) of the box that is sampled (a crop, or
// the whole volume), len its extents, sy / sz the strides of the volume it lies in, c the coordinates in the box (inside it on every
// axis).  64-bit index arithmetic.
__device__ __forceinline__ unsigned char volume_sample_linear(const unsigned char* base, const int (&len)[3], long long sy, long long sz,
                                                              const double (&c)[3]) {
#pragma clang fp contract(off)
  int st[3];
  double w[3][2];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double f = floor(c[k]);
    st[k] = (int)f;
    const double x = c[k] - f;
    w[k][0] = 1.0 - x;
    w[k][1] = 1.0 - w[k][0];
  }
  double t = 0.0;
#pragma unroll
  for (int dz = 0; dz < 2; ++dz)
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const long long iz = volume_mirror(st[0] + dz, len[0]), iy = volume_mirror(st[1] + dy, len[1]),
                        ix = volume_mirror(st[2] + dx, len[2]);
        double coeff = (double)base[iz * sz + iy * sy + ix];
        coeff = coeff * w[0][dz];
        coeff = coeff * w[1][dy];
        coeff = coeff * w[2][dx];
        t = t + coeff;
      }
  t = t > 0.0 ? t + 0.5 : 0.0;
  t = t > 255.0 ? 255.0 : t;
  return (unsigned char)t;
}

// The class of a voxel of a predicted volume: the index of the first largest byte, and that byte (0: never predicted).
// CT: 1 a class map (C = 1: the byte is the class and counts as predicted, best = 1), 2 two classes, 0 any number
struct TopByte { int at, best; };
template <int CT>
__device__ __forceinline__ TopByte volume_top_byte(const unsigned char* src, long long v, int C) {
  if (CT == 1) return TopByte{src[v], 1};
  const unsigned char* q = src + v * C;              // 64-bit: Z Y X C passes 2^31
  int best = q[0], at = 0;
  const int n = CT == 2 ? 2 : C;
  for (int c = 1; c < n; ++c) {                      // fixed trip count
    const int t = q[c];
    if (t > best) { best = t; at = c; }
  }
  return TopByte{at, best};
}

// The streaming pass of cc_filter and edt_select: out[v] = pick(map[v], cls[v]) over N voxels; out may be cls.  A workgroup takes CHUNK
// voxels (a fixed trip count), a thread V per step: 4 where map, cls and out are aligned for 16- and 4-byte accesses, else 1; the last
// voxels of a volume that is no multiple of 4 go one by one.  Pick: a small trivially-copyable functor, passed by value.
template <int CHUNK, int THREADS, int V, class Pick>
__global__ __launch_bounds__(THREADS) void volume_select_kernel(const int* map, const unsigned char* cls, Pick pick, unsigned char* out,
                                                                long long N) {
  const long long base = (long long)blockIdx.x * CHUNK;
  for (int s = 0; s < CHUNK / THREADS / V; ++s) {
    const long long v = base + ((long long)s * THREADS + threadIdx.x) * V;
    if (v >= N) break;
    if (V == 4 && v + 4 <= N) {
      const int4 m = *(const int4*)(map + v);
      uchar4 c = *(const uchar4*)(cls + v);
      c.x = pick(m.x, c.x); c.y = pick(m.y, c.y); c.z = pick(m.z, c.z); c.w = pick(m.w, c.w);
      *(uchar4*)(out + v) = c;
    } else {
      for (int j = 0; j < V && v + j < N; ++j) out[v + j] = pick(map[v + j], cls[v + j]);
    }
  }
}
template <int CHUNK, int THREADS, class Pick>
inline void volume_select_launch(const void* map, const void* cls, Pick pick, void* out, long long N, hipStream_t stream) {
  static_assert(std::is_trivially_copyable<Pick>::value && CHUNK % (4 * THREADS) == 0, "Pick goes by value; whole steps at V = 4");
  const unsigned int chunks = (unsigned int)((N + CHUNK - 1) / CHUNK);
  const bool wide = ((uintptr_t)map & 15) == 0 && (((uintptr_t)cls | (uintptr_t)out) & 3) == 0;
  if (wide) hipLaunchKernelGGL((volume_select_kernel<CHUNK, THREADS, 4, Pick>), dim3(chunks), dim3(THREADS), 0, stream, (const int*)map,
                               (const unsigned char*)cls, pick, (unsigned char*)out, N);
  else hipLaunchKernelGGL((volume_select_kernel<CHUNK, THREADS, 1, Pick>), dim3(chunks), dim3(THREADS), 0, stream, (const int*)map,
                          (const unsigned char*)cls, pick, (unsigned char*)out, N);
}

// ---- host ----
// the voxels of a volume the gathers, the scatter and the scores accept: below 2^42 (the scatter's table keys a voxel in 43 bits)
constexpr long long VOLUME_MAX_SAMPLED = (1ll << 42) - 1;
inline long long volume_align16(long long n) { return (n + 15) & ~15ll; }
// every dimension at least 1 and at most max_voxels voxels (the product is not formed: it may pass 2^63)
inline bool volume_ok(int Z, int Y, int X, long long max_voxels) { return Z > 0 && Y > 0 && X > 0 && (long long)Z * Y <= max_voxels / X; }
// more groups than cap: a workgroup takes several (a trip count fixed at launch)
inline unsigned int volume_grid(long long groups, long long cap) { return (unsigned int)(groups < cap ? groups : cap); }
#define VOLUME_REQUIRE_DIMS(who, Z, Y, X) IUNET_REQUIRE(Z > 0 && Y > 0 && X > 0, who ": volume %d x %d x %d: a dimension below 1", Z, Y, X)
