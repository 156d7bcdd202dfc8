// Oblique slab around the slicer's plane: the input of the 3-D net's interactive prediction, and the way its result goes back
// into a resident predicted volume (defined bit for bit by tests/slab_ref.py).
//
// Gather.  Sample (k, i, j) of the uint8 [T][sw][sw] slab lies at c = ((a * r_i + b * r_j) + n * r_k) + o per axis, r_i = start + i,
// r_j = start + j, r_k = start_k + k (slab_point, volume_rules.h) -- at r_k = 0 the plane of Slicer.get_interpolation_coords.  It is
// sampled from the WHOLE volume by the rules slice_gather_kernel (slicer.hip) applies to its crop (coord_inside, coord_nearest,
// volume_sample_linear), i.e. as scipy.ndimage.map_coordinates(mode='constant', cval=0) does for spline orders 0 and 1.
// Paste. The adjoint direction as a gather over the voxels of a host-given box (no holes, no atomics): voxel p has the slab
// coordinates t_v = (d_0 v_0 + d_1 v_1) + d_2 v_2, d = p - o, for v in (n, a, b); its sample is the nearest one (ties to even), and it
// is written iff that sample lies in the kept planes and inside the border.  The fp32 probabilities are quantised on the way to the
// bytes iunet_normalize_quantize gives at weight 1.
// Both are HBM-bound: one lane per output element, 64 consecutive lanes on 64 consecutive j (gather) / x (paste), 4 rows per workgroup.
#include "common.h"
#include "volume_rules.h"

namespace {

struct SlabGeom {
  double a[3], b[3], n[3], o[3];
};

struct SlabGatherParams {
  const unsigned char* vol;
  int dim[3];
  SlabGeom g;
  int sw, start, start_k, order;
  unsigned char* out;
};

struct SlabPasteParams {
  unsigned char* vol;
  int Y, X, C;
  SlabGeom g;
  int lo[3], len[3];
  const float* probs;
  int sw, start, start_k, k_lo, k_hi, border;
};

__global__ __launch_bounds__(256) void slab_gather_kernel(SlabGatherParams p) {
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), i = blockIdx.y * 4 + (threadIdx.x >> 6), k = blockIdx.z;
  if (i >= p.sw || j >= p.sw) return;
  const double ri = (double)(p.start + i), rj = (double)(p.start + j), rk = (double)(p.start_k + k);
  double c[3];
  bool inside = true;
#pragma unroll
  for (int x = 0; x < 3; ++x) {
    c[x] = slab_point(p.g.a[x], p.g.b[x], p.g.n[x], p.g.o[x], ri, rj, rk);
    inside = inside && coord_inside(c[x], p.dim[x]);
  }
  unsigned char res = 0;
  if (inside) {
    const long long sy = p.dim[2], sz = (long long)p.dim[1] * p.dim[2];
    if (p.order == 0) {
      const long long z = (long long)coord_nearest(c[0]), y = (long long)coord_nearest(c[1]), x = (long long)coord_nearest(c[2]);
      res = p.vol[z * sz + y * sy + x];
    } else {
      res = volume_sample_linear(p.vol, p.dim, sy, sz, c);
    }
  }
  p.out[((long long)k * p.sw + i) * p.sw + j] = res;
}

// rint((d_0 v_0 + d_1 v_1) + d_2 v_2): the index of the nearest sample along v (np.rint: half to even)
__device__ __forceinline__ double slab_nearest(double d0, double d1, double d2, const double (&v)[3]) {
#pragma clang fp contract(off)
  const double t0 = d0 * v[0], t1 = d1 * v[1], t2 = d2 * v[2];
  const double s = t0 + t1;
  return rint(s + t2);
}

__global__ __launch_bounds__(256) void slab_paste_kernel(SlabPasteParams p) {
#pragma clang fp contract(off)
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), z = blockIdx.z;
  if (x >= p.len[2] || y >= p.len[1]) return;
  const int vz = p.lo[0] + z, vy = p.lo[1] + y, vx = p.lo[2] + x;
  const double d0 = (double)vz - p.g.o[0], d1 = (double)vy - p.g.o[1], d2 = (double)vx - p.g.o[2];
  // compared as doubles: an rint result is integral, and its difference to an int is exact
  const double k = slab_nearest(d0, d1, d2, p.g.n) - (double)p.start_k, i = slab_nearest(d0, d1, d2, p.g.a) - (double)p.start,
               j = slab_nearest(d0, d1, d2, p.g.b) - (double)p.start;
  const double b_lo = (double)p.border, b_hi = (double)(p.sw - p.border);
  if (!(k >= (double)p.k_lo && k < (double)p.k_hi && i >= b_lo && i < b_hi && j >= b_lo && j < b_hi)) return;
  const float* src = p.probs + (((long long)k * p.sw + (long long)i) * p.sw + (long long)j) * p.C;
  unsigned char* dst = p.vol + (((long long)vz * p.Y + vy) * p.X + vx) * p.C;
  for (int c = 0; c < p.C; ++c) {
    const float q = __fdiv_rn(__fmul_rn(255.0f, src[c]), 1.0f);   // predict.hip: normalize_quantize_kernel at weight 1
    dst[c] = (unsigned char)(int)q;
  }
}

void slab_geom(SlabGeom& g, const double* geom) {
  for (int x = 0; x < 3; ++x) { g.a[x] = geom[x]; g.b[x] = geom[3 + x]; g.n[x] = geom[6 + x]; g.o[x] = geom[9 + x]; }
}

}  // namespace

extern "C" {

// vol: uint8 [Z][Y][X] on the device; geom: 12 host doubles (a[3], b[3], n[3], origin[3]); out: uint8 [T][sw][sw] on the device.
int iunet_slab_gather(const void* vol, int Z, int Y, int X, const double* geom, int T, int sw, int start, int start_k, int order,
                      void* out, void* stream) {
  IUNET_REQUIRE(vol && geom && out, "slab_gather: null pointer");
  IUNET_REQUIRE(order == 0 || order == 1, "slab_gather: spline order must be 0 or 1 (got %d)", order);
  IUNET_REQUIRE(T >= 1 && sw >= 1, "slab_gather: bad slab %d x %d x %d", T, sw, sw);
  IUNET_REQUIRE(T <= 65535 && (sw + 3) / 4 <= 65535, "slab_gather: slab %d x %d x %d exceeds the grid (65535 planes, 262140 rows)", T, sw, sw);
  IUNET_REQUIRE(volume_ok(Z, Y, X, VOLUME_MAX_SAMPLED), "slab_gather: volume %d x %d x %d", Z, Y, X);
  SlabGatherParams p;
  p.vol = (const unsigned char*)vol; p.dim[0] = Z; p.dim[1] = Y; p.dim[2] = X;
  slab_geom(p.g, geom);
  p.sw = sw; p.start = start; p.start_k = start_k; p.order = order; p.out = (unsigned char*)out;
  hipLaunchKernelGGL(slab_gather_kernel, dim3((sw + 63) / 64, (sw + 3) / 4, T), dim3(256), 0, (hipStream_t)stream, p);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

// vol: uint8 [Z][Y][X][C] on the device; geom as above; lo / len: the box of voxels to visit (host ints, 0 <= lo, lo + len <= shape);
// probs: fp32 [T][sw][sw][C] on the device.
int iunet_slab_paste(void* vol, int Z, int Y, int X, int C, const double* geom, const int* lo, const int* len, const void* probs,
                     int T, int sw, int start, int start_k, int k_lo, int k_hi, int border, void* stream) {
  IUNET_REQUIRE(vol && geom && lo && len && probs, "slab_paste: null pointer");
  IUNET_REQUIRE(T >= 1 && sw >= 1, "slab_paste: bad slab %d x %d x %d", T, sw, sw);
  IUNET_REQUIRE(C >= 1 && C <= 16, "slab_paste: %d classes outside 1..16", C);
  IUNET_REQUIRE(volume_ok(Z, Y, X, VOLUME_MAX_SAMPLED), "slab_paste: volume %d x %d x %d", Z, Y, X);
  IUNET_REQUIRE(k_lo >= 0 && k_hi <= T && k_hi > k_lo, "slab_paste: empty or outlying plane range [%d, %d) of %d planes", k_lo, k_hi, T);
  IUNET_REQUIRE(border >= 0 && 2 * (long long)border < sw, "slab_paste: border %d leaves nothing of %d pixels", border, sw);
  SlabPasteParams p;
  p.vol = (unsigned char*)vol; p.Y = Y; p.X = X; p.C = C;
  slab_geom(p.g, geom);
  const int dims[3] = {Z, Y, X};
  for (int x = 0; x < 3; ++x) {
    IUNET_REQUIRE(lo[x] >= 0 && len[x] >= 0 && (long long)lo[x] + len[x] <= dims[x], "slab_paste: box outside the volume (axis %d)", x);
    p.lo[x] = lo[x]; p.len[x] = len[x];
  }
  IUNET_REQUIRE(len[0] <= 65535 && (len[1] + 3) / 4 <= 65535, "slab_paste: box %d x %d x %d exceeds the grid (65535 planes, 262140 rows)",
                len[0], len[1], len[2]);
  p.probs = (const float*)probs; p.sw = sw; p.start = start; p.start_k = start_k; p.k_lo = k_lo; p.k_hi = k_hi; p.border = border;
  if (len[0] == 0 || len[1] == 0 || len[2] == 0) return IUNET_OK;          // nothing to visit
  hipLaunchKernelGGL(slab_paste_kernel, dim3((len[2] + 63) / 64, (len[1] + 3) / 4, len[0]), dim3(256), 0, (hipStream_t)stream, p);
  IUNET_CHECK_HIP(hipGetLastError());
  return IUNET_OK;
}

}  // extern "C"
