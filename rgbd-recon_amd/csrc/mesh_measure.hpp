// The arithmetic of the mesh component measures (tsdf_mesh_component_measures; include/rgbd_recon_hip.h has the definition), once, for host and device:
// the measure grid, a vertex's grid coordinate and its packed form, a triangle's doubled area and six-fold signed volume in exact integers, the split of
// the volume for accumulation, and the keep rule.  HIP-free: k_mesh_component_measures.hip compiles it for the device, abi.cpp for the grid, and
// tests/cpp/mesh_measure_main.cpp runs it under the host sanitizers against Python integers (tests/mesh_measure_reference.py is its numpy twin).
// Every file that includes it is compiled with -ffp-contract=off: the three double operations of a coordinate round one by one.
#ifndef RR_MESH_MEASURE_HPP
#define RR_MESH_MEASURE_HPP
#include <cmath>
#include <cstdint>

#include "../../include/rgbd_recon_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RR_MEASURE_HD __host__ __device__ inline
#else
#define RR_MEASURE_HD inline
#endif

namespace rr {

constexpr uint32_t kMeasureBits = 20u, kMeasureMax = 1u << kMeasureBits;   // a coordinate lies in [0, 2^20]: 21 bits
typedef unsigned __int128 measure_u128;
typedef __int128 measure_i128;
static_assert(sizeof(tsdf_mesh_component_measure) == 80 && sizeof(tsdf_mesh_measure_grid) == 24 && sizeof(tsdf_mesh_measure_rule) == 32, "the records' sizes");

// ---- the grid: isotropic, 2^20 units along the box's longest edge.  ext as vol_to_world forms it (fp32), one double division on the host.
struct MeasureScale { double scale, unit; float bbox_min[3]; };
inline bool measure_scale(const float bbox_min[3], const float bbox_max[3], MeasureScale* S) {
  float e = 0.0f;
  for (int a = 0; a < 3; ++a) { const float ext = bbox_max[a] - bbox_min[a]; if (a == 0 || ext > e) e = ext; S->bbox_min[a] = bbox_min[a]; }
  if (!(e > 0.0f) || !std::isfinite(e)) return false;
  S->scale = 1048576.0 / (double)e;
  S->unit = 1.0 / S->scale;
  return true;
}

// ---- a vertex: q = rint((p - bbox_min) * scale) in double, half-way cases to even, clamped to [0, 2^20]; NaN gives 0
RR_MEASURE_HD uint32_t measure_quantise(float p, float bbox_min, double scale) {
  const double d = (double)p - (double)bbox_min;
  const double r = rint(d * scale);
  if (!(r > 0.0)) return 0u;                                             // (NaN too)
  return r >= (double)kMeasureMax ? kMeasureMax : (uint32_t)r;
}
RR_MEASURE_HD uint64_t measure_pack(uint32_t qx, uint32_t qy, uint32_t qz) { return (uint64_t)qx | (uint64_t)qy << 21 | (uint64_t)qz << 42; }
RR_MEASURE_HD void measure_unpack(uint64_t w, int64_t q[3]) {
  q[0] = (int64_t)(w & 0x1fffffu); q[1] = (int64_t)(w >> 21 & 0x1fffffu); q[2] = (int64_t)(w >> 42 & 0x1fffffu);
}

// ---- a triangle.  e1, e2: each component within +-2^20; c = e1 x e2: within +-2^41; n2 = c . c < 2^84: two 64-bit limbs
RR_MEASURE_HD void measure_cross(const int64_t a[3], const int64_t b[3], int64_t c[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
RR_MEASURE_HD measure_u128 measure_n2(const int64_t c[3]) {
  measure_u128 n = 0;
  for (int a = 0; a < 3; ++a) { const uint64_t m = (uint64_t)(c[a] < 0 ? -c[a] : c[a]); n += (measure_u128)m * m; }
  return n;
}
// floor(sqrt(n)) for n < 2^88: a double estimate (never trusted: it is off by one where n is near a square), corrected by exact comparisons
RR_MEASURE_HD uint64_t measure_isqrt(measure_u128 n) {
  const double d = (double)(uint64_t)(n >> 64) * 18446744073709551616.0 + (double)(uint64_t)n;
  uint64_t r = (uint64_t)sqrt(d);
  while ((measure_u128)r * r > n) --r;
  while ((measure_u128)(r + 1) * (r + 1) <= n) ++r;
  return r;
}
// det(q0, q1, q2): q1 x q2 lies within +-2^40 a component, each of the three products within +-2^60, their sum within +-3 * 2^60: no overflow
RR_MEASURE_HD int64_t measure_det(const int64_t q0[3], const int64_t q1[3], const int64_t q2[3]) {
  int64_t c[3];
  measure_cross(q1, q2, c);
  return q0[0] * c[0] + q0[1] * c[1] + q0[2] * c[2];
}
struct MeasureTriangle { uint64_t a2; int64_t v6; };
RR_MEASURE_HD MeasureTriangle measure_triangle(uint64_t w0, uint64_t w1, uint64_t w2) {
  int64_t q0[3], q1[3], q2[3], e1[3], e2[3], c[3];
  measure_unpack(w0, q0); measure_unpack(w1, q1); measure_unpack(w2, q2);
  for (int a = 0; a < 3; ++a) { e1[a] = q1[a] - q0[a]; e2[a] = q2[a] - q0[a]; }
  measure_cross(e1, e2, c);
  return MeasureTriangle{measure_isqrt(measure_n2(c)), measure_det(q0, q1, q2)};
}

// ---- the sum of v6 over up to 2^32 triangles: the low 32 bits (unsigned) and the rest (arithmetic shift) are summed apart, each far inside 64 bits,
// and sum v6 = hi * 2^32 + lo exactly; the canonical form is one two's-complement 128-bit integer
RR_MEASURE_HD uint64_t measure_v6_lo(int64_t v6) { return (uint64_t)(uint32_t)v6; }
RR_MEASURE_HD int64_t measure_v6_hi(int64_t v6) { return (v6 - (int64_t)(uint32_t)v6) / 4294967296ll; }   // (= v6 >> 32, without shifting a negative)
RR_MEASURE_HD void measure_v6_join(uint64_t lo_sum, int64_t hi_sum, uint64_t* volume6_lo, int64_t* volume6_hi) {
  const measure_i128 t = (measure_i128)hi_sum * 4294967296ll + (measure_i128)lo_sum;
  const measure_u128 u = (measure_u128)t;
  *volume6_lo = (uint64_t)u;
  *volume6_hi = (int64_t)(uint64_t)(u >> 64);
}

// ---- the keep rule of tsdf_mesh_filter_components_measured: every clause has to hold
RR_MEASURE_HD bool measure_keeps(const tsdf_mesh_component_measure& m, uint32_t n_triangles, const tsdf_mesh_measure_rule& r) {
  uint32_t extent = 0;
  for (int a = 0; a < 3; ++a) { const uint32_t e = m.q_max[a] - m.q_min[a]; if (e > extent) extent = e; }
  const bool negative = m.volume6_hi < 0;
  measure_u128 mag = (measure_u128)(uint64_t)m.volume6_hi << 64 | m.volume6_lo;
  if (negative) mag = (measure_u128)0 - mag;
  const bool positive = !negative && mag != 0;
  return n_triangles >= r.min_triangles && extent >= r.min_extent && m.area2 >= r.min_area2 && mag >= (measure_u128)r.min_abs_volume6 &&
         (!(r.flags & TSDF_MESH_RULE_POSITIVE_VOLUME) || positive);
}

}  // namespace rr
#endif
