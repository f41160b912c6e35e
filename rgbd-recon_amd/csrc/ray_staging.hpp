// Host bookkeeping of the ray queries (tsdf_cast_rays / tsdf_cast_rays_dev / tsdf_view_rays), free of HIP: which arguments a cast accepts and the two
// numbers the march kernel is launched with; how the staging grows and how a cast is cut into launches is result_paths.hpp's (CallStaging, CallChunks).
// abi.cpp holds the buffers and issues the calls; a stand-alone program (tests/test_ray_staging.py) runs this text under the host sanitizers.
#pragma once
#include <stdint.h>

namespace rr {

constexpr uint32_t kRayFlagUnitCube = 1u, kRayFlagNormals = 2u, kRayFlagColours = 4u;   // TSDF_RAYS_UNIT_CUBE, TSDF_RAY_NORMALS, TSDF_RAY_COLOURS
constexpr uint32_t kRayFlagsAll = kRayFlagUnitCube | kRayFlagNormals | kRayFlagColours;
constexpr uint64_t kRayBytes = 32;               // sizeof(tsdf_ray) == sizeof(tsdf_ray_hit) == sizeof(tsdf_ray_surface)
constexpr uint64_t kRayMaxCount = 1ull << 40;    // rays of one cast: keeps every byte count below 2^46

// 0: the arguments of a cast are acceptable; 1: unknown flag; 2: a NULL ray / hit array with n > 0; 3: `surface` given without an attribute flag, or
// missing with one; 4: more rays than a cast takes
inline int ray_cast_arguments(uint64_t n, uint32_t flags, bool have_rays, bool have_hits, bool have_surface) {
  if (flags & ~kRayFlagsAll) return 1;
  const bool wants = (flags & (kRayFlagNormals | kRayFlagColours)) != 0;
  if (n == 0) return 0;
  if (!have_rays || !have_hits) return 2;
  if (wants != have_surface) return 3;
  if (n > kRayMaxCount) return 4;
  return 0;
}
// The merge of slab parts (tsdf_merge_ray_parts_dev).  0: acceptable; 1: no part; 2: a NULL hit array with n > 0; 3: exactly one of the two surface
// arrays; 4: parts closer together than their n records; 5: more than the entries index (n as a cast's, and parts * stride below 2^48 records)
inline int ray_merge_arguments(uint32_t parts, uint64_t n, uint64_t stride_records, bool have_hit_parts, bool have_hits, bool have_surface_parts, bool have_surface) {
  if (parts == 0) return 1;
  if (n == 0) return 0;
  if (!have_hit_parts || !have_hits) return 2;
  if (have_surface_parts != have_surface) return 3;
  if (stride_records < n) return 4;
  if (n > kRayMaxCount || stride_records > (1ull << 48) / parts) return 5;
  return 0;
}
// 0, or what is wrong with the pixel rectangle of tsdf_view_rays in a view of vw x vh: 1 empty or negative, 2 outside the view
inline int ray_view_rect(int32_t x0, int32_t y0, int32_t w, int32_t h, int32_t vw, int32_t vh) {
  if (w <= 0 || h <= 0 || x0 < 0 || y0 < 0) return 1;
  if ((int64_t)x0 + w > vw || (int64_t)y0 + h > vh) return 2;
  return 0;
}

// Samples per look at the tile classes: the most for which a run's taps span at most two 8-voxel tiles on every axis, whatever the direction.  A step
// moves a ray by at most limit / 2 * res voxels on an axis; (run - 1) steps, one voxel of filter footprint and the fraction must stay within 8.  (The
// kernel tests the span of every run itself and fetches when it is larger: this only sizes the attempt.)
inline int ray_run_length(float limit, const int res[3]) {
  int r = res[0] > res[1] ? res[0] : res[1];
  if (res[2] > r) r = res[2];
  const float per_step = limit * 0.5f * (float)r;
  if (!(per_step > 0.0f)) return 1;
  const float k = 6.0f / per_step;
  return k >= 31.0f ? 32 : (k < 1.0f ? 1 : (int)k + 1);
}
// The bound on a ray's sample count.  Inside the unit cube a ray is at most sqrt(3) long and a step limit / 2: every ray of the definition stays below
// 2 / (limit / 2) + 2 samples.  Only a ray whose origin is so far off that t0 and t1 have lost the box to rounding is cut by it.
inline float ray_sample_cap(float limit) {
  const float c = 4.0f / limit + 2.0f;
  return c > 0.0f && c < 4.0e9f ? c : 4.0e9f;
}

}  // namespace rr
