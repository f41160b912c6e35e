// The view ray of a pixel in the volume's unit cube: one text for the draw's march kernels (k_raymarch.hip) and for tsdf_view_rays
// (k_rays.hip), so a ray handed to the caller and the ray the draw marches are the same bits.  And which slab owns a sample: one text for the draw's
// slab march (k_march, kPartial) and the ray queries' part form (k_rays_march, kPart), so a pixel's ray and a caller's ray are split over slabs alike.
// And tsdf_raymarch.fs' leaf functions -- step, cube test, start, hit refinement -- once each for k_march, k_march_box, march_long and k_rays_march.
#ifndef RR_RAY_DEV_HPP
#define RR_RAY_DEV_HPP
#include "sampling.hpp"

namespace rr {

// Unnormalised volume-space direction of the ray through pixel centre (fx, fy)
__device__ __forceinline__ float3 pixel_dir_vol(const ViewParams& P, float fx, float fy) {
  const float4 p = mat_mul(P.img_to_eye, fx, fy, 1.0f, 1.0f);
  const float4 wd = mat_mul(P.mv_inv, p.x / p.w, p.y / p.w, p.z / p.w, 0.0f);
  const float4 vd = mat_mul(P.v2w_inv, wd.x, wd.y, wd.z, wd.w);
  return make_float3(vd.x, vd.y, vd.z);
}
// sampleStep = normalize(direction) * sampleDistance, tsdf_raymarch.fs:64
__device__ __forceinline__ float3 ray_step(float3 dir, float sd) {
  const float3 dn = normalize3(dir);
  return make_float3(dn.x * sd, dn.y * sd, dn.z * sd);
}
// ... of the ray through the centre of pixel (px, py)
__device__ __forceinline__ float3 pixel_step(const ViewParams& P, int px, int py, float sd) { return ray_step(pixel_dir_vol(P, (float)px + 0.5f, (float)py + 0.5f), sd); }
// `pos += sampleStep`, :108: every sample position is reached by a chain of these, never by a multiple of the step
__device__ __forceinline__ float3 ray_advance(float3 p, float3 step) { return make_float3(p.x + step.x, p.y + step.y, p.z + step.z); }

// intersectBox(), :363-374, of the unit cube with the ray o + t * step: the span [t0, t1] in steps, and whether there is one in front of the origin
// (a NaN in either bound is a miss)
struct CubeSpan { float t0, t1; bool hit; };
__device__ __forceinline__ CubeSpan unit_cube_span(float3 o, float3 step) {
  const float3 inv = make_float3(1.0f / step.x, 1.0f / step.y, 1.0f / step.z);
  const float3 tbot = make_float3(inv.x * (0.0f - o.x), inv.y * (0.0f - o.y), inv.z * (0.0f - o.z));
  const float3 ttop = make_float3(inv.x * (1.0f - o.x), inv.y * (1.0f - o.y), inv.z * (1.0f - o.z));
  const float3 tmn = make_float3(fminf(ttop.x, tbot.x), fminf(ttop.y, tbot.y), fminf(ttop.z, tbot.z));
  const float3 tmx = make_float3(fmaxf(ttop.x, tbot.x), fmaxf(ttop.y, tbot.y), fmaxf(ttop.z, tbot.z));
  const float t0 = fmaxf(fmaxf(tmn.x, tmn.y), fmaxf(tmn.x, tmn.z));
  const float t1 = fminf(fminf(tmx.x, tmx.y), fminf(tmx.x, tmx.z));
  return CubeSpan{t0, t1, t0 <= t1 && !(t1 < 0.0f)};
}
// The march without skipSpace, :75-86: it starts where the ray enters the cube, or at the origin inside it ...
__device__ __forceinline__ float span_near(float t0) { return t0 < 0.0f ? 0.0f : t0; }
// ... at this position, and takes this many samples to t1 (a float: the caller caps and converts it)
__device__ __forceinline__ float3 ray_at(float3 o, float3 step, float t) { return make_float3(o.x + step.x * t, o.y + step.y * t, o.z + step.z * t); }
__device__ __forceinline__ float span_samples(float t_near, float t1) { return ceilf(fabsf(t1 - t_near)); }

// approximate ray-cell intersection, :99-101: from the first sample with a positive density (hit_pos, hit_d) back towards the one before it (prev)
__device__ __forceinline__ float3 refine_hit(float3 hit_pos, float3 step, float prev, float hit_d) {
  const float kk = prev / (hit_d - prev);
  return make_float3((hit_pos.x - step.x) - step.x * kk, (hit_pos.y - step.y) - step.y * kk, (hit_pos.z - step.z) - step.z * kk);
}

// Which slab owns a sample (multi-GPU): the voxel plane floor(pos.z * rz), clamped (fmaxf drops a NaN: plane 0; +-inf clamp).
__device__ __forceinline__ bool sample_owned(const Volume& V, float pz) {
  const float f = fminf(fmaxf(floorf(pz * (float)V.res[2]), 0.0f), (float)(V.res[2] - 1));
  const int tz = ((int)f) >> 3;
  return tz >= V.own_tz0 && tz < V.own_tz1;
}

}  // namespace rr
#endif
