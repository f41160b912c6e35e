// The view ray of a pixel in the volume's unit cube: one text for the draw's march kernels (k_raymarch.hip) and for tsdf_view_rays
// (k_rays.hip), so a ray handed to the caller and the ray the draw marches are the same bits.  And which slab owns a sample: one text for the draw's
// slab march (k_march, kPartial) and the ray queries' part form (k_rays_march, kPart), so a pixel's ray and a caller's ray are split over slabs alike.
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

// Which slab owns a sample (multi-GPU): the voxel plane floor(pos.z * rz), clamped (fmaxf drops a NaN: plane 0; +-inf clamp).
__device__ __forceinline__ bool sample_owned(const Volume& V, float pz) {
  const float f = fminf(fmaxf(floorf(pz * (float)V.res[2]), 0.0f), (float)(V.res[2] - 1));
  const int tz = ((int)f) >> 3;
  return tz >= V.own_tz0 && tz < V.own_tz1;
}

}  // namespace rr
#endif
