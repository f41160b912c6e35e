// blendColors() (tsdf_raymarch.fs:295-330), shared by the raymarch's shading (k_raymarch.hip) and the mesh extraction's vertex
// colours (k_mesh.hip): one definition, so a mesh vertex and a frame pixel at the same volume position get the same bits.
#ifndef RR_BLEND_DEV_HPP
#define RR_BLEND_DEV_HPP
#include "shading_dev.hpp"

namespace rr {

// blendColors(), tsdf_raymarch.fs:295-330.  Streams are taken kShadeChunk at a time: the inverse-LUT taps of the whole chunk are
// issued together, then the colour-LUT taps, then the image footprints; the accumulation itself stays in stream order.
#ifndef RR_SHADE_CHUNK
#define RR_SHADE_CHUNK 4
#endif
constexpr int kShadeChunk = RR_SHADE_CHUNK;   // streams whose taps are in flight together
__device__ float4 blend_colors(const StreamTable& T, const FrameImages& F, float limit, float3 sp) {
  float3 tc = make_float3(0, 0, 0), tc2 = make_float3(0, 0, 0);
  float tw = 0.0f, tw2 = 0.0f;
  for (int cb = 0; cb < T.n; cb += kShadeChunk) {
    const int nc = min(kShadeChunk, T.n - cb);
    float3 pc[kShadeChunk], col[kShadeChunk];
    float2 pcol[kShadeChunk];
    Dqs q[kShadeChunk];
#pragma unroll
    for (int c = 0; c < kShadeChunk; ++c)
      if (c < nc) pc[c] = tex3d_rgba_xyz(T.s[cb + c].inv, T.s[cb + c].inv_res, sp.x, sp.y, sp.z);
#pragma unroll
    for (int c = 0; c < kShadeChunk; ++c)
      if (c < nc) pcol[c] = tex3d_rg(T.s[cb + c].uv, T.s[cb + c].uv_res, pc[c].x, pc[c].y, pc[c].z);
#pragma unroll
    for (int c = 0; c < kShadeChunk; ++c)
      if (c < nc) { col[c] = color_bilinear(F, cb + c, pcol[c].x, pcol[c].y); q[c] = dqs_fetch(F, cb + c, pc[c].x, pc[c].y); }
#pragma unroll
    for (int c = 0; c < kShadeChunk; ++c)
      if (c < nc) {
        const float dist = fabsf(dqs_depth(q[c]) - pc[c].z);
        float quality = 0.0f;
        if (dist < limit) quality = dqs_quality(q[c]);
        const float de = dist + 0.01f;
        tc.x = tc.x + col[c].x * quality / de; tc.y = tc.y + col[c].y * quality / de; tc.z = tc.z + col[c].z * quality / de;
        tw += quality / de;
        tc2.x = tc2.x + col[c].x / dist; tc2.y = tc2.y + col[c].y / dist; tc2.z = tc2.z + col[c].z / dist;
        tw2 += 1.0f / dist;
      }
  }
  if (tw > 0.0f) return make_float4(tc.x / tw, tc.y / tw, tc.z / tw, 1.0f);
  return make_float4(tc2.x / tw2, tc2.y / tw2, tc2.z / tw2, -1.0f);
}

}  // namespace rr
#endif
