// Point back-end (gfx950), SURVEY.md section 8 f4: kinect::ReconPoints::draw(), framework/reconstruction/recon_points.cpp:71-111
// with glsl/points.vs / points.gs / points.fs -- one GL point sprite per depth pixel and layer, depth-tested into the framebuffer by the
// depth-key rasteriser of raster_dev.hpp; the point id (layer, then row-major pixel) is the draw order, the keys are seeded with the far plane.
// A second kernel shades the winner of every pixel once (all varyings are `flat`).  The definitions GL leaves open are listed in the oracle.
#include "raster_dev.hpp"
#include "shading_dev.hpp"

namespace rr {

struct PointVertex { float3 pos_cs, pos_es; float2 tc; WindowPoint win; float size; };

__device__ __forceinline__ PointVertex point_vertex(const ViewParams& P, const PointParams& Q, const StreamTable& T, const FrameImages& F, int l, int x, int y) {
  PointVertex o;
  o.win.ok = false;
  const float stepX = 1.0f / (float)F.w, stepY = 1.0f / (float)F.h;                    // recon_points.cpp:44-45
  const float u = (float)(((double)x + 0.5) * (double)stepX), v = (float)(((double)y + 0.5) * (double)stepY);   // :48
  const float depth = F.depth[((size_t)l * F.h + y) * F.w + x];
  const StreamLut& L = T.s[l];
  o.pos_cs = tex3d_rgba_xyz(L.xyz, L.xyz_res, u, v, depth);                             // points.vs:27
  o.tc = tex3d_rg(L.uv, L.uv_res, u, v, depth);                                         // :29
  const bool in_box = o.pos_cs.x >= Q.bbox_min[0] && o.pos_cs.y >= Q.bbox_min[1] && o.pos_cs.z >= Q.bbox_min[2] &&
                      o.pos_cs.x <= Q.bbox_max[0] && o.pos_cs.y <= Q.bbox_max[1] && o.pos_cs.z <= Q.bbox_max[2];
  if (!in_box || depth <= 0.0f) return o;                                               // points.gs:36-38
  if (o.tc.x > 0.99f || o.tc.x < 0.01f || o.tc.y > 0.99f || o.tc.y < 0.01f) return o;   // points.fs:38-41
  const float4 pe = mat_mul(P.mv, o.pos_cs.x, o.pos_cs.y, o.pos_cs.z, 1.0f);
  o.pos_es = make_float3(pe.x, pe.y, pe.z);
  const float4 clip = mat_mul(Q.pmv, o.pos_cs.x, o.pos_cs.y, o.pos_cs.z, 1.0f);
  o.win = point_to_window(clip, P.w, P.h);
  if (!o.win.ok) return o;
  const float max_size = P.shade_mode == 3 ? 4.0f : 10.0f;                              // points.gs:49-53
  o.size = fminf(fmaxf(max_size / sqrtf(o.pos_es.x * o.pos_es.x + o.pos_es.y * o.pos_es.y + o.pos_es.z * o.pos_es.z), 1.0f), 2047.0f);
  return o;
}

__global__ __launch_bounds__(256) void k_points_clear(unsigned long long* __restrict__ key, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) key[i] = depth_key(1.0f, kNoId);
}

__global__ __launch_bounds__(256) void k_points_scatter(ViewParams P, PointParams Q, StreamTable T, FrameImages F, unsigned long long* __restrict__ key) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), l = blockIdx.z;
  if (x >= F.w || y >= F.h) return;
  const PointVertex pv = point_vertex(P, Q, T, F, l, x, y);
  if (!pv.win.ok) return;
  const PixelBox b = square_coverage(pv.win.pos.x, pv.win.pos.y, pv.size * 0.5f, P.w, P.h);
  const unsigned long long k = depth_key(pv.win.pos.z, (uint32_t)((l * F.h + y) * F.w + x));
  for (int py = b.y0; py <= b.y1; ++py)
    for (int px = b.x0; px <= b.x1; ++px) keyed_fragment(key, (size_t)py * P.w + px, k);
}

__global__ __launch_bounds__(256) void k_points_resolve(ViewParams P, PointParams Q, StreamTable T, FrameImages F, const unsigned long long* __restrict__ key,
                                                        float4* __restrict__ fb_c, float* __restrict__ fb_d) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P.w * P.h) return;
  const unsigned long long k = key[i];
  const uint32_t id = key_id(k);
  if (id == kNoId) { fb_c[i] = make_float4(0, 0, 0, 0); fb_d[i] = 1.0f; return; }
  const int x = (int)(id % (uint32_t)F.w), y = (int)((id / (uint32_t)F.w) % (uint32_t)F.h), l = (int)(id / (uint32_t)(F.w * F.h));
  const PointVertex pv = point_vertex(P, Q, T, F, l, x, y);
  float3 out;
  if (P.shade_mode == 3) out = make_float3(c_camera_colors[l & 7][0], c_camera_colors[l & 7][1], c_camera_colors[l & 7][2]);   // points.fs:69-71
  else {
    const float3 col = color_bilinear(F, l, pv.tc.x, pv.tc.y);
    float3 n = make_float3(0, 0, 0);
    if (Q.normals) { const float4 t = Q.normals[((size_t)l * F.h + y) * F.w + x]; n = make_float3(t.x, t.y, t.z); }
    const float* mi = P.mv_inv.m;                                                       // inverseTranspose(MV) * (n, 0)
    const float3 vn = make_float3(mi[0] * n.x + mi[1] * n.y + mi[2] * n.z, mi[4] * n.x + mi[5] * n.y + mi[6] * n.z, mi[8] * n.x + mi[9] * n.y + mi[10] * n.z);
    out = shade(P, pv.pos_es, vn, col);
  }
  fb_c[i] = make_float4(out.x, out.y, out.z, 1.0f);
  fb_d[i] = key_depth(k);
}

void launch_draw_points(hipStream_t st, const ViewParams& P, const PointParams& Q, const StreamTable& T, const FrameImages& F, unsigned long long* key,
                        float4* fb_c, float* fb_d) {
  const int n = P.w * P.h;
  hipLaunchKernelGGL(k_points_clear, dim3((n + 255) / 256), dim3(256), 0, st, key, n);
  hipLaunchKernelGGL(k_points_scatter, dim3((F.w + 63) / 64, (F.h + 3) / 4, T.n), dim3(256), 0, st, P, Q, T, F, key);
  hipLaunchKernelGGL(k_points_resolve, dim3((n + 255) / 256), dim3(256), 0, st, P, Q, T, F, key, fb_c, fb_d);
}

}  // namespace rr
