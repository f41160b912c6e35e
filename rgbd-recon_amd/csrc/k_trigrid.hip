// Triangle-grid back-end (gfx950), SURVEY.md section 8 f4: kinect::ReconTrigrid::draw(), framework/reconstruction/recon_trigrid.cpp:85-148
// with glsl/trigrid_accum.{vs,gs,fs} and trigrid_normalize.fs.  Two triangles per depth-pixel cell and sensor:
//   stage 0  z-buffer of all surviving fragments           -> atomicMin on the window-z bit pattern (z in [0,1])
//   stage 1  quality-weighted shaded colour of every fragment within epsilon of the front surface, ONE/ONE blending
//                                                           -> four fp32 atomicAdd per fragment
//   stage 2  colour / weight where weight > 0, depth from stage 0
// One thread per (cell, sensor) sets up both triangles (the triangles are a pixel or two across: a scan of the bounding box
// is the whole rasteriser).  Coverage, interpolation and every test are the oracle's expressions in the oracle's order; the
// only difference is the ORDER of the additive blend (GL blends in draw order, atomics in arrival order), which moves the
// last bits of the colour, never the depth or the coverage.  Literal quirks kept: the vertex buffer's swapped loop bounds
// (cells x < H, y < W, recon_trigrid.cpp:53-54) and trigrid_accum.fs:69's extra half pixel.
#include "trigrid_dev.hpp"

namespace rr {

__device__ __forceinline__ TriVert tri_vertex(const ViewParams& P, const PointParams& Q, const StreamTable& T, const FrameImages& F, int l, int gx, int gy) {
  const float u = grid_u(gx, F.w), v = grid_u(gy, F.h);                  // recon_trigrid.cpp:51-52
  const int nx = axis_nearest(u, F.w), ny = axis_nearest(v, F.h);
  const float4 dq = F.dqs[((size_t)l * F.h + ny) * F.w + nx];
  return tri_vertex_at(P, Q, T, l, u, v, dq.x, dq.x, dq.y);
}

template <int kStage>
__global__ __launch_bounds__(256) void k_trigrid(ViewParams P, PointParams Q, StreamTable T, FrameImages F, float min_length, uint32_t* __restrict__ zbuf,
                                                 float* __restrict__ acc) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), l = blockIdx.z;
  if (x >= F.h || y >= F.w) return;                                      // sic: cells x < height, y < width (recon_trigrid.cpp:53-54)
  const TriVert v00 = tri_vertex(P, Q, T, F, l, x, y), v10 = tri_vertex(P, Q, T, F, l, x + 1, y), v01 = tri_vertex(P, Q, T, F, l, x, y + 1),
                v11 = tri_vertex(P, Q, T, F, l, x + 1, y + 1);
  tri_cell<kStage, false>(P, Q, F, min_length, l, v00, v10, v01, v11, zbuf, acc);
}

__global__ __launch_bounds__(256) void k_trigrid_clear(uint32_t* __restrict__ zbuf, float4* __restrict__ acc, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { zbuf[i] = __float_as_uint(1.0f); acc[i] = make_float4(0, 0, 0, 0); }
}
__global__ __launch_bounds__(256) void k_trigrid_normalize(const uint32_t* __restrict__ zbuf, const float4* __restrict__ acc, int n, float4* __restrict__ fb_c,
                                                           float* __restrict__ fb_d) {                        // trigrid_normalize.fs
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 a = acc[i];
  if (a.w > 0.0f) { fb_c[i] = make_float4(a.x / a.w, a.y / a.w, a.z / a.w, a.w / a.w); fb_d[i] = __uint_as_float(zbuf[i]); }
  else { fb_c[i] = make_float4(0, 0, 0, 0); fb_d[i] = 1.0f; }
}

void launch_tri_clear(hipStream_t st, uint32_t* zbuf, float4* acc, int n) {
  hipLaunchKernelGGL(k_trigrid_clear, dim3((n + 255) / 256), dim3(256), 0, st, zbuf, acc, n);
}
void launch_tri_normalize(hipStream_t st, const uint32_t* zbuf, const float4* acc, int n, float4* fb_c, float* fb_d) {
  hipLaunchKernelGGL(k_trigrid_normalize, dim3((n + 255) / 256), dim3(256), 0, st, zbuf, acc, n, fb_c, fb_d);
}
void launch_draw_trigrid(hipStream_t st, const ViewParams& P, const PointParams& Q, const StreamTable& T, const FrameImages& F, float min_length, uint32_t* zbuf,
                         float4* acc, float4* fb_c, float* fb_d) {
  const int n = P.w * P.h;
  const dim3 cells((F.h + 63) / 64, (F.w + 3) / 4, T.n);
  launch_tri_clear(st, zbuf, acc, n);
  hipLaunchKernelGGL(k_trigrid<0>, cells, dim3(256), 0, st, P, Q, T, F, min_length, zbuf, (float*)acc);
  hipLaunchKernelGGL(k_trigrid<1>, cells, dim3(256), 0, st, P, Q, T, F, min_length, zbuf, (float*)acc);
  launch_tri_normalize(st, zbuf, acc, n, fb_c, fb_d);
}

}  // namespace rr
