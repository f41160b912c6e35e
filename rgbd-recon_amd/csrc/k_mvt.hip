// MVT triangle-grid back-end (gfx950): kinect::ReconMVT::draw(), framework/reconstruction/recon_mvt.cpp:84-150, with
// glsl/mvt_accum.{vs,gs,fs} and trigrid_normalize.fs.  The host code and the raster passes are Trigrid's (k_trigrid.hip,
// trigrid_dev.hpp); the vertex stage is not:
//   vertex pass  a 13 x 13 bilateral filter of the RAW sensor depth (metres, NetKinectArray.cpp:173,180,191: the float array; the
//                reference's 8-bit compressed raw array of :170 is not reproduced) around every grid vertex, ONCE per draw, into a
//                per-vertex record (filtered depth, lateral quality) [N][W+1][H+1]: the grid's swapped loop bounds (recon_mvt.cpp:53-54)
//                put whole vertex rows / columns outside the image whenever W != H, and their clamped windows are shifted, so the
//                result belongs to the vertex, not to a texel
//   raster       stage 0 z pre-pass, stage 1 ONE/ONE blend with quality = lateral_quality / depth, normalise (Trigrid's kernels)
// Literal quirks kept (mvt_accum.vs:43-115): constant depth limits 0.5 / 4.5 m (recon_mvt.cpp:35-36, not the sensors' own), range
// threshold 0.35 * (depth / 4.5), spatial weight 1 - |(x, y)| / 6 -- negative for the 56 taps past radius 6, so weights can cancel
// and w <= 0 gives depth 0 --, depth 0 when the range weights sum below 169 * 0.65, and the LUT coordinate (depth - 0.5) / 4 of
// the FILTERED depth.
#include "trigrid_dev.hpp"

namespace rr {

constexpr int kMvtR = 6;                                     // kernel_size, mvt_accum.vs:22
constexpr int kMvtTX = 32, kMvtTY = 8;                       // vertices per workgroup
constexpr int kMvtLW = kMvtTX + 2 * kMvtR, kMvtLH = kMvtTY + 2 * kMvtR;

// bilateral_filter(), mvt_accum.vs:47-101.  c points at the vertex's own texel in the LDS tile (row stride kMvtLW).  Tap (x, y) of
// vertex (gx, gy) is texel (clamp(gx + x, 0, W - 1), clamp(gy + y, 0, H - 1)): the literal fp32 NEAREST lookup of
// u + float(x) * (1 / W) equals that index for every size the project uses (tests/test_mvt_reference.py proves it per size).
__device__ __forceinline__ float2 mvt_filter(const float* c) {
  const float depth = c[0];
  if (depth < 0.5f || depth > 4.5f) return make_float2(0.0f, 0.0f);   // is_outside, cv_min_d / cv_max_d = 0.5 / 4.5
  const float d_dmax = depth / 4.5f;
  const float drm = 0.35f * d_dmax, drm_inv = 1.0f / drm;
  float depth_bf = 0.0f, w = 0.0f, w_range = 0.0f, border = 0.0f;
#pragma unroll
  for (int y = -kMvtR; y <= kMvtR; ++y)
#pragma unroll
    for (int x = -kMvtR; x <= kMvtR; ++x) {
      const float ds = c[y * kMvtLW + x];
      const float dr = fabsf(ds - depth);
      if (ds < 0.5f || ds > 4.5f || dr > drm) { border += 1.0f; continue; }
      const float gs = 1.0f - sqrtf((float)(x * x + y * y)) * (1.0f / 6.0f);   // computeGaussSpace (a constant per tap)
      const float gr = 1.0f - fminf(dr, drm) * drm_inv;                        // computeGaussRange
      const float ws = gs * gr;
      depth_bf += ws * ds;
      w += ws;
      w_range += gr;
    }
  const float lq = 1.0f - border / 169.0f;
  float fd = w > 0.0f ? depth_bf / w : 0.0f;
  if (w_range < 169.0f * 0.65f) fd = 0.0f;
  return make_float2(fd, powf(lq, 30.0f));
}

// one thread per grid vertex (gx in [0, H], gy in [0, W]), 32 x 8 per workgroup; the tile's depth texels plus the 6-texel halo
// (clamped to the image) are staged in LDS once
__global__ __launch_bounds__(256) void k_mvt_vertices(const float* __restrict__ raw, int W, int H, float2* __restrict__ out) {
  __shared__ float tile[kMvtLH * kMvtLW];
  const int l = blockIdx.z, gx0 = blockIdx.x * kMvtTX, gy0 = blockIdx.y * kMvtTY;
  const float* __restrict__ img = raw + (size_t)l * W * H;
  for (int i = threadIdx.x; i < kMvtLH * kMvtLW; i += 256) {
    const int r = i / kMvtLW, q = i - r * kMvtLW;
    tile[i] = img[(size_t)clampi(gy0 - kMvtR + r, 0, H - 1) * W + clampi(gx0 - kMvtR + q, 0, W - 1)];
  }
  __syncthreads();
  const int tx = threadIdx.x & (kMvtTX - 1), ty = threadIdx.x / kMvtTX, gx = gx0 + tx, gy = gy0 + ty;
  if (gx > H || gy > W) return;
  out[((size_t)l * (W + 1) + gy) * (H + 1) + gx] = mvt_filter(&tile[(ty + kMvtR) * kMvtLW + tx + kMvtR]);
}

// main() of mvt_accum.vs after the filter: d_idx = (depth - cv_min_d) / (cv_max_d - cv_min_d), LUT lookups and projection
__device__ __forceinline__ TriVert mvt_vertex(const ViewParams& P, const PointParams& Q, const StreamTable& T, const FrameImages& F, const float2* __restrict__ vtx,
                                              int l, int gx, int gy) {
  const float2 r = vtx[((size_t)l * (F.w + 1) + gy) * (F.h + 1) + gx];
  return tri_vertex_at(P, Q, T, l, grid_u(gx, F.w), grid_u(gy, F.h), (r.x - 0.5f) / 4.0f, r.x, r.y);
}

template <int kStage>
__global__ __launch_bounds__(256) void k_mvt(ViewParams P, PointParams Q, StreamTable T, FrameImages F, float min_length, const float2* __restrict__ vtx,
                                             uint32_t* __restrict__ zbuf, float* __restrict__ acc) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), l = blockIdx.z;
  if (x >= F.h || y >= F.w) return;                                      // sic: cells x < height, y < width (recon_mvt.cpp:53-54)
  const TriVert v00 = mvt_vertex(P, Q, T, F, vtx, l, x, y), v10 = mvt_vertex(P, Q, T, F, vtx, l, x + 1, y), v01 = mvt_vertex(P, Q, T, F, vtx, l, x, y + 1),
                v11 = mvt_vertex(P, Q, T, F, vtx, l, x + 1, y + 1);
  tri_cell<kStage, true>(P, Q, F, min_length, l, v00, v10, v01, v11, zbuf, acc);
}

void launch_draw_mvt(hipStream_t st, const ViewParams& P, const PointParams& Q, const StreamTable& T, const FrameImages& F, const float* raw, float min_length,
                     float2* vtx, uint32_t* zbuf, float4* acc, float4* fb_c, float* fb_d) {
  const int n = P.w * P.h;
  const dim3 verts((F.h + 1 + kMvtTX - 1) / kMvtTX, (F.w + 1 + kMvtTY - 1) / kMvtTY, T.n);
  hipLaunchKernelGGL(k_mvt_vertices, verts, dim3(256), 0, st, raw, F.w, F.h, vtx);
  const dim3 cells((F.h + 63) / 64, (F.w + 3) / 4, T.n);
  launch_tri_clear(st, zbuf, acc, n);
  hipLaunchKernelGGL(k_mvt<0>, cells, dim3(256), 0, st, P, Q, T, F, min_length, (const float2*)vtx, zbuf, (float*)acc);
  hipLaunchKernelGGL(k_mvt<1>, cells, dim3(256), 0, st, P, Q, T, F, min_length, (const float2*)vtx, zbuf, (float*)acc);
  launch_tri_normalize(st, zbuf, acc, n, fb_c, fb_d);
}

}  // namespace rr
