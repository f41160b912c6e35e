// The overlays the client draws after drawF() in mono mode (source/kinect_client.cpp:672-683), depth-tested into the framebuffer:
//   "Draw TSDF"      kinect::ReconCalibs::draw(), framework/reconstruction/recon_calibs.cpp:54-61 + glsl/calib_vis.{vs,fs}: one GL point per
//                    cell of stream 0's inverse LUT grid, coloured by the TSDF sampled there
//   "Draw frustums"  CalibVolumes::drawFrustums() -> Frustum::draw(), framework/calibration/frustum.cpp:45-95: per stream 12 lines between
//                    the forward LUT's corner samples and a 3-pixel point at the camera position
// GL_LESS with primitives drawn in order is the depth-key rasteriser of raster_dev.hpp, the single statement of the scheme; here the keys are
// seeded with the framebuffer's depth as it was before the overlay, and the resolve leaves a pixel without a winner as the previous draw left it.
// The client then draws the bounding-box wireframe (gloost::BoundingBox::draw, width-2 lines, same scheme) and the texture view
// (TextureBlitter::blit, a bilinear blit of texture unit 15 or 16 into the lower-left of the frame, no depth test).
// Between the frustums and the bounding box (or inside drawF() itself, setDrawBricks) come the wireframes of the occupied bricks
// (ReconIntegration::drawOccupiedBricks, recon_integration.cpp:447-454): width-1 lines, the same scheme, thousands of short segments.
// Last in this file: the GUI's per-sensor "Show textures" windows (tsdf_draw_sensor_texture), one lane per pixel, blended, no depth.
// The definitions GL leaves open (point size, line rasterisation, depth clamp) are listed in include/rgbd_recon_hip.h and restated in
// tests/overlay_reference.py.
#include "raster_dev.hpp"

namespace rr {

__global__ __launch_bounds__(256) void k_overlay_clear(const float* __restrict__ fb_d, unsigned long long* __restrict__ key, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) key[i] = depth_key(fb_d[i], kNoId);
}

// the winner's colour from its primitive index (a functor), and its depth; a pixel no fragment passed at stays as the previous draw left it
template <class Color>
__global__ __launch_bounds__(256) void k_overlay_resolve(Color color, int n, const unsigned long long* __restrict__ key, float4* __restrict__ fb_c,
                                                         float* __restrict__ fb_d) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = key[i];
  if (key_id(k) == kNoId) return;
  fb_c[i] = color(key_id(k));
  fb_d[i] = key_depth(k);
}
struct SolidColor { float4 c; __device__ float4 operator()(uint32_t) const { return c; } };

// one overlay draw: clear, the caller's scatter launch, resolve
template <class Scatter, class Color>
static void overlay_draw(hipStream_t st, const OverlayView& view, unsigned long long* key, float4* fb_c, float* fb_d, Scatter scatter, Color color) {
  const int n = view.w * view.h;
  hipLaunchKernelGGL(k_overlay_clear, dim3((n + 255) / 256), dim3(256), 0, st, fb_d, key, n);
  scatter();
  hipLaunchKernelGGL(k_overlay_resolve<Color>, dim3((n + 255) / 256), dim3(256), 0, st, color, n, key, fb_c, fb_d);
}

// ---- "Draw TSDF"
template <bool kSparse>
__device__ __forceinline__ float calib_sample(const CalibVisParams& Q, const Volume& V, int x, int y, int z, float* u) {
  u[0] = ((float)x + 0.5f) * Q.step[0]; u[1] = ((float)y + 0.5f) * Q.step[1]; u[2] = ((float)z + 0.5f) * Q.step[2];   // volume_sampler.cpp:33-45
  return tex3d_tsdf<kSparse, true>(V, u[0], u[1], u[2]);                                                               // calib_vis.vs:37
}
// calib_vis.fs:17-30; the division is IEEE (not a multiply by the reciprocal)
__device__ __forceinline__ float4 calib_color(float d) {
  const float inv = fabsf(d) / kCalibVisLimit;
  float4 c = d > 0.0f ? make_float4(1.0f - inv, 0.0f, 0.0f, 1.0f) : make_float4(0.0f, 1.0f - inv, 0.0f, 1.0f);
  if (d >= kCalibVisLimit) c = make_float4(0.0f, 0.0f, 1.0f, 1.0f);
  return c;
}

template <bool kSparse>
__global__ __launch_bounds__(256) void k_calibvis_scatter(CalibVisParams Q, Volume V, const float* __restrict__ fb_d, unsigned long long* __restrict__ key) {
  const int t = threadIdx.x;
  const int b0[3] = {(int)blockIdx.x * 8, (int)blockIdx.y * 8, (int)blockIdx.z * 4}, bn[3] = {8, 8, 4};
  if (Q.skip) {
    // Empty-space skip.  lerpf(a, a, t) == a, so a sample whose eight taps all hold the clear value -limit IS -limit, and -limit <= -0.01 is
    // discarded (the host sets skip only then).  Taps are monotone in the grid coordinate: the block's first and last point bound them.
    int lo[3], hi[3], cnt = 1;
    for (int a = 0; a < 3; ++a) {
      const int last = min(b0[a] + bn[a], Q.gres[a]) - 1;
      lo[a] = axis_linear(((float)b0[a] + 0.5f) * Q.step[a], V.res[a]).i0 >> 3;
      hi[a] = axis_linear(((float)last + 0.5f) * Q.step[a], V.res[a]).i1 >> 3;
      cnt *= last - b0[a] + 1;
    }
    const int nx = hi[0] - lo[0] + 1, ny = hi[1] - lo[1] + 1, nt = nx * ny * (hi[2] - lo[2] + 1);
    if (nt <= 1024) {                                                    // (a LUT far coarser than the volume: too many tiles to be worth a look)
      int mixed = 0;
      for (int k = t; k < nt; k += 256) {
        const int tx = lo[0] + k % nx, ty = lo[1] + (k / nx) % ny, tz = lo[2] + k / (nx * ny);
        mixed |= V.cls[(uint32_t)__mul24(__mul24(tz - V.tz0, V.nty) + ty, V.ntx) + (uint32_t)tx] != kTileMinus;
      }
      if (!__syncthreads_or(mixed)) {
        if (t == 0) atomicAdd(Q.skipped, (unsigned long long)cnt);
        return;
      }
    }
  }
  const int x = b0[0] + (t & 7), y = b0[1] + ((t >> 3) & 7), z = b0[2] + (t >> 6);
  if (x >= Q.gres[0] || y >= Q.gres[1] || z >= Q.gres[2]) return;
  float u[3];
  const float d = calib_sample<kSparse>(Q, V, x, y, z, u);
  if (d <= -kCalibVisLimit) return;                                      // calib_vis.fs:29: discard (before the depth test)
  const float4 pw = mat_mul(Q.v2w, u[0], u[1], u[2], 1.0f);              // calib_vis.vs:29-38, in this order
  const float4 pe = mat_mul(Q.view.mv, pw.x, pw.y, pw.z, 1.0f);
  const float4 clip = mat_mul(Q.view.proj, pe.x, pe.y, pe.z, 1.0f);      // (w = 1 here, not pe.w: the shader's own expression)
  const WindowPoint win = point_to_window(clip, Q.view.w, Q.view.h);
  if (!win.ok) return;
  const PixelBox b = square_coverage(win.pos.x, win.pos.y, 0.5f, Q.view.w, Q.view.h);   // a 1-pixel point
  const uint32_t id = (uint32_t)((z * Q.gres[1] + y) * Q.gres[0] + x);   // draw order: x fastest, then y, then z
  for (int py = b.y0; py <= b.y1; ++py)
    for (int px = b.x0; px <= b.x1; ++px) overlay_fragment(fb_d, key, py * Q.view.w + px, win.pos.z, id);
}

template <bool kSparse>
struct CalibVisColor {                                                   // recomputed from the id: no per-point colour store
  CalibVisParams Q; Volume V;
  __device__ float4 operator()(uint32_t id) const {
    const int x = (int)(id % (uint32_t)Q.gres[0]), y = (int)((id / (uint32_t)Q.gres[0]) % (uint32_t)Q.gres[1]), z = (int)(id / (uint32_t)(Q.gres[0] * Q.gres[1]));
    float u[3];
    return calib_color(calib_sample<kSparse>(Q, V, x, y, z, u));
  }
};
template <bool kSparse>
static void draw_calibvis(hipStream_t st, const CalibVisParams& Q, const Volume& V, unsigned long long* key, float4* fb_c, float* fb_d) {
  const dim3 grid((Q.gres[0] + 7) / 8, (Q.gres[1] + 7) / 8, (Q.gres[2] + 3) / 4);
  overlay_draw(st, Q.view, key, fb_c, fb_d, [&] { hipLaunchKernelGGL(k_calibvis_scatter<kSparse>, grid, dim3(256), 0, st, Q, V, fb_d, key); },
               CalibVisColor<kSparse>{Q, V});
}
void launch_draw_calibvis(hipStream_t st, const CalibVisParams& Q, const Volume& V, unsigned long long* key, float4* fb_c, float* fb_d) {
  if (V.slot) draw_calibvis<true>(st, Q, V, key, fb_c, fb_d); else draw_calibvis<false>(st, Q, V, key, fb_c, fb_d);
}

// ---- "Draw frustums": 13 primitives per stream (the 12 lines of frustum.cpp:48-84, then the camera point of :87-94), one wave each
__constant__ int c_frustum_lines[12][2] = {{0, 4}, {1, 5}, {2, 6}, {3, 7}, {0, 1}, {1, 2}, {2, 3}, {3, 0}, {4, 5}, {5, 6}, {6, 7}, {7, 4}};

__device__ __forceinline__ float4 frustum_clip(const FrustumParams& Q, const float* p) { return clip_pos(Q.view.mv, Q.view.proj, p[0], p[1], p[2]); }
__global__ __launch_bounds__(64) void k_frustum_lines(FrustumParams Q, const float* __restrict__ fb_d, unsigned long long* __restrict__ key) {
  const int prim = blockIdx.x, s = prim / 13, k = prim % 13, lane = threadIdx.x;
  const uint32_t id = (uint32_t)prim;                                    // stream * 13 + k: the draw order
  const int w = Q.view.w, h = Q.view.h;
  if (k == 12) {                                                         // glPointSize(3) at the camera position
    const WindowPoint win = point_to_window(frustum_clip(Q, Q.cam[s]), w, h);
    if (!win.ok) return;
    const PixelBox b = square_coverage(win.pos.x, win.pos.y, 1.5f, w, h);
    const int nx = b.x1 - b.x0 + 1, ny = b.y1 - b.y0 + 1;
    if (nx <= 0 || ny <= 0) return;
    for (int q = lane; q < nx * ny; q += 64) overlay_fragment(fb_d, key, (b.y0 + q / nx) * w + b.x0 + q % nx, win.pos.z, id);
    return;
  }
  overlay_line(frustum_clip(Q, Q.corner[s][c_frustum_lines[k][0]]), frustum_clip(Q, Q.corner[s][c_frustum_lines[k][1]]), w, h, 1, id, lane, fb_d, key);
}

struct FrustumColor {                                                    // frustum.cpp:49 (the lines) / :91 (the point)
  __device__ float4 operator()(uint32_t id) const { return id % 13 == 12 ? make_float4(1.0f, 0.0f, 0.0f, 1.0f) : make_float4(0.0f, 1.0f, 0.0f, 1.0f); }
};
void launch_draw_frustums(hipStream_t st, const FrustumParams& Q, unsigned long long* key, float4* fb_c, float* fb_d) {
  overlay_draw(st, Q.view, key, fb_c, fb_d, [&] { hipLaunchKernelGGL(k_frustum_lines, dim3(Q.n * 13), dim3(64), 0, st, Q, fb_d, key); }, FrustumColor{});
}

// ---- the bounding-box wireframe: gloost::BoundingBox::draw() -> drawWiredBox (gloostRenderGoodies.h:251-304), glLineWidth(2).  Six
// GL_LINE_LOOPs of four corners (front, right, back, left, top, bottom), each closed by its v3 -> v0 segment: 24 segments, one wave each,
// primitive index 4 * loop + k.  A corner is x | y << 1 | z << 2 with 0 = bbox_min and 1 = bbox_max on that axis.
__constant__ uint8_t c_bbox_loops[6][4] = {{4, 5, 7, 6}, {5, 1, 3, 7}, {1, 0, 2, 3}, {0, 4, 6, 2}, {6, 7, 3, 2}, {0, 1, 5, 4}};

__device__ __forceinline__ float4 bbox_clip(const BBoxParams& Q, int corner) {
  return clip_pos(Q.view.mv, Q.view.proj, (corner & 1) ? Q.hi[0] : Q.lo[0], (corner & 2) ? Q.hi[1] : Q.lo[1], (corner & 4) ? Q.hi[2] : Q.lo[2]);
}

__global__ __launch_bounds__(64) void k_bbox_lines(BBoxParams Q, const float* __restrict__ fb_d, unsigned long long* __restrict__ key) {
  const int prim = blockIdx.x, loop = prim >> 2, k = prim & 3;
  overlay_line(bbox_clip(Q, c_bbox_loops[loop][k]), bbox_clip(Q, c_bbox_loops[loop][(k + 1) & 3]), Q.view.w, Q.view.h, 2, (uint32_t)prim, threadIdx.x, fb_d,
               key);
}

void launch_draw_bbox(hipStream_t st, const BBoxParams& Q, unsigned long long* key, float4* fb_c, float* fb_d) {
  overlay_draw(st, Q.view, key, fb_c, fb_d, [&] { hipLaunchKernelGGL(k_bbox_lines, dim3(24), dim3(64), 0, st, Q, fb_d, key); },
               SolidColor{make_float4(1.0f, 1.0f, 1.0f, 0.75f)});        // glColor4f(1, 1, 1, 0.75), BoundingBox.cpp:304-305
}

// ---- "Draw occupied bricks": ReconIntegration::drawOccupiedBricks() (recon_integration.cpp:447-454) = glsl/bricks.vs + glsl/solid.fs over
// UnitCube::drawWireInstanced (unit_cube.cpp:20-29,74-83): 12 width-1 lines per brick of the latest updateOccupiedBricks(), colour (1, 0, 0, 1).
// A cube corner is x | y << 1 | z << 2 (0 / 1 = the unit cube's coordinate); the cube's vertex v0..v7 and its 12 segments start -> end, in
// draw order.  Primitive index 12 * brick id + segment: GL draws the instances in list order and the reference's list ascends in brick id,
// so the key is independent of the order of the device list.
__constant__ uint8_t c_cube_vertex[8] = {7, 6, 3, 2, 5, 4, 0, 1};
__constant__ uint8_t c_cube_wire[12][2] = {{0, 1}, {0, 2}, {0, 4}, {5, 1}, {5, 4}, {5, 6}, {3, 1}, {3, 6}, {3, 2}, {7, 2}, {7, 4}, {7, 6}};

// bricks.vs:16-20: P . (MV . to_world(position, index_3d(id))), to_world in the operand order of inc_bricks.glsl:22-24 (k_depth_limits)
__device__ __forceinline__ float4 brick_corner_clip(const BrickWireParams& Q, const Bricks& B, uint32_t id, int corner) {
  int idx[3];
  idx[2] = (int)(id / (uint32_t)(B.res[0] * B.res[1]));                  // index_3d(), inc_bricks.glsl:30-38
  const uint32_t rem = id % (uint32_t)(B.res[0] * B.res[1]);
  idx[1] = (int)(rem / (uint32_t)B.res[0]);
  idx[0] = (int)(rem % (uint32_t)B.res[0]);
  float p[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) p[a] = (float)idx[a] * B.size[a] + B.bbox_min[a] + (((corner >> a) & 1) ? 1.0f : 0.0f) * B.size[a];
  return clip_pos(Q.view.mv, Q.view.proj, p[0], p[1], p[2]);
}

// The plain form (kept for comparison, RR_BRICKWIRE_PLAIN=1): one wave per (brick, segment) pair, each projecting its two corners and
// walking its segment with overlay_line -- for a brick of a few tens of pixels most of the 64 lanes have no pixel column.
__global__ __launch_bounds__(64) void k_brickwire_plain(BrickWireParams Q, Bricks B, const float* __restrict__ fb_d, unsigned long long* __restrict__ key) {
  const uint32_t n = *B.num_occupied * 12u;
  for (uint32_t p = blockIdx.x; p < n; p += gridDim.x) {
    const uint32_t id = B.occupied[p / 12u], s = p % 12u;
    overlay_line(brick_corner_clip(Q, B, id, c_cube_vertex[c_cube_wire[s][0]]), brick_corner_clip(Q, B, id, c_cube_vertex[c_cube_wire[s][1]]), Q.view.w,
                 Q.view.h, 1, id * 12u + s, threadIdx.x, fb_d, key);
  }
}

// The balanced form: a persistent grid of single-wave workgroups, one brick at a time from the compacted list (k_depth_limits' shape).
// Lanes 0..7 project the cube's eight vertices once; lanes 0..11 clip and set up one segment each (overlay_line_setup, the operations of
// overlay_line); the candidate pixel columns / rows [lo, hi] of the 12 segments are concatenated and the 64 lanes walk that one list with
// overlay_line_fragment, so that the lanes stay busy whatever the segments' lengths.  Vertices and set-ups go through LDS (one b128
// write and two b128 reads per lane and phase; twelve ds_bpermute per phase would cost more LDS issue slots than that).
__global__ __launch_bounds__(64) void k_brickwire_scatter(BrickWireParams Q, Bricks B, const float* __restrict__ fb_d, unsigned long long* __restrict__ key) {
  __shared__ float4 s_clip[8];
  __shared__ float4 s_seg[12][2];                                        // (s0, s1, o0, o1), (az, bz, bits of lo, bits of xmajor)
  __shared__ int s_cnt[12];                                              // candidate pixel columns / rows per segment
  const int lane = threadIdx.x;
  const int n_occ = (int)*B.num_occupied;
  for (int w = blockIdx.x; w < n_occ; w += gridDim.x) {
    const uint32_t id = B.occupied[w];
    float4 cl = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (lane < 8) { cl = brick_corner_clip(Q, B, id, c_cube_vertex[lane]); s_clip[lane] = cl; }
    // Early out, exact: (a) every vertex fails the near test, or every vertex fails the far test -- clip_plane drops each of the 12
    // segments; (b) no vertex fails either (no segment is clipped, so every end point is a vertex with w > 0: z + w >= 0 and w - z >= 0
    // give w >= 0, and w = 0 would make z = 0 and the window depth NaN -- excluded with w > 0) and every vertex lies beyond the same side of
    // the view: x > w > 0 makes x / w >= 1 and the window coordinate >= W, x < -w makes it <= 0 (y alike), and no pixel centre i + 0.5
    // with 0 <= i < W lies in a half-open interval between two such coordinates.
    const bool live = lane < 8;
    const bool near_in = cl.z + cl.w >= 0.0f, far_in = cl.w - cl.z >= 0.0f;
    const unsigned long long all8 = 0xffull;
    const unsigned long long m_near = __ballot(live && near_in), m_far = __ballot(live && far_in);
    if (m_near == 0 || m_far == 0) continue;
    if (m_near == all8 && m_far == all8 && __ballot(live && cl.w > 0.0f) == all8) {
      if (__ballot(live && cl.x > cl.w) == all8 || __ballot(live && cl.x < -cl.w) == all8 || __ballot(live && cl.y > cl.w) == all8 ||
          __ballot(live && cl.y < -cl.w) == all8) continue;
    }
    __syncthreads();
    int cnt = 0;
    if (lane < 12) {
      LineSetup L;
      if (overlay_line_setup(s_clip[c_cube_wire[lane][0]], s_clip[c_cube_wire[lane][1]], Q.view.w, Q.view.h, 1, L)) {
        cnt = L.hi - L.lo + 1;
        s_seg[lane][0] = make_float4(L.s0, L.s1, L.o0, L.o1);
        s_seg[lane][1] = make_float4(L.az, L.bz, __int_as_float(L.lo), __int_as_float(L.xmajor));
      }
    }
    if (lane < 12) s_cnt[lane] = cnt;
    __syncthreads();
    int end[12];                                                          // inclusive prefix sum of the counts, in every lane (broadcast reads)
    end[0] = s_cnt[0];
#pragma unroll
    for (int s = 1; s < 12; ++s) end[s] = end[s - 1] + s_cnt[s];
    for (int k = lane; k < end[11]; k += 64) {
      int s = 0, first = 0;
#pragma unroll
      for (int q = 0; q < 11; ++q) if (k >= end[q]) { s = q + 1; first = end[q]; }   // the segment whose range holds candidate k
      const float4 g0 = s_seg[s][0], g1 = s_seg[s][1];
      overlay_line_fragment(g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, __float_as_int(g1.w) != 0, __float_as_int(g1.z) + (k - first), Q.view.w,
                            Q.view.h, 1, id * 12u + (uint32_t)s, fb_d, key);
    }
  }
}

void launch_draw_brickwire(hipStream_t st, const BrickWireParams& Q, const Bricks& B, unsigned long long* key, float4* fb_c, float* fb_d, bool plain) {
  // the list's length is a device scalar: the grids are sized by the brick grid, never by a read-back
  overlay_draw(st, Q.view, key, fb_c, fb_d, [&] {
    if (plain) hipLaunchKernelGGL(k_brickwire_plain, dim3(12ll * B.n < 65536 ? 12 * B.n : 65536), dim3(64), 0, st, Q, B, fb_d, key);
    else hipLaunchKernelGGL(k_brickwire_scatter, dim3(B.n < 8192 ? B.n : 8192), dim3(64), 0, st, Q, B, fb_d, key);
  }, SolidColor{make_float4(1.0f, 0.0f, 0.0f, 1.0f)});                   // uniform Color (1, 0, 0), solid.fs: (Color, 1)
}

// ---- the texture view: TextureBlitter::blit(unit, res) (texture_blitter.cpp, glsl/texture_passthrough.{vs,fs} mode 0) of texture unit 15
// (the hole-filling atlas) or 16 (the brick depth-limit image) into the viewport (0, 0, vw, vh), one lane per output pixel.  No depth test,
// no depth write: fb_d is not touched, nor is any pixel outside the viewport.
__device__ __forceinline__ float4 blit_texel(const BlitParams& Q, int x, int y) {
  const size_t o = (size_t)y * (size_t)Q.sw + (size_t)x;
  if (!Q.peels) return Q.src[o];
  // the depth-limit image as GL's MIN blend leaves it, clear (1, 0, 1, 0) (recon_integration.cpp:144): the peels hold (min z, MAX z, min
  // back-face z, 0) as bits, GL's green channel is min(0, -z) = 0 - max z (+0 where no brick fragment landed)
  const uint4 p = ((const uint4*)Q.src)[o];
  return make_float4(__uint_as_float(p.x), 0.0f - __uint_as_float(p.y), __uint_as_float(p.z), __uint_as_float(p.w));
}

__global__ __launch_bounds__(256) void k_blit_texture(BlitParams Q, float4* __restrict__ fb_c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Q.vw * Q.vh) return;
  const int x = i % Q.vw, y = i / Q.vw;
  const float u = ((float)x + 0.5f) / (float)Q.vw, v = ((float)y + 0.5f) / (float)Q.vh;   // the full-screen triangle's texcoord at the pixel centre
  const Axis X = axis_linear(u, Q.sw), Y = axis_linear(v, Q.sh);          // LINEAR, CLAMP_TO_EDGE (= MIRRORED_REPEAT for u, v in [0, 1])
  const float4 t00 = blit_texel(Q, X.i0, Y.i0), t10 = blit_texel(Q, X.i1, Y.i0), t01 = blit_texel(Q, X.i0, Y.i1), t11 = blit_texel(Q, X.i1, Y.i1);
  fb_c[(size_t)y * Q.fw + x] = make_float4(lerpf(lerpf(t00.x, t10.x, X.a), lerpf(t01.x, t11.x, X.a), Y.a),
                                           lerpf(lerpf(t00.y, t10.y, X.a), lerpf(t01.y, t11.y, X.a), Y.a),
                                           lerpf(lerpf(t00.z, t10.z, X.a), lerpf(t01.z, t11.z, X.a), Y.a), 1.0f);   // vec4(texture(..).rgb, 1)
}

void launch_blit_texture(hipStream_t st, const BlitParams& Q, float4* fb_c) {
  const int n = Q.vw * Q.vh;
  hipLaunchKernelGGL(k_blit_texture, dim3((n + 255) / 256), dim3(256), 0, st, Q, fb_c);
}

// ---- the GUI's "Show textures" windows (kinect_client.cpp:483-515): ImGui::Image of one layer of one of NetKinectArray's texture arrays,
// drawn by the ImGui back-end's array mode (imgui_impl_glfw_glb.cpp:68-74,111-124,260-285): an alpha-blended quad whose fragment shader turns
// the texture coordinate by radians(90.0) about (.5, .5).  One lane per destination pixel; no depth test, no depth write.  The definition
// (coverage, Frag_UV, the turn, the blend) is in include/rgbd_recon_hip.h and restated by tests/sensor_view_reference.py.
// cosf / sinf of the fp32 value of radians(90.0) = 1.5707964f
constexpr float kSensorRotC = -4.37113883e-08f, kSensorRotS = 1.0f;

template <int kMode>
__device__ __forceinline__ float4 sensor_sample(const SensorTexParams& Q, const FrameImages& F, float u, float v) {
  if (kMode == kSensorSlotDepth || kMode == kSensorSlotQuality || kMode == kSensorSlotSilhouette) {
    const Dqs d = dqs_fetch(F, Q.layer, u, v);
    if (kMode == kSensorSlotDepth) return make_float4(dqs_depth(d), 0.0f, 0.0f, 1.0f);
    if (kMode == kSensorSlotSilhouette) return make_float4(dqs_silhouette(d), 0.0f, 0.0f, 1.0f);
    const float q = dqs_quality(d);
    return make_float4(q, q, q, 1.0f);
  }
  if (kMode == kSensorRgNearest || kMode == kSensorLumNearest) {
    const uint32_t o = (uint32_t)__mul24(axis_nearest(v, Q.sh), Q.sw) + (uint32_t)axis_nearest(u, Q.sw);
    if (kMode == kSensorRgNearest) { const float2 t = ((const float2*)Q.src)[o]; return make_float4(t.x, t.y, 0.0f, 1.0f); }
    const float t = ((const float*)Q.src)[o];
    return make_float4(t, t, t, 1.0f);
  }
  const Axis X = axis_linear(u, Q.sw), Y = axis_linear(v, Q.sh);
  const uint32_t r0 = (uint32_t)__mul24(Y.i0, Q.sw), r1 = (uint32_t)__mul24(Y.i1, Q.sw);
  if (kMode == kSensorRgb32f) {
    const float4* __restrict__ t = (const float4*)Q.src;
    const float3 c = lerp3(lerp3(t[r0 + X.i0], t[r0 + X.i1], X.a), lerp3(t[r1 + X.i0], t[r1 + X.i1], X.a), Y.a);
    return make_float4(c.x, c.y, c.z, 1.0f);
  }
  // RGBA8, unsigned normalised: c / 255 (an IEEE division) before the filter, all four channels
  const uchar4* __restrict__ t = (const uchar4*)Q.src;
  const uchar4 t00 = t[r0 + X.i0], t10 = t[r0 + X.i1], t01 = t[r1 + X.i0], t11 = t[r1 + X.i1];
  return make_float4(lerpf(lerpf(t00.x / 255.0f, t10.x / 255.0f, X.a), lerpf(t01.x / 255.0f, t11.x / 255.0f, X.a), Y.a),
                     lerpf(lerpf(t00.y / 255.0f, t10.y / 255.0f, X.a), lerpf(t01.y / 255.0f, t11.y / 255.0f, X.a), Y.a),
                     lerpf(lerpf(t00.z / 255.0f, t10.z / 255.0f, X.a), lerpf(t01.z / 255.0f, t11.z / 255.0f, X.a), Y.a),
                     lerpf(lerpf(t00.w / 255.0f, t10.w / 255.0f, X.a), lerpf(t01.w / 255.0f, t11.w / 255.0f, X.a), Y.a));
}

// A workgroup is four waves, a wave an 8 x 8 tile of destination pixels: the quarter turn makes destination rows walk source columns, so a
// wave laid out as a 64-pixel row would read 64 texels a full source row apart.  As a square its loads and its stores fall into 8 runs each.
template <int kMode>
__global__ __launch_bounds__(256) void k_sensor_texture(SensorTexParams Q, FrameImages F, float4* __restrict__ fb_c) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = Q.x0 + (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
  const int j = Q.y0 + (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
  if (i < Q.sx0 || i >= Q.sx1 || j < Q.sy0 || j >= Q.sy1) return;         // scissor box and view (and with them the launch rectangle's overhang)
  const float cx = (float)i + 0.5f, cy = (float)Q.fh - ((float)j + 0.5f); // the pixel centre in ImGui coordinates
  if (!(Q.pmin[0] <= cx && cx < Q.pmax[0] && Q.pmin[1] <= cy && cy < Q.pmax[1])) return;
  float u = (cx - Q.pmin[0]) / (Q.pmax[0] - Q.pmin[0]), v = (cy - Q.pmin[1]) / (Q.pmax[1] - Q.pmin[1]);   // Frag_UV
  u -= 0.5f; v -= 0.5f;
  const float ru = kSensorRotC * u + kSensorRotS * v, rv = (-kSensorRotS) * u + kSensorRotC * v;   // mat2(c, -s, s, c) * uv, column major
  const float4 s = sensor_sample<kMode>(Q, F, ru + 0.5f, rv + 0.5f);
  float4* const px = fb_c + (size_t)j * Q.fw + i;
  if (s.w == 1.0f) { *px = s; return; }                                   // (every source but DXT colour; nothing from underneath gets through d * 0)
  const float4 d = *px;
  const float k = 1.0f - s.w;                                             // SRC_ALPHA, ONE_MINUS_SRC_ALPHA on all four channels
  *px = make_float4(s.x * s.w + d.x * k, s.y * s.w + d.y * k, s.z * s.w + d.z * k, s.w * s.w + d.w * k);
}

void launch_sensor_texture(hipStream_t st, const SensorTexParams& Q, const FrameImages& F, float4* fb_c) {
  if (Q.nx <= 0 || Q.ny <= 0) return;
  const dim3 grid((Q.nx + 15) / 16, (Q.ny + 15) / 16), block(256);
  switch (Q.mode) {
#define RR_SENSOR_CASE(m) case m: hipLaunchKernelGGL(k_sensor_texture<m>, grid, block, 0, st, Q, F, fb_c); break
    RR_SENSOR_CASE(kSensorRgba8); RR_SENSOR_CASE(kSensorRgNearest); RR_SENSOR_CASE(kSensorSlotDepth); RR_SENSOR_CASE(kSensorSlotQuality);
    RR_SENSOR_CASE(kSensorSlotSilhouette); RR_SENSOR_CASE(kSensorRgb32f); RR_SENSOR_CASE(kSensorLumNearest);
#undef RR_SENSOR_CASE
  }
}

}  // namespace rr
