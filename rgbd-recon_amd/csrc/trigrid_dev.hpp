// Device helpers of the two triangle-grid back-ends: kinect::ReconTrigrid (k_trigrid.hip, glsl/trigrid_accum.{vs,gs,fs}) and
// kinect::ReconMVT (k_mvt.hip, glsl/mvt_accum.{vs,gs,fs}).  The two share the host code (recon_trigrid.cpp / recon_mvt.cpp differ in
// their uniforms only), the rasteriser and the fragment tests; they differ in where a vertex's depth comes from, in validSurface and in
// the fragment's quality (kMvt below).  Coverage, interpolation and every test are the oracle's expressions in the oracle's order.
#ifndef RR_TRIGRID_DEV_HPP
#define RR_TRIGRID_DEV_HPP
#include "raster_dev.hpp"
#include "shading_dev.hpp"

namespace rr {

struct TriVert { float3 pos_cs, pos_es; float tcx, tcy, depth, quality, xw, yw, zw, iw, nd; bool front; };   // nd = clip.z + clip.w: >= 0 in front of the near plane
struct TriSetup { TriVert v[3]; float3 normal; float area; bool ok, cut; };
struct TriFragment { float z, tcx, tcy, quality, depth; float3 pos_es, pos_cs; };

__device__ __forceinline__ float len3(float3 a) { return sqrtf(a.x * a.x + a.y * a.y + a.z * a.z); }
__device__ __forceinline__ float3 sub3(float3 a, float3 b) { return make_float3(a.x - b.x, a.y - b.y, a.z - b.z); }

// vertex (gx, gy) of the grid (recon_trigrid.cpp:51-62 = recon_mvt.cpp:51-62): texel-centre position (u, v) in the depth image
__device__ __forceinline__ float grid_u(int gx, int w) { const float step = 1.0f / (float)w; return (float)(((double)gx + 0.5) * (double)step); }

// eye, clip and window position of a vertex at pos_cs (trigrid_accum.vs:28,33)
__device__ __forceinline__ void tri_project(const ViewParams& P, const PointParams& Q, TriVert& t) {
  const float4 pe = mat_mul(P.mv, t.pos_cs.x, t.pos_cs.y, t.pos_cs.z, 1.0f);
  t.pos_es = make_float3(pe.x, pe.y, pe.z);
  const float4 clip = mat_mul(Q.pmv, t.pos_cs.x, t.pos_cs.y, t.pos_cs.z, 1.0f);
  t.front = clip.w > 0.0f;
  t.nd = clip.z + clip.w;
  t.iw = 1.0f / clip.w;
  const float3 win = clip_to_window(clip, P.w, P.h);                     // (no clip here: tri_clip_near cuts a triangle that reaches behind the eye)
  t.xw = win.x; t.yw = win.y; t.zw = win.z;
}

// the vertex stage after the depth fetch: calibration-volume lookups at (u, v, lut_w), eye / clip / window position
__device__ __forceinline__ TriVert tri_vertex_at(const ViewParams& P, const PointParams& Q, const StreamTable& T, int l, float u, float v, float lut_w,
                                                 float depth, float quality) {
  TriVert t;
  t.depth = depth; t.quality = quality;
  const StreamLut& L = T.s[l];
  t.pos_cs = tex3d_rgba_xyz(L.xyz, L.xyz_res, u, v, lut_w);
  const float2 tc = tex3d_rg(L.uv, L.uv_res, u, v, lut_w);
  t.tcx = tc.x; t.tcy = tc.y;
  tri_project(P, Q, t);
  return t;
}

// validSurface + triangle set-up of the geometry stage.  Trigrid (trigrid_accum.gs:31-42): depth < 0 rejects, edges < min_length * avg * 4
// (depth normalised to [0, 1]).  MVT (mvt_accum.gs:29-41): depth < 0.5 m rejects, edges < min_length * avg + 0.005 (depth in metres).
template <bool kMvt>
__device__ __forceinline__ TriSetup tri_setup(float min_length, const TriVert& a, const TriVert& b, const TriVert& d) {
  TriSetup S; S.v[0] = a; S.v[1] = b; S.v[2] = d; S.ok = S.cut = false;
  const float dmin = kMvt ? 0.5f : 0.0f;
  if (a.depth < dmin || b.depth < dmin || d.depth < dmin) return S;
  const float avg = (a.depth + b.depth + d.depth) / 3.0f;
  const float l = kMvt ? min_length * avg + 0.005f : min_length * avg * 4.0f;
  if (!(len3(sub3(b.pos_cs, a.pos_cs)) < l && len3(sub3(d.pos_cs, a.pos_cs)) < l && len3(sub3(d.pos_cs, b.pos_cs)) < l)) return S;
  if (!(a.front || b.front || d.front)) return S;
  const float3 ea = sub3(b.pos_es, a.pos_es), eb = sub3(d.pos_es, a.pos_es);
  S.normal = normalize3(make_float3(ea.y * eb.z - eb.y * ea.z, ea.z * eb.x - eb.z * ea.x, ea.x * eb.y - eb.x * ea.y));   // :59
  if (!(a.front && b.front && d.front)) { S.ok = S.cut = true; return S; }   // reaches behind the eye: tri_clip_near() before it is drawn
  S.area = (b.xw - a.xw) * (d.yw - a.yw) - (d.xw - a.xw) * (b.yw - a.yw);
  if (!(S.area != 0.0f)) return S;
  S.ok = true;
  return S;
}

// GL clips a primitive before the window transform.  With every w > 0 the division by w is defined and the per-fragment 0 <= z <= 1 test IS the
// near / far clip: such a triangle is drawn as it stands.  One that reaches behind the eye is cut at the near plane (z = -w; there w > 0 under a
// perspective projection) into one or two triangles with the flat normal of the whole.  A vertex on the plane is i + t (o - i) in pos_cs and in
// every varying, t = nd_i / (nd_i - nd_o) from the inside vertex i to the outside vertex o whichever way the edge runs, so the two triangles of
// an edge get the same point; its eye, clip and window positions follow from pos_cs as a vertex's do.  Part `part` (0, 1) of the cut triangle:
// ok is false where there is none.  The oracle's tri_clip_near, expression for expression.
__device__ __forceinline__ TriSetup tri_clip_near(const ViewParams& P, const PointParams& Q, const TriSetup& T, int part) {
  TriVert p[4];
  int n = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const TriVert &a = T.v[k], &b = T.v[(k + 1) % 3];
    const bool ia = a.front && a.nd >= 0.0f, ib = b.front && b.nd >= 0.0f;
    if (ia) p[n++] = a;
    if (ia != ib) {
      const TriVert &i = ia ? a : b, &o = ia ? b : a;
      const float t = i.nd / (i.nd - o.nd);
      TriVert m;
      m.pos_cs = make_float3(i.pos_cs.x + t * (o.pos_cs.x - i.pos_cs.x), i.pos_cs.y + t * (o.pos_cs.y - i.pos_cs.y), i.pos_cs.z + t * (o.pos_cs.z - i.pos_cs.z));
      m.tcx = i.tcx + t * (o.tcx - i.tcx); m.tcy = i.tcy + t * (o.tcy - i.tcy);
      m.depth = i.depth + t * (o.depth - i.depth); m.quality = i.quality + t * (o.quality - i.quality);
      tri_project(P, Q, m);
      p[n++] = m;
    }
  }
  TriSetup S = T;
  S.cut = S.ok = false;
  const int k = part + 2;
  if (k >= n) return S;
  S.v[0] = p[0]; S.v[1] = p[k - 1]; S.v[2] = p[k];
  S.area = (S.v[1].xw - S.v[0].xw) * (S.v[2].yw - S.v[0].yw) - (S.v[2].xw - S.v[0].xw) * (S.v[1].yw - S.v[0].yw);
  S.ok = S.v[0].front && S.v[1].front && S.v[2].front && S.area != 0.0f;
  return S;
}

__device__ __forceinline__ bool tri_fragment(const TriSetup& S, int px, int py, TriFragment& f) {
  const float x = (float)px + 0.5f, y = (float)py + 0.5f;
  const TriVert &a = S.v[0], &b = S.v[1], &d = S.v[2];
  const float e0 = (d.xw - b.xw) * (y - b.yw) - (d.yw - b.yw) * (x - b.xw);
  const float e1 = (a.xw - d.xw) * (y - d.yw) - (a.yw - d.yw) * (x - d.xw);
  const float e2 = (b.xw - a.xw) * (y - a.yw) - (b.yw - a.yw) * (x - a.xw);
  const float sgn = S.area > 0.0f ? 1.0f : -1.0f;
  const float ex[3] = {(d.xw - b.xw) * sgn, (a.xw - d.xw) * sgn, (b.xw - a.xw) * sgn}, ey[3] = {(d.yw - b.yw) * sgn, (a.yw - d.yw) * sgn, (b.yw - a.yw) * sgn};
  const float ee[3] = {e0 * sgn, e1 * sgn, e2 * sgn};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    if (ee[i] < 0.0f) return false;
    if (ee[i] == 0.0f && !(ey[i] > 0.0f || (ey[i] == 0.0f && ex[i] < 0.0f))) return false;
    if (!(ee[i] >= 0.0f)) return false;
  }
  const float l0 = e0 / S.area, l1 = e1 / S.area, l2 = e2 / S.area;
  f.z = l0 * a.zw + l1 * b.zw + l2 * d.zw;
  if (!(f.z >= 0.0f && f.z <= 1.0f)) return false;
  const float w0 = l0 * a.iw, w1 = l1 * b.iw, w2 = l2 * d.iw, iw = w0 + w1 + w2;
#define RR_IP(p, q, r) ((w0 * (p) + w1 * (q) + w2 * (r)) / iw)
  f.tcx = RR_IP(a.tcx, b.tcx, d.tcx); f.tcy = RR_IP(a.tcy, b.tcy, d.tcy); f.quality = RR_IP(a.quality, b.quality, d.quality);
  f.depth = RR_IP(a.depth, b.depth, d.depth);                            // (read by MVT only)
  f.pos_es = make_float3(RR_IP(a.pos_es.x, b.pos_es.x, d.pos_es.x), RR_IP(a.pos_es.y, b.pos_es.y, d.pos_es.y), RR_IP(a.pos_es.z, b.pos_es.z, d.pos_es.z));
  f.pos_cs = make_float3(RR_IP(a.pos_cs.x, b.pos_cs.x, d.pos_cs.x), RR_IP(a.pos_cs.y, b.pos_cs.y, d.pos_cs.y), RR_IP(a.pos_cs.z, b.pos_cs.z, d.pos_cs.z));
#undef RR_IP
  return true;
}

__device__ __forceinline__ bool tri_fragment_kept(const PointParams& Q, const TriSetup& S, const TriFragment& f, float3& n) {   // trigrid_accum.fs:44-62 = mvt_accum.fs:35-50
  const bool in_box = f.pos_cs.x >= Q.bbox_min[0] && f.pos_cs.y >= Q.bbox_min[1] && f.pos_cs.z >= Q.bbox_min[2] &&
                      f.pos_cs.x <= Q.bbox_max[0] && f.pos_cs.y <= Q.bbox_max[1] && f.pos_cs.z <= Q.bbox_max[2];
  if (!in_box) return false;
  if (f.tcx > 0.99f || f.tcx < 0.01f || f.tcy > 0.99f || f.tcy < 0.01f) return false;
  const float3 nn = normalize3(S.normal);
  n = make_float3(-nn.x, -nn.y, -nn.z);
  const float3 pe = normalize3(f.pos_es);
  if (n.x * pe.x + n.y * pe.y + n.z * pe.z > 0.0f) return false;
  return true;
}

// One set-up triangle, rasterised into the z pre-pass (kStage 0) or the blend (kStage 1): a scan of its bounding box.
// Fragment quality: Trigrid the interpolated quality; MVT lateral_quality / depth, both interpolated (mvt_accum.fs:53).
template <int kStage, bool kMvt>
__device__ __forceinline__ void tri_raster(const ViewParams& P, const PointParams& Q, const FrameImages& F, int l, const TriSetup& S, uint32_t* __restrict__ zbuf,
                                           float* __restrict__ acc) {
  const float minx = fminf(fminf(S.v[0].xw, S.v[1].xw), S.v[2].xw), maxx = fmaxf(fmaxf(S.v[0].xw, S.v[1].xw), S.v[2].xw);
  const float miny = fminf(fminf(S.v[0].yw, S.v[1].yw), S.v[2].yw), maxy = fmaxf(fmaxf(S.v[0].yw, S.v[1].yw), S.v[2].yw);
  if (!(maxx >= 0.0f && maxy >= 0.0f && minx <= (float)P.w && miny <= (float)P.h)) return;
  const int x0 = (int)fmaxf(floorf(minx - 0.5f), 0.0f), x1 = (int)fminf(ceilf(maxx - 0.5f), (float)(P.w - 1));
  const int y0 = (int)fmaxf(floorf(miny - 0.5f), 0.0f), y1 = (int)fminf(ceilf(maxy - 0.5f), (float)(P.h - 1));
  for (int py = y0; py <= y1; ++py)
    for (int px = x0; px <= x1; ++px) {
      TriFragment f;
      if (!tri_fragment(S, px, py, f)) continue;
      float3 n;
      if (!tri_fragment_kept(Q, S, f, n)) continue;
      const size_t o = (size_t)py * P.w + px;
      if (kStage == 0) {
        atomicMin(&zbuf[o], __float_as_uint(f.z));                       // GL_LESS
      } else {
        const float depth_curr = __uint_as_float(zbuf[o]);
        const float4 pc = mat_mul(P.img_to_eye, ((float)px + 0.5f) + 0.5f, ((float)py + 0.5f) + 0.5f, depth_curr, 1.0f);   // sic, trigrid_accum.fs:69
        const float3 es = make_float3(pc.x / pc.w, pc.y / pc.w, pc.z / pc.w);
        if (0.075f < len3(sub3(es, f.pos_es))) continue;                 // epsilon, recon_trigrid.cpp:35
        const float q = kMvt ? f.quality / f.depth : f.quality;
        float3 col;
        if (P.shade_mode == 3) col = make_float3(c_camera_colors[l & 7][0], c_camera_colors[l & 7][1], c_camera_colors[l & 7][2]);
        else col = shade(P, f.pos_es, n, color_bilinear(F, l, f.tcx, f.tcy));
        atomicAdd(&acc[4 * o], col.x * q); atomicAdd(&acc[4 * o + 1], col.y * q);
        atomicAdd(&acc[4 * o + 2], col.z * q); atomicAdd(&acc[4 * o + 3], q);
      }
    }
}

// The two triangles of one cell (recon_trigrid.cpp:55-61); one that reaches behind the eye is drawn as the one or two parts the near plane leaves of it.
template <int kStage, bool kMvt>
__device__ __forceinline__ void tri_cell(const ViewParams& P, const PointParams& Q, const FrameImages& F, float min_length, int l, const TriVert& v00,
                                         const TriVert& v10, const TriVert& v01, const TriVert& v11, uint32_t* __restrict__ zbuf, float* __restrict__ acc) {
#pragma unroll 1
  for (int t = 0; t < 2; ++t) {
    const TriSetup W = t == 0 ? tri_setup<kMvt>(min_length, v00, v10, v01) : tri_setup<kMvt>(min_length, v10, v11, v01);
    if (!W.ok) continue;
#pragma unroll 1
    for (int part = 0; part < (W.cut ? 2 : 1); ++part) {
      const TriSetup S = W.cut ? tri_clip_near(P, Q, W, part) : W;
      if (S.ok) tri_raster<kStage, kMvt>(P, Q, F, l, S, zbuf, acc);
    }
  }
}

}  // namespace rr
#endif
