// The depth-key rasteriser of the point back-end (k_points.hip) and the overlays (k_overlay.hip): GL_LESS with primitives drawn in order.
// A draw clears a 64-bit key per pixel, every fragment does an atomicMin of (window z bits << 32 | primitive index) on its pixel, and a
// resolve pass writes the winners' colour and depth.  z is in [0, 1), where uint order == float order, and the index is the draw order, so
// equal depths resolve as GL_LESS does for primitives drawn in order -- deterministic whatever the scheduling.  This file is the single
// statement of the key's layout, the depth test, the whole-point clip, the window transform (fp32, in this operand order; shared with
// trigrid_dev.hpp and k_depth_limits), the square point's coverage and the line rule.
#pragma once
#include "sampling.hpp"

namespace rr {

constexpr uint32_t kNoId = 0xffffffffu;                                  // no fragment: above every primitive index
__device__ __forceinline__ unsigned long long depth_key(float z, uint32_t id) { return ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)id; }
__device__ __forceinline__ float key_depth(unsigned long long k) { return __uint_as_float((uint32_t)(k >> 32)); }
__device__ __forceinline__ uint32_t key_id(unsigned long long k) { return (uint32_t)k; }

// one fragment into a key buffer seeded with the far plane (the point back-end, which draws into a cleared frame): the atomic alone
__device__ __forceinline__ void keyed_fragment(unsigned long long* __restrict__ key, size_t pix, unsigned long long k) { atomicMin(&key[pix], k); }
// one fragment over an earlier draw: strict GL_LESS against the framebuffer's depth, then the in-order tie rule through the key.  Keys only
// decrease: a plain load that already holds a key <= k makes the atomic redundant.
__device__ __forceinline__ void overlay_fragment(const float* __restrict__ fb_d, unsigned long long* __restrict__ key, int pix, float z, uint32_t id) {
  if (!(z < fb_d[pix])) return;
  const unsigned long long k = depth_key(z, id);
  if (k < key[pix]) keyed_fragment(key, pix, k);
}

__device__ __forceinline__ float4 clip_pos(const Mat4& mv, const Mat4& proj, float x, float y, float z) {   // P . (MV . p)
  const float4 e = mat_mul(mv, x, y, z, 1.0f);
  return mat_mul(proj, e.x, e.y, e.z, e.w);
}
__device__ __forceinline__ float3 clip_to_window(float4 clip, int w, int h) {
  return make_float3((clip.x / clip.w * 0.5f + 0.5f) * (float)w, (clip.y / clip.w * 0.5f + 0.5f) * (float)h, clip.z / clip.w * 0.5f + 0.5f);
}
// a GL point: clipped whole by its centre, and dropped at the far plane (the depth test of a cleared buffer is strict).  Returned by value:
// an out-parameter keeps the compiler from sinking the callers' loads below their own early exits (k_points_scatter: 44 -> 66 VGPRs)
struct WindowPoint { float3 pos; bool ok; };
__device__ __forceinline__ WindowPoint point_to_window(float4 clip, int w, int h) {
  WindowPoint p; p.ok = false;
  if (!(clip.w > 0.0f) || fabsf(clip.x) > clip.w || fabsf(clip.y) > clip.w || fabsf(clip.z) > clip.w) return p;
  p.pos = clip_to_window(clip, w, h);
  if (!(p.pos.z < 1.0f)) return p;
  p.ok = true;
  return p;
}
// ... and its coverage: the pixels whose centres lie in the square of half-width `half` about (xw, yw), cut to the view (empty: x1 < x0 or y1 < y0)
struct PixelBox { int x0, y0, x1, y1; };
__device__ __forceinline__ PixelBox square_coverage(float xw, float yw, float half, int w, int h) {
  return {max((int)ceilf((xw - half) - 0.5f), 0), max((int)ceilf((yw - half) - 0.5f), 0),
          min((int)ceilf((xw + half) - 0.5f) - 1, w - 1), min((int)ceilf((yw + half) - 0.5f) - 1, h - 1)};
}

// clip the segment a -> b against one plane (inside: dist >= 0); false = nothing left
__device__ __forceinline__ bool clip_plane(float4& a, float4& b, float da, float db) {
  if (!(da >= 0.0f) && !(db >= 0.0f)) return false;
  if (!(da >= 0.0f)) {
    const float t = da / (da - db);
    a = make_float4(a.x + (b.x - a.x) * t, a.y + (b.y - a.y) * t, a.z + (b.z - a.z) * t, a.w + (b.w - a.w) * t);
  } else if (!(db >= 0.0f)) {
    const float t = db / (db - da);
    b = make_float4(b.x + (a.x - b.x) * t, b.y + (a.y - b.y) * t, b.z + (a.z - b.z) * t, b.w + (a.w - b.w) * t);
  }
  return true;
}

// The set-up of a clipped segment: window coordinates, major / minor axis, and the conservative range [lo, hi] of pixel columns (rows) whose
// centres can lie on it.  false = nothing to walk.
struct LineSetup {
  float s0, s1, o0, o1, az, bz;                                          // major start / end, minor start / end, depth start / end
  int lo, hi, xmajor;
};
__device__ __forceinline__ bool overlay_line_setup(float4 a, float4 b, int w, int h, int width, LineSetup& L) {
  if (!clip_plane(a, b, a.z + a.w, b.z + b.w) || !clip_plane(a, b, a.w - a.z, b.w - b.z)) return false;   // near, then far
  if (!(a.w > 0.0f) || !(b.w > 0.0f)) return false;
  const float3 wa = clip_to_window(a, w, h), wb = clip_to_window(b, w, h);
  const bool xmajor = fabsf(wb.x - wa.x) >= fabsf(wb.y - wa.y);
  float s0 = xmajor ? wa.x : wa.y, s1 = xmajor ? wb.x : wb.y, o0 = xmajor ? wa.y : wa.x, o1 = xmajor ? wb.y : wb.x;
  if (width > 1) {
    const float shift = 0.5f * (float)(width - 1);
    o0 -= shift; o1 -= shift;
  }
  const int n_major = xmajor ? w : h;
  const float lo = fmaxf(floorf(fminf(s0, s1)) - 1.0f, 0.0f), hi = fminf(ceilf(fmaxf(s0, s1)) + 1.0f, (float)(n_major - 1));
  if (!(lo <= hi)) return false;
  L.s0 = s0; L.s1 = s1; L.o0 = o0; L.o1 = o1; L.az = wa.z; L.bz = wb.z;
  L.lo = (int)lo; L.hi = (int)hi; L.xmajor = xmajor ? 1 : 0;
  return true;
}
// ... and the fragment(s) of pixel column (row) i of such a segment
__device__ __forceinline__ void overlay_line_fragment(float s0, float s1, float o0, float o1, float az, float bz, bool xmajor, int i, int w, int h, int width,
                                                      uint32_t id, const float* __restrict__ fb_d, unsigned long long* __restrict__ key) {
  const float c = (float)i + 0.5f;
  if (!(s1 > s0 ? (c >= s0 && c < s1) : (c <= s0 && c > s1))) return;
  const float ds = s1 - s0, dm = o1 - o0;
  const float t = (c - s0) / ds;
  const float m = floorf(o0 + dm * t);
  // the depth is that of the fragment's centre projected onto the segment (GL 4.4 eq. 14.5, 14.6), not that of the line where it crosses column c
  const float tz = ((c - s0) * ds + ((m + 0.5f) - o0) * dm) / (ds * ds + dm * dm);
  float z = az + (bz - az) * tz;
  if (z != z) return;
  z = z > 0.0f ? (z < 1.0f ? z : 1.0f) : 0.0f;                            // the depth range [0, 1]
  const int n_minor = xmajor ? h : w;
  for (int r = 0; r < width; ++r) {
    const float mr = m + (float)r;
    if (!(mr >= 0.0f && mr < (float)n_minor)) continue;
    const int px = xmajor ? i : (int)mr, py = xmajor ? (int)mr : i;
    overlay_fragment(fb_d, key, py * w + px, z, id);
  }
}
// One segment between the clip-space points a -> b, walked by the 64 lanes of a wave: near, then far clip, then the diamond exit for
// width 1 -- an x-major line makes one fragment per pixel column whose centre c lies in [start, end) along the line's direction, in the row
// floor(y(c)); y-major the same with rows.  Wider lines (GL 4.4 section 14.5.2.2, aliased): the segment moves by -(width - 1) / 2 in its
// minor direction, is walked by the same rule, and each of its fragments becomes `width` fragments upwards in the minor direction at that
// fragment's depth, each dropped on its own outside the view.
__device__ __forceinline__ void overlay_line(float4 a, float4 b, int w, int h, int width, uint32_t id, int lane, const float* __restrict__ fb_d,
                                             unsigned long long* __restrict__ key) {
  LineSetup L;
  if (!overlay_line_setup(a, b, w, h, width, L)) return;
  for (int i = L.lo + lane; i <= L.hi; i += 64) overlay_line_fragment(L.s0, L.s1, L.o0, L.o1, L.az, L.bz, L.xmajor != 0, i, w, h, width, id, fb_d, key);
}

}  // namespace rr
