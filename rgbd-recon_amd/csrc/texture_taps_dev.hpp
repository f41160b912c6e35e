// Device side of the texture taps, shared by k_texture_taps.hip (the fp32 records at caller-given points) and k_mesh_stream_taps.hip (the packed taps of a
// streamed frame): the per-stream evaluation of the header's "texture taps" section through blend_colors()' own device functions (sampling.hpp), and
// the 8-byte packed tap of "mesh streaming: texture taps in the frame".
#pragma once
#include "sampling.hpp"

namespace rr {

// what one (point, stream) pair evaluates to: pc = texture(cv_xyz_inv, u).xyz, pcol = texture(cv_uv, pc).xy, the nearest depth at pc.xy,
// dist = |depth - pc.z|, quality = dist < limit ? the linear quality at pc.xy : 0   (every tap index is clamped into its array, whatever u and pc hold)
struct TapValues { float3 pc; float2 pcol; float depth, dist, quality; };
__device__ __forceinline__ TapValues texture_tap_values(const StreamLut& L, const FrameImages& F, int stream, float limit, float3 u) {
  TapValues t;
  t.pc = tex3d_rgba_xyz(L.inv, L.inv_res, u.x, u.y, u.z);
  t.pcol = tex3d_rg(L.uv, L.uv_res, t.pc.x, t.pc.y, t.pc.z);
  const Dqs q = dqs_fetch(F, stream, t.pc.x, t.pc.y);
  t.depth = dqs_depth(q);
  t.dist = fabsf(t.depth - t.pc.z);
  t.quality = 0.0f;
  if (t.dist < limit) t.quality = dqs_quality(q);
  return t;
}

// the packed tap's coordinate: the packed vertex's position rule (mesh_dev.hpp: unorm16) -- the clamp maps NaN to 0, the product in fp32, half-way to even
__device__ __forceinline__ uint32_t tap_unorm16(float x) { return (uint32_t)__float2int_rn(fminf(fmaxf(x, 0.0f), 1.0f) * 65535.0f); }
// the packed tap's weights: IEEE binary16 of an fp32, round to nearest even, overflow to +-inf, subnormals kept (the conversion instruction under the
// kernel's default mode, which keeps binary16 denormals); every NaN becomes 0x7E00, whatever its sign and payload
__device__ __forceinline__ uint32_t tap_half(float x) {
  const _Float16 h = (_Float16)x;
  return x != x ? 0x7E00u : (uint32_t)__builtin_bit_cast(unsigned short, h);
}
// {u, v, quality_h, dist_h}, little endian, as two dwords
__device__ __forceinline__ uint2 pack_tap(float2 pcol, float quality, float dist) {
  return make_uint2(tap_unorm16(pcol.x) | (tap_unorm16(pcol.y) << 16), tap_half(quality) | (tap_half(dist) << 16));
}

}  // namespace rr
