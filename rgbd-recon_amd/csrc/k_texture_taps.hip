// Texture taps (tsdf_texture_taps / tsdf_texture_taps_dev / tsdf_mesh_texture_taps; include/rgbd_recon_hip.h has the definition): per point and
// stream the colour-image coordinates and the two numbers blendColors (tsdf_raymarch.fs:295-330) weights that read with -- what blend_colors()
// (blend_dev.hpp) forms per stream and throws away.  The reference has no counterpart: its client runs blendColors per pixel against the colour images.
//
// blend_colors() keeps four streams' taps in flight in one lane because it has to accumulate in stream order.  The taps themselves are independent per
// stream, so here a lane is one (point, stream) pair:
//   three dword loads of the point, the 8 taps of cv_xyz_inv, the 8 taps of cv_uv and the 2 x 2 footprint of the packed depth / quality image through
//   the same device functions as blend_colors() (sampling.hpp), ONE 16-byte store of the record and a second one for the sensor record on request.
//   No LDS, no barrier, no scratch.
// Which pair a lane takes: blockIdx.y is the stream and a wave holds 64 neighbouring points, so the stream's LUT pointers and resolutions are scalars and
// the 64 lanes read one LUT next to each other; the records of a wave are then 16 bytes every 16 * N bytes.  The other mapping -- g = point * N + stream,
// a wave's 64 records 1 KiB contiguous, the LUT pointers fetched per lane from the by-value StreamTable -- was built and measured too: byte-equal, 40 %
// slower without sensor records on a mesh, 5 % faster with them (DESIGN.md "Texture taps" has both rows).
// tsdf_texture_tap_stats' two counts are taken per wave with a ballot and one vector atomic per wave and count, as k_rays_march does -- but into one of
// kTapStatSlots pairs of counters chosen by the wave's number: these waves are short, and a hundred thousand of them adding to one address took five
// times as long as everything else the launch does (texture_taps.hpp, DESIGN.md "Texture taps").
#include "texture_taps_dev.hpp"
#include "texture_taps.hpp"

namespace rr {

__global__ __launch_bounds__(kTapsThreads) void k_texture_taps(StreamTable T, FrameImages F, float limit, TapsLaunch Q, const float* __restrict__ xyz,
                                                               float4* __restrict__ taps, float4* __restrict__ sensor, unsigned long long* __restrict__ stats) {
  const uint32_t point = blockIdx.x * kTapsThreads + threadIdx.x, stream = blockIdx.y;   // (gridDim.y = T.n)
  const bool in = point < Q.n_points;
  bool evaluated = false;
  float quality = 0.0f;
  if (in) {
    const uint32_t g = point * (uint32_t)T.n + stream;                  // the record: [point][stream] (< 2^18 x 16)
    const float* __restrict__ p = xyz + 3 * (size_t)point;
    float3 u = make_float3(p[0], p[1], p[2]);
    if (!(Q.flags & TSDF_TAPS_UNIT_CUBE))                                // the ray section's mapping: the difference, then the division
      u = make_float3((u.x - Q.bbox_min[0]) / Q.ext[0], (u.y - Q.bbox_min[1]) / Q.ext[1], (u.z - Q.bbox_min[2]) / Q.ext[2]);
    // beyond 1e6 the product with a resolution could overflow and a filter weight be NaN (as ray_tame of k_rays.hip); a NaN or an infinity compares false
    evaluated = fabsf(u.x) < 1.0e6f && fabsf(u.y) < 1.0e6f && fabsf(u.z) < 1.0e6f;
    float4 tap = make_float4(0.0f, 0.0f, 0.0f, -1.0f), sen = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (evaluated) {                                                     // blend_colors()' per-stream values, by its own device functions
      const TapValues t = texture_tap_values(T.s[stream], F, (int)stream, limit, u);   // (texture_taps_dev.hpp: shared with the mesh ring's packed taps)
      quality = t.quality;
      tap = make_float4(t.pcol.x, t.pcol.y, t.quality, t.dist);
      sen = make_float4(t.pc.x, t.pc.y, t.pc.z, t.depth);
    }
    taps[g] = tap;                                                       // (point < n_points, stream < N: inside the launch's [points][N] records)
    if (sensor) sensor[g] = sen;
  }
  const unsigned long long with_quality = __ballot(evaluated && quality > 0.0f), skipped = __ballot(in && !evaluated);
  if ((threadIdx.x & 63) == 0) {                                          // (the wave's pair of counters: texture_taps.hpp says why there are many)
    unsigned long long* __restrict__ s = stats + tap_stat_word((blockIdx.y * gridDim.x + blockIdx.x) * (kTapsThreads / 64) + (threadIdx.x >> 6));
    if (with_quality) atomicAdd(&s[0], (unsigned long long)__popcll(with_quality));
    if (skipped) atomicAdd(&s[1], (unsigned long long)__popcll(skipped));
  }
}

void launch_texture_taps(hipStream_t st, const StreamTable& T, const FrameImages& F, float limit, const TapsLaunch& Q, const float* xyz, tsdf_texture_tap* taps,
                         tsdf_sensor_tap* sensor, unsigned long long* stats) {
  const dim3 g((uint32_t)tap_grid(Q.n_points), (uint32_t)T.n), b(kTapsThreads);   // (at most 2^18 points / 256 = 2^10 workgroups per stream)
  hipLaunchKernelGGL(k_texture_taps, g, b, 0, st, T, F, limit, Q, xyz, (float4*)taps, (float4*)sensor, stats);
}

}  // namespace rr
