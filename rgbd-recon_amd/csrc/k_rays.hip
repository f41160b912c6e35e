// Ray queries (tsdf_cast_rays / tsdf_cast_rays_dev / tsdf_view_rays; include/rgbd_recon_hip.h has the definition): caller-given rays marched
// through the fused volume by the draw's rule (tsdf_raymarch.fs:62-114 with skipSpace off), the hit's normal and colour on request.  The reference has no
// counterpart (its GUI picks nothing); the entries are built on what the draw restates: intersectBox (:363-374), the march (:89-110), get_gradient
// (:140-149), blendColors (:295-330) and vol_to_world (recon_integration.cpp:66-72).
//
// k_march / k_march_box (k_raymarch.hip) take their ray from the pixel grid and skip space either by a screen-space rasterisation of the bricks or by a
// leap the 64 neighbouring rays of a wave take together.  Neither means anything for rays that are no neighbours, so here everything is per lane:
//   k_rays_march    one lane per ray.  The ray comes in as two 16-byte loads and the answer leaves as two 16-byte stores.  Samples are fetched kRayBatch at a
//                   time (positions never depend on densities) and examined in order.  Empty space: for the next `run` samples the lane performs the
//                   reference's chain of additions FIRST, takes the tap indices of the run's first and last position with the filter's own arithmetic
//                   (axis_linear: the taps of the samples between lie between them, because a chain of additions of one step is monotonic per axis), and
//                   looks up the classes (sparse pool: slots) of the at most 2 x 2 x 2 tiles those taps touch.  All "every voxel is -limit": the samples
//                   are -limit (lerp(a, a, t) = a in fp32), so the run is accounted for and prev = -limit.  Anything else -- a mixed tile, a run that
//                   spans more than two tiles on an axis, a position beyond 1e6 or not finite -- and the lane fetches from the run's first position.  No estimate takes
//                   part: the positions tested are the positions sampled.
//   k_rays_surface  one lane per HIT, over the list k_rays_march compacted (one atomic per wave, as k_march -> k_shade): the 128-register blend_colors
//                   runs in dense waves and for hits only.  Results are indexed by ray number, so the list's order shows nowhere.
//   k_view_rays     the draw's own rays of a pixel rectangle, through pixel_dir_vol (ray_dev.hpp: the function k_march calls).
//   k_rays_march<., true> / k_rays_merge   a Z-slab context's part of a cast and the merge of the parts (tsdf_cast_rays_part, tsdf_merge_ray_parts_dev).
#include <cfloat>

#include "blend_dev.hpp"
#include "ray_dev.hpp"

namespace rr {

#ifndef RR_RAY_BATCH
#define RR_RAY_BATCH 4
#endif
constexpr int kRayBatch = RR_RAY_BATCH;      // samples in flight per lane
constexpr int kRayThreads = 256;

__device__ __forceinline__ bool ray_finite(float v) { return fabsf(v) <= FLT_MAX; }

// A position whose trilinear weights are proper numbers: beyond this the product with the resolution could overflow and a weight be NaN (as k_march_box's
// leap: such a position takes the fetching path, which restates the filter whatever it gives)
__device__ __forceinline__ bool ray_tame(float3 p) { return fabsf(p.x) < 1.0e6f && fabsf(p.y) < 1.0e6f && fabsf(p.z) < 1.0e6f; }
// every voxel a tap of the positions a .. b (the run's first and last sample; the chain between them is monotonic per axis) can read is -limit
// kPart (a slab's part cast): the caller has found a and b owned, so their taps lie at most one plane outside the owned layers, inside the halo; the
// test below restates it on the tile layers themselves, so that no lookup can index outside the stored [tz0, tz1) whatever the positions are.
template <bool kSparse, bool kPart = false>
__device__ __forceinline__ bool ray_run_clear(const Volume& V, float3 a, float3 b) {
  if (!(ray_tame(a) && ray_tame(b))) return false;
  const Axis ax = axis_linear(a.x, V.res[0]), ay = axis_linear(a.y, V.res[1]), az = axis_linear(a.z, V.res[2]);
  const Axis bx = axis_linear(b.x, V.res[0]), by = axis_linear(b.y, V.res[1]), bz = axis_linear(b.z, V.res[2]);
  const int lx = min(ax.i0, bx.i0) >> 3, ly = min(ay.i0, by.i0) >> 3, lz = min(az.i0, bz.i0) >> 3;
  const int hx = max(ax.i1, bx.i1) >> 3, hy = max(ay.i1, by.i1) >> 3, hz = max(az.i1, bz.i1) >> 3;
  if (hx - lx > 1 || hy - ly > 1 || hz - lz > 1) return false;       // more than two tiles on an axis: not looked up
  if (kPart && (lz < V.tz0 || hz >= V.tz1)) return false;            // a tile layer this context does not store: not looked up
  bool clear = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int tx = (k & 1) ? hx : lx, ty = (k & 2) ? hy : ly, tz = (k & 4) ? hz : lz;   // (tap indices are clamped into the grid: so are these)
    const uint32_t id = (uint32_t)__mul24(__mul24(tz - V.tz0, V.nty) + ty, V.ntx) + (uint32_t)tx;
    clear &= kSparse ? (V.slot[id] == kNoSlot) : (V.cls[id] == kTileMinus);
  }
  return clear;
}

// kPart: the part cast of a Z-slab context (tsdf_cast_rays_part; the header's "ray queries: slab parts"), as k_march has kPartial.  The lane examines
// the samples its context owns (sample_owned, ray_dev.hpp: the draw's rule) and nothing else:
//   - z is monotonic along a chain of additions of one step and the owner plane is monotonic in z, so the owned samples are ONE contiguous run.  The
//     samples in front of it cost only the reference's `pos += step`; behind it the lane stops (a miss reports max_n, which every slab computes alike).
//   - inside the run batches are fetched unconditionally with the clamped filter (tex3d_tsdf<kSparse>, not the kWhole form): an owned sample's taps lie
//     in the stored planes, and whatever else a batch touches is clamped into them and never examined.
//   - the hit's prev is sample k - 1's density: the lane's own when it examined that sample, else (the run's first sample, with samples in front of it)
//     fetched at pos_{k-1} from the halo, which is sized for a sample one step behind an owned one (grid_plan.hpp, above halo_layers_for).
//   - tile-class skipping stays.  A run is tested only when its first and last sample are both owned (then all between are), and ray_run_clear<., true>
//     refuses any tile layer outside the stored [tz0, tz1).  What cls and slot hold on halo layers (abi.cpp): the class array covers every STORED tile and
//     is created kTileMixed; TileState::cls points at the first INTEGRATED layer.  Under an exchanged halo integrate() computes the owned layers only,
//     tsdf_halo_unpack_dev copies voxels and no classes, so halo layers stay kTileMixed for good -- a run that touches one is fetched.  Under a
//     recomputed halo (the only form a sparse slab takes) the halo layers are integrated like owned ones: their class / slot is what integrate() left,
//     exact for the voxels the context itself stores and reads.  tsdf_upload_volume marks every integrated tile mixed.  So "clear" is only ever said of
//     voxels this context wrote as -limit: a wrong "clear" would change bits, a mixed class only costs a fetch.
// The kPart = false instantiations are the text they were: every addition is behind `if (kPart)`.
template <bool kSparse, bool kPart>
__global__ __launch_bounds__(kRayThreads) void k_rays_march(Volume V, RayCast Q, const float4* __restrict__ rays, float4* __restrict__ hits, float4* __restrict__ surf,
                                                            RayHitRec* __restrict__ list, uint32_t* __restrict__ list_count, unsigned long long* __restrict__ stats) {
  const uint32_t i = blockIdx.x * kRayThreads + threadIdx.x;
  const int ln = threadIdx.x & 63;
  const bool in = i < Q.n;
  float4 r0 = make_float4(0, 0, 0, 0), r1 = make_float4(0, 0, 0, 0);
  if (in) { r0 = rays[2 * i]; r1 = rays[2 * i + 1]; }
  const float limit = V.limit, sd = limit * 0.5f;                       // sampleDistance, tsdf_raymarch.fs:34
  float3 o = make_float3(r0.x, r0.y, r0.z), d = make_float3(r1.x, r1.y, r1.z);
  const float t_min = r0.w, t_max = r1.w;
  if (!(Q.flags & TSDF_RAYS_UNIT_CUBE)) {
    o = make_float3((o.x - Q.bbox_min[0]) / Q.ext[0], (o.y - Q.bbox_min[1]) / Q.ext[1], (o.z - Q.bbox_min[2]) / Q.ext[2]);
    d = make_float3(d.x / Q.ext[0], d.y / Q.ext[1], d.z / Q.ext[2]);
  }
  const float len2 = d.x * d.x + d.y * d.y + d.z * d.z;                 // (normalize3's sum)
  const float len = sqrtf(len2);
  const bool valid = in && ray_finite(o.x) && ray_finite(o.y) && ray_finite(o.z) && ray_finite(d.x) && ray_finite(d.y) && ray_finite(d.z) &&
                     len > 0.0f && ray_finite(len) && !(t_min != t_min);
  const float3 step = ray_step(d, sd);
  uint32_t max_n = 0, status = valid ? 0u : TSDF_RAY_INVALID;
  float3 pos = make_float3(0, 0, 0);
  if (valid) {
    const CubeSpan span = unit_cube_span(o, step);
    if (!span.hit) status = TSDF_RAY_OUTSIDE;
    else {
      float t_near = span_near(span.t0), t1 = span.t1;
      // the caller's interval, from units of `dir` to steps: one step is sd / len of them
      const float per = len / sd, s_min = t_min * per, s_max = t_max * per;
      if (s_min > t_near) t_near = s_min;
      if (s_max < t1) t1 = s_max;
      if (!(t_near <= t1)) status = TSDF_RAY_OUTSIDE;
      else {
        pos = ray_at(o, step, t_near);
        max_n = (uint32_t)fminf(span_samples(t_near, t1), Q.n_cap);
      }
    }
  }
  // The march, :89-110: positions by chained additions, dens > 0 the hit test, prev starts at -limit
  float prev = -limit;
  uint32_t n = 0, fetched = 0;
  bool hit = false, try_skip = true;
  float3 hit_pos = pos;
  float hit_d = 0.0f;
  const float ml = -limit;
  uint32_t owned = 0;                                                   // kPart: owned samples accounted for (n counts the definition's, a neighbour's included)
  bool prev_mine = true;                                                // kPart: prev is sample n - 1's density (or -limit at n = 0); false: that sample is a neighbour's
  float3 pos_prev = pos;
  if (kPart) {
    while (n < max_n && !sample_owned(V, pos.z)) {                      // in front of the run: the additions alone
      pos_prev = pos;
      pos = ray_advance(pos, step);
      n += 1; prev_mine = false;
    }
  }
  while (n < max_n && !hit) {
    if (kPart && !sample_owned(V, pos.z)) break;                        // behind the run: nothing further is ours
    if (try_skip) {
      const uint32_t m = min((uint32_t)Q.run, max_n - n);
      float3 e = pos;
      for (uint32_t k = 1; k < m; ++k) e = ray_advance(e, step);
      if ((!kPart || sample_owned(V, e.z)) && ray_run_clear<kSparse, kPart>(V, pos, e)) {
        pos = ray_advance(e, step);
        n += m; prev = ml;
        if (kPart) { owned += m; prev_mine = true; }
        continue;
      }
      try_skip = false;
    }
    float3 p[kRayBatch];
    float dv[kRayBatch];
    p[0] = pos;
#pragma unroll
    for (int k = 1; k < kRayBatch; ++k) p[k] = ray_advance(p[k - 1], step);
#pragma unroll
    for (int k = 0; k < kRayBatch; ++k) dv[k] = tex3d_tsdf<kSparse, !kPart>(V, p[k].x, p[k].y, p[k].z);   // unconditional: taps are clamped into the allocation
    bool all_clear = true;
    bool mine = true;                                                   // kPart: p[0] is owned; the first sample that is not ends the run
#pragma unroll
    for (int k = 0; k < kRayBatch; ++k) {
      if (kPart) mine = mine && sample_owned(V, p[k].z);
      if (!hit && n < max_n && mine) {
        n += 1; fetched += 1;
        all_clear &= dv[k] == ml;
        if (dv[k] > 0.0f) { hit = true; hit_pos = p[k]; hit_d = dv[k]; }   // (a NaN density compares as no hit, as in the draw)
        else { prev = dv[k]; if (kPart) prev_mine = true; }
        if (kPart) owned += 1;
      }
    }
    if (kPart && !mine) break;                                          // the batch left the slab
    if (!hit) pos = ray_advance(p[kRayBatch - 1], step);
    try_skip = all_clear;                                               // back in empty space: look at the classes again
  }
  if (kPart) {
    if (!hit) n = max_n;                                                // a part's miss: max_n, identical on every slab
    else if (!prev_mine) prev = tex3d_tsdf<kSparse>(V, pos_prev.x, pos_prev.y, pos_prev.z);   // sample n - 1 is a neighbour's: read it from the halo
  }
  float3 pu = make_float3(0, 0, 0), pw = make_float3(0, 0, 0);
  float t = -1.0f;
  if (hit) {
    pu = refine_hit(hit_pos, step, prev, hit_d);
    t = ((pu.x - o.x) * d.x + (pu.y - o.y) * d.y + (pu.z - o.z) * d.z) / len2;
    pw = pu;
    if (!(Q.flags & TSDF_RAYS_UNIT_CUBE)) pw = vol_to_world(Q.bbox_min, pu, Q.ext[0], Q.ext[1], Q.ext[2]);
    status |= TSDF_RAY_HIT;
  }
  if (in) {
    hits[2 * i] = make_float4(pw.x, pw.y, pw.z, t);
    hits[2 * i + 1] = make_float4(__uint_as_float(n), __uint_as_float(status), 0.0f, 0.0f);
    if (surf && !hit) { surf[2 * i] = make_float4(0, 0, 0, 0); surf[2 * i + 1] = make_float4(0, 0, 0, 0); }
  }
  // compact the hits of this wave into the list (one atomic per wave): what k_rays_surface runs over
  const unsigned long long hm = __ballot(hit);
  if (surf && hm) {
    const uint32_t base = wave_append(list_count, hm, ln);
    if (hit) {
      RayHitRec h;
      h.x = pu.x; h.y = pu.y; h.z = pu.z; h.ray = i;
      list[base + wave_rank(hm, ln)] = h;   // (base + rank < hits of the launch <= Q.n <= the list's capacity)
    }
  }
  // tsdf_ray_stats: hits, samples accounted for, samples fetched
  uint32_t sa = kPart ? owned : n, sf = fetched;                        // (a part accounts for the samples it owns)
  for (int s = 32; s; s >>= 1) { sa += (uint32_t)__shfl_xor((int)sa, s); sf += (uint32_t)__shfl_xor((int)sf, s); }   // (a wave's sums: 64 x max_n, far below 2^32 at n_cap)
  if (ln == 0) {
    if (hm) atomicAdd(&stats[0], (unsigned long long)__popcll(hm));
    if (sa) { atomicAdd(&stats[1], (unsigned long long)sa); atomicAdd(&stats[2], (unsigned long long)sf); }
  }
}

// the surface at the hits: the mesh section's normal (tsdf_gradient, world_normal: sampling.hpp) and colour at the hit's unit-cube position
template <bool kSparse>
__global__ __launch_bounds__(kRayThreads) void k_rays_surface(Volume V, StreamTable T, FrameImages F, RayCast Q, const RayHitRec* __restrict__ list,
                                                              const uint32_t* __restrict__ list_count, float4* __restrict__ surf) {
  const uint32_t j = blockIdx.x * kRayThreads + threadIdx.x;
  if (j >= *list_count) return;
  const RayHitRec h = list[j];
  const float3 u = make_float3(h.x, h.y, h.z);
  const float limit = V.limit, sd = limit * 0.5f;
  float4 nrm = make_float4(0, 0, 0, 0), col = make_float4(0, 0, 0, 0);
  if (Q.flags & TSDF_RAY_NORMALS) {
    const float3 nn = world_normal(tsdf_gradient<kSparse>(V, u, sd), Q.ext[0], Q.ext[1], Q.ext[2]);
    nrm = make_float4(nn.x, nn.y, nn.z, 0.0f);
  }
  if (Q.flags & TSDF_RAY_COLOURS) col = blend_colors(T, F, limit, u);
  surf[2 * h.ray] = nrm;
  surf[2 * h.ray + 1] = col;
}

// the draw's rays of the pixel rectangle (x0, y0, w, h), row-major: origin cam_vol, direction the un-normalised pixel_dir_vol of the pixel centre
__global__ __launch_bounds__(kRayThreads) void k_view_rays(ViewParams P, int x0, int y0, int w, int n, float4* __restrict__ rays) {
  const int i = blockIdx.x * kRayThreads + threadIdx.x;
  if (i >= n) return;
  const int px = x0 + i % w, py = y0 + i / w;
  const float3 d = pixel_dir_vol(P, (float)px + 0.5f, (float)py + 0.5f);
  rays[2 * i] = make_float4(P.cam_vol[0], P.cam_vol[1], P.cam_vol[2], 0.0f);
  rays[2 * i + 1] = make_float4(d.x, d.y, d.z, __int_as_float(0x7f800000));
}

// The merge of K slabs' parts (tsdf_merge_ray_parts_dev): one lane per ray.  The decision reads the K second halves of the hit records ({n_samples,
// status, pad}: one 16-byte load each) -- the part with TSDF_RAY_HIT and the smallest n_samples, part 0 when none hit; no two parts tie, a sample has one
// owner --, then the winner's first half and its two surface halves move as 16-byte loads and stores.  No atomics, no LDS; parts are stride records apart.
__global__ __launch_bounds__(kRayThreads) void k_rays_merge(const float4* __restrict__ hit_parts, const float4* __restrict__ surf_parts, uint32_t parts, uint32_t n,
                                                            unsigned long long stride, float4* __restrict__ hits, float4* __restrict__ surf) {
  const uint32_t i = blockIdx.x * kRayThreads + threadIdx.x;
  if (i >= n) return;
  const size_t at = 2 * (size_t)i, pitch = 2 * (size_t)stride;          // in 16-byte halves
  uint32_t win = 0, best = 0xffffffffu;
  float4 tail = hit_parts[at + 1];
  for (uint32_t k = 0; k < parts; ++k) {
    const float4 t = hit_parts[(size_t)k * pitch + at + 1];
    const uint32_t ns = __float_as_uint(t.x), status = __float_as_uint(t.y);
    if ((status & TSDF_RAY_HIT) && ns < best) { best = ns; win = k; tail = t; }
  }
  const size_t from = (size_t)win * pitch + at;
  hits[at] = hit_parts[from];
  hits[at + 1] = tail;
  if (surf) { surf[at] = surf_parts[from]; surf[at + 1] = surf_parts[from + 1]; }
}

// the one launcher of k_rays_march: part = a Z-slab context's part cast.  (The two names below are what the binding selects between; they only set the flag.)
static void launch_rays_march_as(bool part, hipStream_t st, const Volume& V, const RayCast& Q, const tsdf_ray* rays, tsdf_ray_hit* hits, tsdf_ray_surface* surf,
                                 RayHitRec* list, uint32_t* list_count, unsigned long long* stats) {
  const auto k = !part ? (V.slot ? k_rays_march<true, false> : k_rays_march<false, false>) : (V.slot ? k_rays_march<true, true> : k_rays_march<false, true>);
  hipLaunchKernelGGL(k, dim3((Q.n + kRayThreads - 1) / kRayThreads), dim3(kRayThreads), 0, st, V, Q, (const float4*)rays, (float4*)hits, (float4*)surf, list, list_count, stats);
}
void launch_rays_march(hipStream_t st, const Volume& V, const RayCast& Q, const tsdf_ray* rays, tsdf_ray_hit* hits, tsdf_ray_surface* surf, RayHitRec* list,
                       uint32_t* list_count, unsigned long long* stats) { launch_rays_march_as(false, st, V, Q, rays, hits, surf, list, list_count, stats); }
void launch_rays_march_part(hipStream_t st, const Volume& V, const RayCast& Q, const tsdf_ray* rays, tsdf_ray_hit* hits, tsdf_ray_surface* surf, RayHitRec* list,
                            uint32_t* list_count, unsigned long long* stats) { launch_rays_march_as(true, st, V, Q, rays, hits, surf, list, list_count, stats); }
void launch_rays_merge(hipStream_t st, const tsdf_ray_hit* hit_parts, const tsdf_ray_surface* surf_parts, uint32_t parts, uint32_t n, uint64_t stride_records,
                       tsdf_ray_hit* hits, tsdf_ray_surface* surf) {
  hipLaunchKernelGGL(k_rays_merge, dim3((n + kRayThreads - 1) / kRayThreads), dim3(kRayThreads), 0, st, (const float4*)hit_parts, (const float4*)surf_parts, parts, n,
                     (unsigned long long)stride_records, (float4*)hits, (float4*)surf);
}
void launch_rays_surface(hipStream_t st, const Volume& V, const StreamTable& T, const FrameImages& F, const RayCast& Q, const RayHitRec* list,
                         const uint32_t* list_count, tsdf_ray_surface* surf) {
  const dim3 g((Q.n + kRayThreads - 1) / kRayThreads), b(kRayThreads);   // (the hit count stays on the device: lanes past it return at once)
  if (V.slot) hipLaunchKernelGGL(k_rays_surface<true>, g, b, 0, st, V, T, F, Q, list, list_count, (float4*)surf);
  else hipLaunchKernelGGL(k_rays_surface<false>, g, b, 0, st, V, T, F, Q, list, list_count, (float4*)surf);
}
void launch_view_rays(hipStream_t st, const ViewParams& P, int x0, int y0, int w, int h, tsdf_ray* rays) {
  const int n = w * h;
  hipLaunchKernelGGL(k_view_rays, dim3((n + kRayThreads - 1) / kRayThreads), dim3(kRayThreads), 0, st, P, x0, y0, w, n, (float4*)rays);
}

}  // namespace rr
