// Mesh component measures (tsdf_mesh_component_measures / _filter_components_measured; include/rgbd_recon_hip.h has the definition, mesh_measure.hpp the
// arithmetic): per component of the labelled mesh the bounds and the sum of its vertices' grid coordinates, the sum of its triangles' doubled areas and
// of their six-fold signed volumes -- all integers, so the result does not depend on the order in which the adds arrive: two runs give identical bytes.
//
// Three launches, no host wait between them.
// Vertices.  One lane per vertex, eight vertices per lane: the 12-byte position row is quantised ONCE, the packed 64-bit coordinate goes to a scratch
//   array, and {~min[3], max[3], sum[3]} is aggregated per run of equal components and flushed with atomicMax (32-bit) and 64-bit atomicAdd.  The row's
//   q_min holds the COMPLEMENT of the minimum until the finish launch, so that zeroed rows are the identity of every field and one memset initialises them.
// Triangles.  One lane per triangle, eight per lane: 12 bytes of indices, three 8-byte gathers from the packed array (not three 12-byte fp32 rows
//   quantised again per triangle: a vertex is used by six triangles), the exact a2 and v6, and {a2, v6's low 32 bits, v6 >> 32} aggregated per run and
//   flushed with three 64-bit adds.  The two halves of v6 are summed apart: each stays far inside 64 bits for 2^32 triangles.
// Finish.  One lane per component: q_min complemented back, the two partial sums of v6 joined into the canonical 128-bit pair.
//
// Run aggregation is the point of the first two kernels (mesh_cc_dev.hpp: adds to one address serialise at about 11 ns each, and one component usually
// holds almost everything).  It is cc_run_add / cc_run_finish generalised from a count to a small struct:
//   a lane first merges its own eight elements while they are of one component (no cross-lane work at all);
//   when some lane's component changes, and at the end, the wave reduces the lanes of each distinct component (xor shuffles over a masked copy) into the
//   wave's run, kept in registers: merged where the component is the run's, else the run is flushed -- one set of adds per run per wave;
//   at the end the four waves' runs meet in LDS, equal neighbours are merged, and thread 0 flushes: a workgroup inside one component issues ONE set.
// No float atomics, no compare-and-swap loops, nothing waits for another lane.
#include "tsdf_common.hpp"
#include "mesh_cc_dev.hpp"
#include "mesh_measure.hpp"

// RR_MM_LANE_TIER 0 builds the form without the lane's own tier (every element goes to the wave's reduction at once), for comparison: at 512^3 culled / 4 streams
// the three launches take 0.176 ms so and 0.164 ms with the tier (profiles/mesh_component_measures_lane_tier_ab_c2.json).
#ifndef RR_MM_LANE_TIER
#define RR_MM_LANE_TIER 1
#endif

namespace rr {

constexpr int kMmPerThread = 8, kMmPerBlock = kCcThreads * kMmPerThread;
typedef unsigned long long mm_u64;

// ---- what is aggregated.  Every field's identity is 0: `A{}` is the empty aggregate.
struct MmVertexAgg {
  uint32_t inv_min[3], top[3]; mm_u64 sum[3];
  __device__ __forceinline__ void merge(const MmVertexAgg& o) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { inv_min[a] = ::max(inv_min[a], o.inv_min[a]); top[a] = ::max(top[a], o.top[a]); sum[a] += o.sum[a]; }
  }
  __device__ __forceinline__ MmVertexAgg shfl_xor(int o) const {
    MmVertexAgg r;
#pragma unroll
    for (int a = 0; a < 3; ++a) { r.inv_min[a] = (uint32_t)__shfl_xor((int)inv_min[a], o); r.top[a] = (uint32_t)__shfl_xor((int)top[a], o); r.sum[a] = __shfl_xor(sum[a], o); }
    return r;
  }
  __device__ __forceinline__ void flush(tsdf_mesh_component_measure* row) const {
#pragma unroll
    for (int a = 0; a < 3; ++a) { atomicMax(&row->q_min[a], inv_min[a]); atomicMax(&row->q_max[a], top[a]); atomicAdd((mm_u64*)&row->sum_q[a], sum[a]); }
  }
};
struct MmTriangleAgg {
  mm_u64 a2, lo, hi;                                                      // hi: two's complement, the adds wrap as the signed sum does
  __device__ __forceinline__ void merge(const MmTriangleAgg& o) { a2 += o.a2; lo += o.lo; hi += o.hi; }
  __device__ __forceinline__ MmTriangleAgg shfl_xor(int o) const { return MmTriangleAgg{__shfl_xor(a2, o), __shfl_xor(lo, o), __shfl_xor(hi, o)}; }
  __device__ __forceinline__ void flush(tsdf_mesh_component_measure* row) const {
    atomicAdd((mm_u64*)&row->area2, a2); atomicAdd((mm_u64*)&row->volume6_lo, lo); atomicAdd((mm_u64*)&row->volume6_hi, hi);
  }
};

// ---- a wave's run (wave-uniform values) and its life
template <typename A> struct MmRun { uint32_t component, has; A agg; };
template <typename A>
__device__ __forceinline__ void mm_run_flush(tsdf_mesh_component_measure* rows, const MmRun<A>& run) {
  if (run.has && (threadIdx.x & 63) == 0) run.agg.flush(rows + run.component);
}
// every lane of the wave calls it; `mine` counts where valid
template <typename A>
__device__ __forceinline__ void mm_run_add(tsdf_mesh_component_measure* rows, MmRun<A>& run, uint32_t component, const A& mine, bool valid) {
  unsigned long long todo = __ballot(valid);
  while (todo) {                                                          // (uniform: at most 64 turns, one when the wave lies inside one component)
    const uint32_t c = (uint32_t)__shfl((int)component, __ffsll(todo) - 1);
    const bool member = valid && component == c;
    const unsigned long long same = __ballot(member);
    A total = member ? mine : A{};
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) total.merge(total.shfl_xor(o));
    if (run.has && c == run.component) run.agg.merge(total);
    else { mm_run_flush(rows, run); run.component = c; run.has = 1u; run.agg = total; }
    todo &= ~same;
  }
}
// every lane of the workgroup calls it
template <typename A>
__device__ __forceinline__ void mm_run_finish(tsdf_mesh_component_measure* rows, const MmRun<A>& run, MmRun<A>* s_run) {
  if ((threadIdx.x & 63) == 0) s_run[threadIdx.x >> 6] = run;
  __syncthreads();
  if (threadIdx.x != 0) return;
  MmRun<A> acc = s_run[0];
  for (int w = 1; w < kCcThreads / 64; ++w) {
    const MmRun<A> r = s_run[w];
    if (!r.has) continue;
    if (acc.has && r.component == acc.component) acc.agg.merge(r.agg);
    else { mm_run_flush(rows, acc); acc = r; }
  }
  mm_run_flush(rows, acc);
}
// a lane's own elements: merged in registers while they are of one component; the wave steps in when a lane's component changes
template <typename A> struct MmLane { uint32_t component; bool has; A agg; };
template <typename A>
__device__ __forceinline__ void mm_lane_add(tsdf_mesh_component_measure* rows, MmRun<A>& run, MmLane<A>& lane, uint32_t component, const A& mine, bool valid) {
#if RR_MM_LANE_TIER
  if (__any(valid && lane.has && component != lane.component)) { mm_run_add(rows, run, lane.component, lane.agg, lane.has); lane.has = false; lane.agg = A{}; }
  if (valid) { lane.component = component; lane.has = true; lane.agg.merge(mine); }
#else
  mm_run_add(rows, run, component, mine, valid);
#endif
}

// ---- 1. vertices
__global__ __launch_bounds__(kCcThreads) void k_mm_vertices(MeshMeasureGeometry G, const float* __restrict__ pos, const uint32_t* __restrict__ vertex_component, uint32_t nv,
                                                            uint32_t n_components, mm_u64* __restrict__ packed, tsdf_mesh_component_measure* rows) {
  __shared__ MmRun<MmVertexAgg> s_run[kCcThreads / 64];
  MmRun<MmVertexAgg> run{};
  MmLane<MmVertexAgg> lane{};
  for (int k = 0; k < kMmPerThread; ++k) {
    const size_t v = (size_t)blockIdx.x * kMmPerBlock + (size_t)k * kCcThreads + threadIdx.x;
    bool valid = v < nv;
    uint32_t c = 0;
    MmVertexAgg mine{};
    if (valid) {
      uint32_t q[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) q[a] = measure_quantise(pos[v * 3 + a], G.bbox_min[a], G.scale);
      packed[v] = measure_pack(q[0], q[1], q[2]);
      c = vertex_component[v];
      valid = c < n_components;                                            // (the labelling writes no other)
#pragma unroll
      for (int a = 0; a < 3; ++a) { mine.inv_min[a] = ~q[a]; mine.top[a] = q[a]; mine.sum[a] = q[a]; }
    }
    mm_lane_add(rows, run, lane, c, mine, valid);
  }
  mm_run_add(rows, run, lane.component, lane.agg, lane.has);
  mm_run_finish(rows, run, s_run);
}

// ---- 2. triangles (behind the vertices' launch boundary: plain reads of packed)
__global__ __launch_bounds__(kCcThreads) void k_mm_triangles(const uint32_t* __restrict__ tri, size_t nt, const uint32_t* __restrict__ triangle_component, uint32_t nv,
                                                             uint32_t n_components, const mm_u64* __restrict__ packed, tsdf_mesh_component_measure* rows) {
  __shared__ MmRun<MmTriangleAgg> s_run[kCcThreads / 64];
  MmRun<MmTriangleAgg> run{};
  MmLane<MmTriangleAgg> lane{};
  for (int k = 0; k < kMmPerThread; ++k) {
    const size_t t = (size_t)blockIdx.x * kMmPerBlock + (size_t)k * kCcThreads + threadIdx.x;
    bool valid = t < nt;
    uint32_t c = 0;
    MmTriangleAgg mine{};
    if (valid) {
      const uint32_t i0 = tri[t * 3], i1 = tri[t * 3 + 1], i2 = tri[t * 3 + 2];
      c = triangle_component[t];
      valid = c < n_components;
      if (i0 < nv && i1 < nv && i2 < nv) {                                 // (an index no extract and no keep writes: the triangle measures nothing)
        const MeasureTriangle m = measure_triangle(packed[i0], packed[i1], packed[i2]);
        mine.a2 = m.a2; mine.lo = measure_v6_lo(m.v6); mine.hi = (mm_u64)measure_v6_hi(m.v6);
      }
    }
    mm_lane_add(rows, run, lane, c, mine, valid);
  }
  mm_run_add(rows, run, lane.component, lane.agg, lane.has);
  mm_run_finish(rows, run, s_run);
}

// ---- 3. finish: the canonical row.  A component without triangles keeps area2 = volume6 = 0.
__global__ __launch_bounds__(kCcThreads) void k_mm_finish(tsdf_mesh_component_measure* __restrict__ rows, uint32_t n_components) {
  const size_t c = (size_t)blockIdx.x * kCcThreads + threadIdx.x;
  if (c >= n_components) return;
  tsdf_mesh_component_measure r = rows[c];
#pragma unroll
  for (int a = 0; a < 3; ++a) r.q_min[a] = ~r.q_min[a];
  measure_v6_join(r.volume6_lo, r.volume6_hi, &r.volume6_lo, &r.volume6_hi);
  r.reserved = 0;
  rows[c] = r;
}
// ---- the keep rule, on final rows
__global__ __launch_bounds__(kCcThreads) void k_mm_keep(const tsdf_mesh_component_measure* __restrict__ rows, const tsdf_mesh_component* __restrict__ table, uint32_t n_components,
                                                        tsdf_mesh_measure_rule rule, uint8_t* __restrict__ keep) {
  const size_t c = (size_t)blockIdx.x * kCcThreads + threadIdx.x;
  if (c < n_components) keep[c] = measure_keeps(rows[c], table[c].n_triangles, rule) ? 1 : 0;
}

// ---- launchers
void launch_mesh_measures(hipStream_t st, const MeshMeasureGeometry& G, const float* pos, const uint32_t* tri, uint32_t nv, size_t nt, const uint32_t* vertex_component,
                          const uint32_t* triangle_component, uint32_t n_components, unsigned long long* packed, tsdf_mesh_component_measure* rows) {
  const auto grid = [](size_t n, size_t per) { return dim3((unsigned)((n + per - 1) / per)); };
  hipLaunchKernelGGL(k_mm_vertices, grid(nv, kMmPerBlock), dim3(kCcThreads), 0, st, G, pos, vertex_component, nv, n_components, packed, rows);
  if (nt) hipLaunchKernelGGL(k_mm_triangles, grid(nt, kMmPerBlock), dim3(kCcThreads), 0, st, tri, nt, triangle_component, nv, n_components, packed, rows);
  hipLaunchKernelGGL(k_mm_finish, grid(n_components, kCcThreads), dim3(kCcThreads), 0, st, rows, n_components);
}
void launch_mesh_measure_keep(hipStream_t st, const tsdf_mesh_component_measure* rows, const tsdf_mesh_component* table, uint32_t n_components,
                              const tsdf_mesh_measure_rule& rule, uint8_t* keep) {
  if (n_components) hipLaunchKernelGGL(k_mm_keep, dim3((n_components + kCcThreads - 1) / kCcThreads), dim3(kCcThreads), 0, st, rows, table, n_components, rule, keep);
}

}  // namespace rr
