// The union-find and the per-component counting the mesh components (k_mesh_components.hip), the streamed filter (k_mesh_stream_filter.hip) and the
// components of a Z-slab's part (k_mesh_slab_components.hip) share.
// k_mesh_components.hip's head explains why the labelling is defined although the arrival order is not; this is its text, as __device__ functions.
#ifndef RR_MESH_CC_DEV_HPP
#define RR_MESH_CC_DEV_HPP
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rr {

constexpr int kCcThreads = 256;

// ---- the global forest: parent[x] <= x, every write an atomicMin
__device__ __forceinline__ uint32_t cc_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t cc_min(uint32_t* p, uint32_t v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// the root above x, halving the path on the way (parent[x] = min(parent[x], grandparent): still an ancestor, still <= x).  x strictly decreases.
__device__ __forceinline__ uint32_t cc_find(uint32_t* parent, uint32_t x) {
  uint32_t p = cc_load(parent + x);
  while (p != x) {
    const uint32_t g = cc_load(parent + p);
    if (g != p) cc_min(parent + x, g);
    x = p; p = g;
  }
  return x;
}
// a ~ b.  max(a, b) strictly decreases from turn to turn, whatever the other lanes do.
__device__ __forceinline__ void cc_hook(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = cc_find(parent, a); b = cc_find(parent, b);
    if (a == b) return;
    const uint32_t hi = max(a, b), lo = min(a, b);
    const uint32_t old = cc_min(parent + hi, lo);
    if (old == hi) return;                                             // hi was a root: it hangs under lo now
    a = old; b = lo;                                                   // it was not any more: hi -> min(old, lo) stands, old ~ lo is what is left to do (both < hi)
  }
}

// ---- the hooks of one chunk, with a workgroup-local first pass.  Triangles are ordered by tile and a tile's triangles use vertices of the tile itself and
// of its +x / +y / +z neighbours only -- never a smaller index than the tile's own first vertex --, so a chunk of consecutive triangles touches a narrow
// window of indices above its smallest one.  The window [base, base + kCcWindow) gets a union-find of its own in LDS (the same algorithm on local
// indices); an edge with an end outside goes to the global forest directly.  Then every window vertex that is not a local root is hooked to its local
// root globally: the global forest connects what the chunk's edges connect, with one global hook per vertex where one lane per triangle would make two
// per triangle.
constexpr int kCcChunkPerThread = 4, kCcChunk = kCcThreads * kCcChunkPerThread, kCcWindow = 2048;
__device__ __forceinline__ uint32_t cc_local_find(uint32_t* s_parent, uint32_t x) {
  uint32_t p = __hip_atomic_load(s_parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  while (p != x) { x = p; p = __hip_atomic_load(s_parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  return x;
}
__device__ __forceinline__ void cc_local_hook(uint32_t* s_parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = cc_local_find(s_parent, a); b = cc_local_find(s_parent, b);
    if (a == b) return;
    const uint32_t hi = max(a, b), lo = min(a, b);
    const uint32_t old = __hip_atomic_fetch_min(s_parent + hi, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (old == hi) return;
    a = old; b = lo;
  }
}
// Every lane of the workgroup calls it (it holds barriers); the triangles are [first, first + kCcChunk) of tri[nt].  s_parent: kCcWindow words of LDS,
// s_min: one word per wave.  A workgroup that takes another chunk afterwards puts a __syncthreads() between the two calls.
// index_base: what the triangles' indices count from (a slab part's are global: k_mesh_slab_components.hip); the forest's index space is
// [0, nv) behind it, and an index below the base wraps past nv and is dropped with the triangle like any other the forest does not hold.
__device__ __forceinline__ void cc_hook_chunk(const uint32_t* __restrict__ tri, size_t nt, uint32_t* parent, uint32_t nv, size_t first, uint32_t* s_parent, uint32_t* s_min,
                                              uint32_t index_base = 0u) {
  uint32_t v[kCcChunkPerThread][3];
  uint32_t lowest = 0xffffffffu;
#pragma unroll
  for (int k = 0; k < kCcChunkPerThread; ++k) {
    const size_t t = first + (size_t)k * kCcThreads + threadIdx.x;
    const bool in = t < nt;
#pragma unroll
    for (int j = 0; j < 3; ++j) v[k][j] = in ? tri[t * 3 + j] - index_base : 0xffffffffu;
    if (v[k][0] >= nv || v[k][1] >= nv || v[k][2] >= nv) v[k][0] = v[k][1] = v[k][2] = 0xffffffffu;   // past the end, or an index no extract and no keep writes
    lowest = min(lowest, min(v[k][0], min(v[k][1], v[k][2])));
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) lowest = min(lowest, (uint32_t)__shfl_xor((int)lowest, o));
  if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = lowest;
  for (int i = threadIdx.x; i < kCcWindow; i += kCcThreads) s_parent[i] = (uint32_t)i;
  __syncthreads();
  uint32_t base = s_min[0];
#pragma unroll
  for (int w = 1; w < kCcThreads / 64; ++w) base = min(base, s_min[w]);
  if (base == 0xffffffffu) return;                                     // (uniform: the chunk holds no triangle)
#pragma unroll
  for (int k = 0; k < kCcChunkPerThread; ++k) {
    if (v[k][0] == 0xffffffffu) continue;
    const uint32_t a = v[k][0] - base;
#pragma unroll
    for (int j = 1; j < 3; ++j) {
      if (v[k][j] == v[k][0]) continue;
      const uint32_t b = v[k][j] - base;
      if (a < (uint32_t)kCcWindow && b < (uint32_t)kCcWindow) cc_local_hook(s_parent, a, b);
      else cc_hook(parent, v[k][0], v[k][j]);
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < (uint32_t)kCcWindow; i += kCcThreads) {
    uint32_t r = s_parent[i];
    if (r == i) continue;                                              // a local root, or a vertex the chunk does not touch
    for (uint32_t p = s_parent[r]; p != r; p = s_parent[r]) r = p;
    cc_hook(parent, base + i, base + r);                               // (base + i < nv: only an edge's end has a parent)
  }
}
// behind the hooks' launch boundary: plain reads
__device__ __forceinline__ uint32_t cc_root(const uint32_t* __restrict__ parent, uint32_t x) {
  uint32_t p = parent[x];
  while (p != x) { x = p; p = parent[x]; }
  return x;
}

// ---- counting per component.  A workgroup takes consecutive elements, 256 at a time.  Each wave keeps a run {component, count} in (uniform) registers:
// per turn it takes the distinct components among its lanes one by one (at most 64 turns, one when the wave lies inside one component), adds to the run
// where the component is the run's and otherwise flushes the run with ONE atomic add and starts the next.  At the end the four waves' runs meet in LDS
// and equal neighbours are merged: a workgroup inside one component adds once.  (Adds to one address serialise at about 11 ns each on this device: with
// one add per wave the big component's counter alone cost 0.6 ms for 3.3 M triangles.)  counter: component c's word is counter[c * kStride].
struct CcRun { uint32_t component, count; };
template <int kStride>
__device__ __forceinline__ void cc_run_flush(uint32_t* counter, const CcRun& run) {
  if (run.count && (threadIdx.x & 63) == 0) atomicAdd(counter + (size_t)run.component * kStride, run.count);
}
template <int kStride>
__device__ __forceinline__ void cc_run_add(uint32_t* counter, CcRun& run, uint32_t component, bool valid) {   // every lane of the wave calls it
  unsigned long long todo = __ballot(valid);
  while (todo) {
    const uint32_t c = (uint32_t)__shfl((int)component, __ffsll(todo) - 1);
    const unsigned long long same = __ballot(valid && component == c);
    const uint32_t n = (uint32_t)__popcll(same);
    if (c == run.component) run.count += n;
    else { cc_run_flush<kStride>(counter, run); run.component = c; run.count = n; }
    todo &= ~same;
  }
}
template <int kStride>
__device__ __forceinline__ void cc_run_finish(uint32_t* counter, const CcRun& run, CcRun* s_run) {          // every lane of the workgroup calls it
  if ((threadIdx.x & 63) == 0) s_run[threadIdx.x >> 6] = run;
  __syncthreads();
  if (threadIdx.x != 0) return;
  CcRun acc = s_run[0];
  for (int w = 1; w < kCcThreads / 64; ++w) {
    const CcRun r = s_run[w];
    if (r.component == acc.component) acc.count += r.count;
    else { cc_run_flush<kStride>(counter, acc); acc = r; }
  }
  cc_run_flush<kStride>(counter, acc);
}

}  // namespace rr
#endif
