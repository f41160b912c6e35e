// Mesh components (tsdf_mesh_components / _keep_components / _filter_components; include/rgbd_recon_hip.h has the definition): the connected components
// of the mesh an extract left in the context -- connectivity by INDEX through the triangles, never by position --, numbered by their smallest vertex, and
// the mesh without a set of them.  Only the mesh arrays are read: every level of detail and both volume storages look the same from here.
//
// Label.  A union-find over parent[V], parent[v] = v at the start; the edges (v0, v1) and (v0, v2) of every triangle are hooked.  The one invariant is
// parent[x] <= x: every link points to a smaller index, every write is an atomicMin, so every walk is strictly decreasing and ends.  No lane waits for a
// value another lane has yet to write -- no flag, no retry whose exit another lane decides; a hook that loses a race goes on with a strictly smaller pair.
// Why the result is defined although arrival order is not: a lane holds an obligation "a ~ b".  It finds both roots; if they differ it lowers the larger
// root's parent to the smaller one (atomicMin).  Whatever the old value was, {links} + {obligations} connect the same vertices before and after: the link
// hi -> old became hi -> min(old, lo) and the obligation hi ~ lo became old ~ lo (none when old == hi: hi was a root and now hangs under lo).  When
// every lane has returned there are no obligations left, so the forest connects exactly what the triangles connect, and each tree's root is its smallest
// index.  The flatten launch (the launch boundary is the fence) writes label[v] = root(v): the same words on every run.
// A workgroup first merges its chunk of consecutive triangles in LDS (k_cc_hook_local) and sends only what is left to the global forest: at 512^3 / 1.67 M
// vertices / 3.33 M triangles the labelling takes 0.47 ms so, 1.78 ms with one lane per triangle hooking both edges globally (agent-scope loads and
// atomics pass the L2 of the lane's XCD by; the plain form was measured and taken out).
// Number.  is_root[v] = label[v] == v, an exclusive scan (block sums, scan of the sums, apply -- the shape of k_mesh.hip's scan) gives every root its
// component index and the count C; then vertex_component[v] = rank[label[v]], triangle_component[t] = that of its first vertex, table[c].first_vertex.
// Count.  Integer atomic adds into the table, once per run of elements of one component inside a workgroup (one component usually holds almost
// everything: neither 64 lanes nor 50 000 waves must hit one address).  Integer sums do not depend on the order.
// Keep.  Per-vertex and per-triangle keep flags from keep[component], two exclusive scans, scatter: no atomic, the order is the scan's.
#include "tsdf_common.hpp"
#include "scan_dev.hpp"
#include "mesh_cc_dev.hpp"

namespace rr {

constexpr int kCcScanThreads = 256, kCcScanPerThread = 4, kCcScanPerBlock = kCcScanThreads * kCcScanPerThread;

// ---- 1. label (the forest, the hooks and a chunk's local first pass: mesh_cc_dev.hpp)
__global__ __launch_bounds__(kCcThreads) void k_cc_init(uint32_t* __restrict__ parent, uint32_t nv) {
  const size_t v = (size_t)blockIdx.x * kCcThreads + threadIdx.x;
  if (v < nv) parent[v] = (uint32_t)v;
}
__global__ __launch_bounds__(kCcThreads) void k_cc_hook_local(const uint32_t* __restrict__ tri, size_t nt, uint32_t* parent, uint32_t nv) {
  __shared__ uint32_t s_parent[kCcWindow];
  __shared__ uint32_t s_min[kCcThreads / 64];
  cc_hook_chunk(tri, nt, parent, nv, (size_t)blockIdx.x * kCcChunk, s_parent, s_min);
}
// behind the hooks' launch boundary: plain reads
__global__ __launch_bounds__(kCcThreads) void k_cc_flatten(const uint32_t* __restrict__ parent, uint32_t* __restrict__ label, uint32_t nv) {
  const size_t v = (size_t)blockIdx.x * kCcThreads + threadIdx.x;
  if (v >= nv) return;
  label[v] = cc_root(parent, (uint32_t)v);
}

// ---- 2. the scan: per-block sums of a 0 / 1 flag, their exclusive scan (sums[nb] = the total), and an apply that hands every element its flag and the
// number of set flags before it.  A block covers kCcScanPerBlock elements; everything across blocks is 64-bit.
struct CcRootFlag {                                                    // element v is a root
  const uint32_t* label;
  __device__ __forceinline__ uint32_t operator()(size_t v) const { return label[v] == (uint32_t)v ? 1u : 0u; }
};
struct CcKeepFlag {                                                    // element i (a vertex or a triangle) belongs to a component that stays
  const uint8_t* keep; const uint32_t* component;
  __device__ __forceinline__ uint32_t operator()(size_t i) const { return keep[component[i]] ? 1u : 0u; }
};
template <typename Flag>
__device__ __forceinline__ uint32_t cc_scan_load(const Flag& f, size_t n, uint32_t fl[kCcScanPerThread]) {
  const size_t first = ((size_t)blockIdx.x * kCcScanThreads + threadIdx.x) * kCcScanPerThread;
  uint32_t sum = 0;
#pragma unroll
  for (int k = 0; k < kCcScanPerThread; ++k) { fl[k] = first + k < n ? f(first + k) : 0u; sum += fl[k]; }
  return sum;
}
template <typename Flag>
__global__ __launch_bounds__(kCcScanThreads) void k_cc_block_sums(Flag f, size_t n, unsigned long long* __restrict__ sums) {
  __shared__ uint32_t s_wave[kCcScanThreads / 64];
  uint32_t fl[kCcScanPerThread], total;
  block_exclusive_sum<kCcScanThreads / 64>(cc_scan_load(f, n, fl), s_wave, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// one workgroup: sums[0 .. nb) become exclusive prefixes, sums[nb] the total.  Every lane takes a contiguous run of blocks.
__global__ __launch_bounds__(kCcScanThreads) void k_cc_scan_sums(unsigned long long* __restrict__ sums, int nb) {
  __shared__ unsigned long long s_run[kCcScanThreads];
  const int per = (nb + kCcScanThreads - 1) / kCcScanThreads, b0 = min((int)threadIdx.x * per, nb), b1 = min(b0 + per, nb);
  unsigned long long run = 0;
  for (int b = b0; b < b1; ++b) run += sums[b];
  s_run[threadIdx.x] = run;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long acc = 0;
    for (int k = 0; k < kCcScanThreads; ++k) { const unsigned long long s = s_run[k]; s_run[k] = acc; acc += s; }
    sums[nb] = acc;
  }
  __syncthreads();
  unsigned long long acc = s_run[threadIdx.x];
  for (int b = b0; b < b1; ++b) { const unsigned long long s = sums[b]; sums[b] = acc; acc += s; }
}
template <typename Flag, typename Emit>
__global__ __launch_bounds__(kCcScanThreads) void k_cc_scan_apply(Flag f, Emit emit, size_t n, const unsigned long long* __restrict__ sums) {
  __shared__ uint32_t s_wave[kCcScanThreads / 64];
  uint32_t fl[kCcScanPerThread], total;
  const uint32_t mine = cc_scan_load(f, n, fl);
  unsigned long long at = sums[blockIdx.x] + block_exclusive_sum<kCcScanThreads / 64>(mine, s_wave, &total);
  const size_t first = ((size_t)blockIdx.x * kCcScanThreads + threadIdx.x) * kCcScanPerThread;
#pragma unroll
  for (int k = 0; k < kCcScanPerThread; ++k)
    if (first + k < n) { emit(first + k, at, fl[k]); at += fl[k]; }
}

// ---- 2b. number: a root's rank is its component; the table's entry starts {first_vertex, 0, 0, 0}
struct CcRankEmit {
  uint32_t* rank; tsdf_mesh_component* table;
  __device__ __forceinline__ void operator()(size_t v, unsigned long long at, uint32_t is_root) const {
    if (!is_root) return;
    rank[v] = (uint32_t)at;
    *(uint4*)&table[at] = make_uint4((uint32_t)v, 0u, 0u, 0u);
  }
};
// ---- 3. count: integer atomic adds into the table, once per run of elements of one component inside a workgroup (mesh_cc_dev.hpp).
// counter: &table[0].field, components 4 words apart.
constexpr int kCcCountPerThread = 8, kCcCountPerBlock = kCcThreads * kCcCountPerThread;
// vertex_component holds the labels on entry (its own word is all a lane reads of it)
__global__ __launch_bounds__(kCcThreads) void k_cc_vertex_component(const uint32_t* __restrict__ rank, uint32_t* __restrict__ vertex_component, uint32_t nv,
                                                                    tsdf_mesh_component* __restrict__ table) {
  __shared__ CcRun s_run[kCcThreads / 64];
  CcRun run{0u, 0u};
  for (int k = 0; k < kCcCountPerThread; ++k) {
    const size_t v = (size_t)blockIdx.x * kCcCountPerBlock + (size_t)k * kCcThreads + threadIdx.x;
    const bool valid = v < nv;
    uint32_t c = 0;
    if (valid) { c = rank[vertex_component[v]]; vertex_component[v] = c; }
    cc_run_add<4>(&table->n_vertices, run, c, valid);
  }
  cc_run_finish<4>(&table->n_vertices, run, s_run);
}
__global__ __launch_bounds__(kCcThreads) void k_cc_triangle_component(const uint32_t* __restrict__ tri, size_t nt, const uint32_t* __restrict__ vertex_component, uint32_t nv,
                                                                      uint32_t* __restrict__ triangle_component, tsdf_mesh_component* __restrict__ table) {
  __shared__ CcRun s_run[kCcThreads / 64];
  CcRun run{0u, 0u};
  for (int k = 0; k < kCcCountPerThread; ++k) {
    const size_t t = (size_t)blockIdx.x * kCcCountPerBlock + (size_t)k * kCcThreads + threadIdx.x;
    const bool valid = t < nt;
    uint32_t c = 0;
    if (valid) { const uint32_t v0 = tri[t * 3]; c = v0 < nv ? vertex_component[v0] : 0u; triangle_component[t] = c; }
    cc_run_add<4>(&table->n_triangles, run, c, valid);
  }
  cc_run_finish<4>(&table->n_triangles, run, s_run);
}
// the largest n_triangles: a maximum per wave, then one atomicMax
__global__ __launch_bounds__(kCcThreads) void k_cc_largest(const tsdf_mesh_component* __restrict__ table, uint32_t n, uint32_t* __restrict__ largest) {
  const size_t c = (size_t)blockIdx.x * kCcThreads + threadIdx.x;
  uint32_t m = c < n ? table[c].n_triangles : 0u;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
  if ((threadIdx.x & 63) == 0 && m) atomicMax(largest, m);
}

// ---- 4. keep
__global__ __launch_bounds__(kCcThreads) void k_cc_keep_from_table(const tsdf_mesh_component* __restrict__ table, uint32_t n, uint32_t min_triangles, uint8_t* __restrict__ keep) {
  const size_t c = (size_t)blockIdx.x * kCcThreads + threadIdx.x;
  if (c < n) keep[c] = table[c].n_triangles >= min_triangles ? 1 : 0;
}
// a kept vertex: its new index, and its rows bit for bit (words, not floats: NaN payloads travel)
struct CcVertexEmit {
  MeshArrays src, dst; uint32_t* new_index;
  __device__ __forceinline__ void operator()(size_t v, unsigned long long at, uint32_t kept) const {
    if (!kept) return;
    new_index[v] = (uint32_t)at;
    const uint32_t* p = (const uint32_t*)src.pos + v * 3; uint32_t* q = (uint32_t*)dst.pos + at * 3;
    q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
    if (src.nrm) {
      const uint32_t* n = (const uint32_t*)src.nrm + v * 3; uint32_t* m = (uint32_t*)dst.nrm + at * 3;
      m[0] = n[0]; m[1] = n[1]; m[2] = n[2];
    }
    if (src.col) ((uint4*)dst.col)[at] = ((const uint4*)src.col)[v];
  }
};
// a kept triangle: its three indices remapped, the winding untouched (all three vertices are kept: they are of its component)
struct CcTriangleEmit {
  const uint32_t* src; uint32_t* dst; const uint32_t* new_index;
  __device__ __forceinline__ void operator()(size_t t, unsigned long long at, uint32_t kept) const {
    if (!kept) return;
    dst[at * 3 + 0] = new_index[src[t * 3 + 0]]; dst[at * 3 + 1] = new_index[src[t * 3 + 1]]; dst[at * 3 + 2] = new_index[src[t * 3 + 2]];
  }
};

// ---- launchers (a count of 0 launches nothing)
static dim3 cc_grid(size_t n) { return dim3((unsigned)((n + kCcThreads - 1) / kCcThreads)); }
int mesh_cc_scan_blocks(size_t n) { return (int)((n + kCcScanPerBlock - 1) / kCcScanPerBlock); }
template <typename Flag>
static void cc_scan_sums(hipStream_t st, const Flag& f, size_t n, unsigned long long* sums) {
  const int nb = mesh_cc_scan_blocks(n);
  if (nb) hipLaunchKernelGGL(k_cc_block_sums<Flag>, dim3(nb), dim3(kCcScanThreads), 0, st, f, n, sums);
  hipLaunchKernelGGL(k_cc_scan_sums, dim3(1), dim3(kCcScanThreads), 0, st, sums, nb);
}
void launch_mesh_cc_label(hipStream_t st, const uint32_t* tri, uint32_t nv, size_t nt, uint32_t* parent, uint32_t* label, unsigned long long* sums) {
  if (nv) hipLaunchKernelGGL(k_cc_init, cc_grid(nv), dim3(kCcThreads), 0, st, parent, nv);
  if (nv && nt) hipLaunchKernelGGL(k_cc_hook_local, dim3((unsigned)((nt + kCcChunk - 1) / kCcChunk)), dim3(kCcThreads), 0, st, tri, nt, parent, nv);
  if (nv) hipLaunchKernelGGL(k_cc_flatten, cc_grid(nv), dim3(kCcThreads), 0, st, parent, label, nv);
  cc_scan_sums(st, CcRootFlag{label}, nv, sums);
}
void launch_mesh_cc_number(hipStream_t st, const uint32_t* tri, uint32_t nv, size_t nt, const unsigned long long* sums, uint32_t n_components, uint32_t* rank,
                           uint32_t* vertex_component, uint32_t* triangle_component, tsdf_mesh_component* table, uint32_t* largest) {
  if (!nv) return;
  hipLaunchKernelGGL((k_cc_scan_apply<CcRootFlag, CcRankEmit>), dim3(mesh_cc_scan_blocks(nv)), dim3(kCcScanThreads), 0, st, CcRootFlag{vertex_component},
                     CcRankEmit{rank, table}, (size_t)nv, sums);
  const auto count_grid = [](size_t n) { return dim3((unsigned)((n + kCcCountPerBlock - 1) / kCcCountPerBlock)); };
  hipLaunchKernelGGL(k_cc_vertex_component, count_grid(nv), dim3(kCcThreads), 0, st, rank, vertex_component, nv, table);
  if (nt) hipLaunchKernelGGL(k_cc_triangle_component, count_grid(nt), dim3(kCcThreads), 0, st, tri, nt, vertex_component, nv, triangle_component, table);
  hipLaunchKernelGGL(k_cc_largest, cc_grid(n_components), dim3(kCcThreads), 0, st, table, n_components, largest);
}
void launch_mesh_cc_keep_from_table(hipStream_t st, const tsdf_mesh_component* table, uint32_t n_components, uint32_t min_triangles, uint8_t* keep) {
  if (n_components) hipLaunchKernelGGL(k_cc_keep_from_table, cc_grid(n_components), dim3(kCcThreads), 0, st, table, n_components, min_triangles, keep);
}
void launch_mesh_cc_keep_count(hipStream_t st, const uint8_t* keep, const uint32_t* vertex_component, const uint32_t* triangle_component, uint32_t nv, size_t nt,
                               unsigned long long* vertex_sums, unsigned long long* triangle_sums) {
  cc_scan_sums(st, CcKeepFlag{keep, vertex_component}, nv, vertex_sums);
  cc_scan_sums(st, CcKeepFlag{keep, triangle_component}, nt, triangle_sums);
}
void launch_mesh_cc_keep_scatter(hipStream_t st, const uint8_t* keep, const uint32_t* vertex_component, const uint32_t* triangle_component, uint32_t nv, size_t nt,
                                 const unsigned long long* vertex_sums, const unsigned long long* triangle_sums, const MeshArrays& src, const MeshArrays& dst,
                                 uint32_t* new_index) {
  if (nv)
    hipLaunchKernelGGL((k_cc_scan_apply<CcKeepFlag, CcVertexEmit>), dim3(mesh_cc_scan_blocks(nv)), dim3(kCcScanThreads), 0, st, CcKeepFlag{keep, vertex_component},
                       CcVertexEmit{src, dst, new_index}, (size_t)nv, vertex_sums);
  if (nt)
    hipLaunchKernelGGL((k_cc_scan_apply<CcKeepFlag, CcTriangleEmit>), dim3(mesh_cc_scan_blocks(nt)), dim3(kCcScanThreads), 0, st, CcKeepFlag{keep, triangle_component},
                       CcTriangleEmit{src.tri, dst.tri, new_index}, nt, triangle_sums);
}

}  // namespace rr
