// Mesh components on a Z-slab context (tsdf_mesh_slab_components / _link_components; include/rgbd_recon_hip.h has the definition): the labels of a
// slab's linked part such that the parts' arrays, concatenated in slab order, are the whole mesh's tsdf_mesh_components byte for byte.
//
// Index space.  A part's triangles hold GLOBAL indices: own vertices [base, base + nv) and, in the top cell layer, vertices of the slab above
// [base + nv, base + n): n - nv is the span the link's host check knows.  Everything here works on LOCAL indices i = global - base in [0, n).
// Label (step 1).  mesh_cc_dev.hpp's union-find over parent[n], the triangles read through its index base.  A triangle has an own vertex and own indices
// are the smaller ones, so a tree with a triangle has an own root; an index of the span that is its own root is a vertex no triangle of the part uses.
// The roots among [0, nv) are the local components: a scan ranks them, a local table row per rank takes the counts (cc_run_*: own vertices, triangles).
// Seam lists.  Three flag + scan compactions, each in ascending index order, so that arrival order decides nothing:
//   up     over [nv, n):  label[i] != i                       -> {base + i, base + label[i]}
//   down   over [0, nv):  the plane-0 vertices of the first owned lattice tile layer (k_sc_mark_down: the first records[tile][64] >> 8 vertices of a
//                         tile, plane 0 comes first in a tile's order)  -> {base + v, base + label[v]}
//   roots  over [0, nv):  the roots the two lists name (a byte per vertex, every writer stores 1)  -> {base + r, rank, own vertices, triangles}
// Link (step 3).  The merged links (mesh_cc_seams.hpp; checked on the host against the exported roots: no index of theirs is used that the slab did not
// make) are scattered to their roots; a local root is an own final representative unless its link names a smaller final root; a scan numbers them from
// component_base on and writes their table rows -- the link's totals for a boundary component, the local row otherwise --; a vertex takes its root's
// number, a triangle that of its first vertex.  One lane per element; a link record is read as 16-byte words.
// The scans are this file's own (block sums, scan of the sums, apply: the shape of k_mesh_components.hip's, on scan_dev.hpp).
#include "tsdf_common.hpp"
#include "scan_dev.hpp"
#include "mesh_cc_dev.hpp"

namespace rr {

constexpr int kScThreads = 256, kScPerThread = 4, kScPerBlock = kScThreads * kScPerThread;
constexpr uint32_t kScNoLink = 0xffffffffu;

// ---- step 1: label
__global__ __launch_bounds__(kCcThreads) void k_sc_init(uint32_t* __restrict__ parent, uint32_t n) {
  const size_t i = (size_t)blockIdx.x * kCcThreads + threadIdx.x;
  if (i < n) parent[i] = (uint32_t)i;
}
__global__ __launch_bounds__(kCcThreads) void k_sc_hook(const uint32_t* __restrict__ tri, size_t nt, uint32_t* parent, uint32_t n, uint32_t base) {
  __shared__ uint32_t s_parent[kCcWindow];
  __shared__ uint32_t s_min[kCcThreads / 64];
  cc_hook_chunk(tri, nt, parent, n, (size_t)blockIdx.x * kCcChunk, s_parent, s_min, base);
}
__global__ __launch_bounds__(kCcThreads) void k_sc_flatten(const uint32_t* __restrict__ parent, uint32_t* __restrict__ label, uint32_t n) {
  const size_t i = (size_t)blockIdx.x * kCcThreads + threadIdx.x;
  if (i < n) label[i] = cc_root(parent, (uint32_t)i);
}
// the plane-0 vertices of the first owned layer's tiles: workgroup b is tile b; mark: nv bytes, zero on entry
__global__ __launch_bounds__(kCcThreads) void k_sc_mark_down(const uint2* __restrict__ tile_cnt, const uint32_t* __restrict__ tile_vbase, const uint32_t* __restrict__ tile_rec,
                                                             const uint32_t* __restrict__ records, uint32_t nv, uint8_t* __restrict__ mark) {
  const uint32_t tile = blockIdx.x, slot = tile_rec[tile];
  if (slot == kNoSlot) return;
  const uint32_t n0 = min(records[(size_t)slot * 512 + 64] >> 8, tile_cnt[tile].x), first = tile_vbase[tile];   // (lane 64's offset: what plane 0 owns)
  for (uint32_t k = threadIdx.x; k < n0; k += kCcThreads)
    if (first + k < nv) mark[first + k] = 1;
}

// ---- the scans: per-block sums of a 0 / 1 flag over elements [first, first + n), their exclusive scan (sums[nb] = the total), and an apply that hands
// every element its flag and the number of set flags before it
struct ScRootFlag {                                                    // own vertex v is a local root
  const uint32_t* label;
  __device__ __forceinline__ uint32_t operator()(size_t v) const { return label[v] == (uint32_t)v ? 1u : 0u; }
};
struct ScUpFlag {                                                      // index i of the span is used by a triangle of the part
  const uint32_t* label;
  __device__ __forceinline__ uint32_t operator()(size_t i) const { return label[i] != (uint32_t)i ? 1u : 0u; }
};
struct ScByteFlag {
  const uint8_t* flag;
  __device__ __forceinline__ uint32_t operator()(size_t v) const { return flag[v] ? 1u : 0u; }
};
// the link of root v, its first 16 bytes {root, final_root, component, 0}; .x == kScNoLink: none
__device__ __forceinline__ uint4 sc_link_head(const uint32_t* __restrict__ link_of, const tsdf_mesh_component_link* __restrict__ links, size_t v) {
  const uint32_t l = link_of[v];
  return l == kScNoLink ? make_uint4(kScNoLink, 0u, 0u, 0u) : *(const uint4*)&links[l];
}
struct ScOwnedFlag {                                                   // own vertex v is the representative of a component of the WHOLE mesh
  const uint32_t* label; const uint32_t* link_of; const tsdf_mesh_component_link* links;
  __device__ __forceinline__ uint32_t operator()(size_t v) const {
    if (label[v] != (uint32_t)v) return 0u;
    const uint4 h = sc_link_head(link_of, links, v);
    return h.x == kScNoLink || h.y == h.x ? 1u : 0u;
  }
};
template <typename Flag>
__device__ __forceinline__ uint32_t sc_scan_load(const Flag& f, size_t first, size_t n, uint32_t fl[kScPerThread]) {
  const size_t at = ((size_t)blockIdx.x * kScThreads + threadIdx.x) * kScPerThread;
  uint32_t sum = 0;
#pragma unroll
  for (int k = 0; k < kScPerThread; ++k) { fl[k] = at + k < n ? f(first + at + k) : 0u; sum += fl[k]; }
  return sum;
}
template <typename Flag>
__global__ __launch_bounds__(kScThreads) void k_sc_block_sums(Flag f, size_t first, size_t n, unsigned long long* __restrict__ sums) {
  __shared__ uint32_t s_wave[kScThreads / 64];
  uint32_t fl[kScPerThread], total;
  block_exclusive_sum<kScThreads / 64>(sc_scan_load(f, first, n, fl), s_wave, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
// one workgroup: sums[0 .. nb) become exclusive prefixes, sums[nb] the total.  Every lane takes a contiguous run of blocks.
__global__ __launch_bounds__(kScThreads) void k_sc_scan_sums(unsigned long long* __restrict__ sums, int nb) {
  __shared__ unsigned long long s_run[kScThreads];
  const int per = (nb + kScThreads - 1) / kScThreads, b0 = min((int)threadIdx.x * per, nb), b1 = min(b0 + per, nb);
  unsigned long long run = 0;
  for (int b = b0; b < b1; ++b) run += sums[b];
  s_run[threadIdx.x] = run;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long acc = 0;
    for (int k = 0; k < kScThreads; ++k) { const unsigned long long s = s_run[k]; s_run[k] = acc; acc += s; }
    sums[nb] = acc;
  }
  __syncthreads();
  unsigned long long acc = s_run[threadIdx.x];
  for (int b = b0; b < b1; ++b) { const unsigned long long s = sums[b]; sums[b] = acc; acc += s; }
}
template <typename Flag, typename Emit>
__global__ __launch_bounds__(kScThreads) void k_sc_scan_apply(Flag f, Emit emit, size_t first, size_t n, const unsigned long long* __restrict__ sums) {
  __shared__ uint32_t s_wave[kScThreads / 64];
  uint32_t fl[kScPerThread], total;
  const uint32_t mine = sc_scan_load(f, first, n, fl);
  unsigned long long at = sums[blockIdx.x] + block_exclusive_sum<kScThreads / 64>(mine, s_wave, &total);
  const size_t e = ((size_t)blockIdx.x * kScThreads + threadIdx.x) * kScPerThread;
#pragma unroll
  for (int k = 0; k < kScPerThread; ++k)
    if (e + k < n) { if (fl[k]) emit(first + e + k, at); at += fl[k]; }
}

// ---- what the scans emit
struct ScRankEmit {                                                    // a local root: its rank, and its local table row {global root, 0, 0, 0}
  uint32_t* rank; tsdf_mesh_component* local; uint32_t base;
  __device__ __forceinline__ void operator()(size_t v, unsigned long long at) const {
    rank[v] = (uint32_t)at;
    *(uint4*)&local[at] = make_uint4(base + (uint32_t)v, 0u, 0u, 0u);
  }
};
struct ScSeamEmit {                                                    // an up or a down record, and its root's byte (label[i] is an own vertex: see the head)
  const uint32_t* label; tsdf_mesh_seam_vertex* out; uint8_t* seam_root; uint32_t base, nv;
  __device__ __forceinline__ void operator()(size_t i, unsigned long long at) const {
    const uint32_t r = label[i];
    *(uint2*)&out[at] = make_uint2(base + (uint32_t)i, base + r);
    if (r < nv) seam_root[r] = 1;                                      // (always, on an extract's triangles; a root that is no own vertex gets no record and the merge refuses the list)
  }
};
struct ScRootEmit {                                                    // a root record: the local row's counts under the root's rank
  const uint32_t* rank; const tsdf_mesh_component* local; tsdf_mesh_seam_root* out; uint32_t base;
  __device__ __forceinline__ void operator()(size_t v, unsigned long long at) const {
    const uint32_t k = rank[v];
    const uint4 row = *(const uint4*)&local[k];
    *(uint4*)&out[at] = make_uint4(base + (uint32_t)v, k, row.y, row.z);
  }
};
struct ScOwnedEmit {                                                   // an own final representative: its number (an unlinked root's: the link's stands already), its row
  const uint32_t* rank; const tsdf_mesh_component* local; const uint32_t* link_of; const tsdf_mesh_component_link* links;
  uint32_t* number; tsdf_mesh_component* table; uint32_t base, component_base;
  __device__ __forceinline__ void operator()(size_t v, unsigned long long at) const {
    const uint32_t l = link_of[v];
    if (l == kScNoLink) {
      number[v] = component_base + (uint32_t)at;
      *(uint4*)&table[at] = *(const uint4*)&local[rank[v]];
    } else {
      const uint4 totals = ((const uint4*)&links[l])[1];                 // {n_vertices, n_triangles, 0, 0} of the whole component
      *(uint4*)&table[at] = make_uint4(base + (uint32_t)v, totals.x, totals.y, 0u);
    }
  }
};

// ---- the local counts: integer adds into the local rows, once per run of elements of one component inside a workgroup (mesh_cc_dev.hpp)
constexpr int kScCountPerThread = 8, kScCountPerBlock = kCcThreads * kScCountPerThread;
__global__ __launch_bounds__(kCcThreads) void k_sc_count_vertices(const uint32_t* __restrict__ label, const uint32_t* __restrict__ rank, uint32_t nv,
                                                                  tsdf_mesh_component* __restrict__ local) {
  __shared__ CcRun s_run[kCcThreads / 64];
  CcRun run{0u, 0u};
  for (int k = 0; k < kScCountPerThread; ++k) {
    const size_t v = (size_t)blockIdx.x * kScCountPerBlock + (size_t)k * kCcThreads + threadIdx.x;
    const bool valid = v < nv;
    const uint32_t c = valid ? rank[label[v]] : 0u;
    cc_run_add<4>(&local->n_vertices, run, c, valid);
  }
  cc_run_finish<4>(&local->n_vertices, run, s_run);
}
// the own root above a triangle's first vertex, or kScNoLink for a triangle whose first index the forest does not hold (no link writes one)
__device__ __forceinline__ uint32_t sc_triangle_root(const uint32_t* __restrict__ tri, size_t t, const uint32_t* __restrict__ label, uint32_t nv, uint32_t n, uint32_t base) {
  const uint32_t i = tri[t * 3] - base;
  if (i >= n) return kScNoLink;
  const uint32_t r = label[i];
  return r < nv ? r : kScNoLink;
}
__global__ __launch_bounds__(kCcThreads) void k_sc_count_triangles(const uint32_t* __restrict__ tri, size_t nt, const uint32_t* __restrict__ label,
                                                                   const uint32_t* __restrict__ rank, uint32_t nv, uint32_t n, uint32_t base,
                                                                   tsdf_mesh_component* __restrict__ local) {
  __shared__ CcRun s_run[kCcThreads / 64];
  CcRun run{0u, 0u};
  for (int k = 0; k < kScCountPerThread; ++k) {
    const size_t t = (size_t)blockIdx.x * kScCountPerBlock + (size_t)k * kCcThreads + threadIdx.x;
    const uint32_t r = t < nt ? sc_triangle_root(tri, t, label, nv, n, base) : kScNoLink;
    const bool valid = r != kScNoLink;
    cc_run_add<4>(&local->n_triangles, run, valid ? rank[r] : 0u, valid);
  }
  cc_run_finish<4>(&local->n_triangles, run, s_run);
}

// ---- step 3: the links to their roots (link_of: nv words of kScNoLink on entry; the host has checked that every root is an exported one), the
// components of the vertices and of the triangles
__global__ __launch_bounds__(kCcThreads) void k_sc_scatter_links(const tsdf_mesh_component_link* __restrict__ links, uint32_t n_links, uint32_t base, uint32_t nv,
                                                                 uint32_t* __restrict__ link_of, uint32_t* __restrict__ number) {
  const uint32_t i = blockIdx.x * kCcThreads + threadIdx.x;
  if (i >= n_links) return;
  const uint4 h = *(const uint4*)&links[i];
  const uint32_t v = h.x - base;
  if (v < nv) { link_of[v] = i; number[v] = h.z; }
}
__global__ __launch_bounds__(kCcThreads) void k_sc_vertex_component(const uint32_t* __restrict__ label, const uint32_t* __restrict__ number, uint32_t nv,
                                                                    uint32_t* __restrict__ vertex_component) {
  const size_t v = (size_t)blockIdx.x * kCcThreads + threadIdx.x;
  if (v < nv) vertex_component[v] = number[label[v]];
}
__global__ __launch_bounds__(kCcThreads) void k_sc_triangle_component(const uint32_t* __restrict__ tri, size_t nt, const uint32_t* __restrict__ label,
                                                                      const uint32_t* __restrict__ number, uint32_t nv, uint32_t n, uint32_t base,
                                                                      uint32_t* __restrict__ triangle_component) {
  const size_t t = (size_t)blockIdx.x * kCcThreads + threadIdx.x;
  if (t >= nt) return;
  const uint32_t r = sc_triangle_root(tri, t, label, nv, n, base);
  triangle_component[t] = r != kScNoLink ? number[r] : 0u;
}

// ---- launchers (a count of 0 launches nothing)
static dim3 sc_grid(size_t n) { return dim3((unsigned)((n + kCcThreads - 1) / kCcThreads)); }
static dim3 sc_count_grid(size_t n) { return dim3((unsigned)((n + kScCountPerBlock - 1) / kScCountPerBlock)); }
int mesh_sc_scan_blocks(size_t n) { return (int)((n + kScPerBlock - 1) / kScPerBlock); }
template <typename Flag>
static void sc_scan_sums(hipStream_t st, const Flag& f, size_t first, size_t n, unsigned long long* sums) {
  const int nb = mesh_sc_scan_blocks(n);
  if (nb) hipLaunchKernelGGL(k_sc_block_sums<Flag>, dim3(nb), dim3(kScThreads), 0, st, f, first, n, sums);
  hipLaunchKernelGGL(k_sc_scan_sums, dim3(1), dim3(kScThreads), 0, st, sums, nb);
}
template <typename Flag, typename Emit>
static void sc_scan_apply(hipStream_t st, const Flag& f, const Emit& e, size_t first, size_t n, const unsigned long long* sums) {
  if (n) hipLaunchKernelGGL((k_sc_scan_apply<Flag, Emit>), dim3(mesh_sc_scan_blocks(n)), dim3(kScThreads), 0, st, f, e, first, n, sums);
}
void launch_mesh_sc_label(hipStream_t st, const MeshSlabLabelling& W, const MeshScratch& S, const uint32_t* records, int first_layer_tiles) {
  const uint32_t nv = W.nv, n = W.n;
  hipLaunchKernelGGL(k_sc_init, sc_grid(n), dim3(kCcThreads), 0, st, W.parent, n);
  if (W.nt) hipLaunchKernelGGL(k_sc_hook, dim3((unsigned)((W.nt + kCcChunk - 1) / kCcChunk)), dim3(kCcThreads), 0, st, W.tri, W.nt, W.parent, n, W.base);
  hipLaunchKernelGGL(k_sc_flatten, sc_grid(n), dim3(kCcThreads), 0, st, W.parent, W.label, n);
  if (first_layer_tiles) hipLaunchKernelGGL(k_sc_mark_down, dim3(first_layer_tiles), dim3(kCcThreads), 0, st, S.tile_cnt, S.tile_vbase, S.tile_rec, records, nv, W.down_mark);
  sc_scan_sums(st, ScRootFlag{W.label}, 0, nv, W.root_sums);
  sc_scan_sums(st, ScUpFlag{W.label}, nv, n - nv, W.up_sums);
  sc_scan_sums(st, ScByteFlag{W.down_mark}, 0, nv, W.down_sums);
}
void launch_mesh_sc_lists(hipStream_t st, const MeshSlabLabelling& W, tsdf_mesh_component* local, tsdf_mesh_seam_vertex* down, tsdf_mesh_seam_vertex* up,
                          tsdf_mesh_seam_root* roots) {
  const uint32_t nv = W.nv, n = W.n;
  sc_scan_apply(st, ScRootFlag{W.label}, ScRankEmit{W.rank, local, W.base}, 0, nv, W.root_sums);
  hipLaunchKernelGGL(k_sc_count_vertices, sc_count_grid(nv), dim3(kCcThreads), 0, st, W.label, W.rank, nv, local);
  if (W.nt) hipLaunchKernelGGL(k_sc_count_triangles, sc_count_grid(W.nt), dim3(kCcThreads), 0, st, W.tri, W.nt, W.label, W.rank, nv, n, W.base, local);
  sc_scan_apply(st, ScUpFlag{W.label}, ScSeamEmit{W.label, up, W.seam_root, W.base, nv}, nv, n - nv, W.up_sums);
  sc_scan_apply(st, ScByteFlag{W.down_mark}, ScSeamEmit{W.label, down, W.seam_root, W.base, nv}, 0, nv, W.down_sums);
  sc_scan_sums(st, ScByteFlag{W.seam_root}, 0, nv, W.seam_sums);
  sc_scan_apply(st, ScByteFlag{W.seam_root}, ScRootEmit{W.rank, local, roots, W.base}, 0, nv, W.seam_sums);
}
void launch_mesh_sc_link(hipStream_t st, const MeshSlabLabelling& W, const tsdf_mesh_component* local, const tsdf_mesh_component_link* links, uint32_t n_links,
                         uint32_t component_base, uint32_t* link_of, uint32_t* number, unsigned long long* sums, uint32_t* vertex_component,
                         uint32_t* triangle_component, tsdf_mesh_component* table) {
  const uint32_t nv = W.nv;
  if (n_links) hipLaunchKernelGGL(k_sc_scatter_links, sc_grid(n_links), dim3(kCcThreads), 0, st, links, n_links, W.base, nv, link_of, number);
  const ScOwnedFlag owned{W.label, link_of, links};
  sc_scan_sums(st, owned, 0, nv, sums);
  sc_scan_apply(st, owned, ScOwnedEmit{W.rank, local, link_of, links, number, table, W.base, component_base}, 0, nv, sums);
  hipLaunchKernelGGL(k_sc_vertex_component, sc_grid(nv), dim3(kCcThreads), 0, st, W.label, number, nv, vertex_component);
  if (W.nt) hipLaunchKernelGGL(k_sc_triangle_component, sc_grid(W.nt), dim3(kCcThreads), 0, st, W.tri, W.nt, W.label, number, nv, W.n, W.base, triangle_component);
}

}  // namespace rr
