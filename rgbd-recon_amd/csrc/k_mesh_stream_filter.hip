// The streamed mesh's filter (tsdf_mesh_stream_config_filter, min_triangles >= 1; include/rgbd_recon_hip.h has the definition): between a frame's emit
// and its header, the components with fewer than min_triangles triangles leave the frame, on the device, without the host knowing a single count.
//
// The emit has left the UNFILTERED frame in the configuration's raw buffer: a MeshStreamHeader, V packed vertices, T triangles.  Every kernel here reads
// V and T from that header (both are 0 when the frame overflowed: nothing was emitted then) and is launched over the configured CAPACITIES; a workgroup
// whose first element lies past the count returns at once, so no launch is sized by a number the host does not have.  Each kernel is written as a loop
// over its workgroup-sized pieces with the grid as the step: the same text serves a grid capped at kSfGridCap workgroups (DESIGN.md has both measured).
//
//   1. k_sf_init      parent[v] = v, count[v] = 0, the two component counters = 0
//   2. k_sf_hook      k_mesh_components.hip's union-find, unchanged (mesh_cc_dev.hpp): LDS window per chunk of consecutive triangles, atomicMin links to
//                     smaller indices only, no lane waits for another
//   3. k_sf_flatten   behind the launch boundary: label[v] = root(v), the smallest index of v's component
//   4. k_sf_count     count[label] += triangles, one integer add per run of one component inside a workgroup (no table, no numbering: the filter needs
//                     a triangle count per ROOT only, so there is no component capacity either)
//   5. k_sf_keep      keep[v] = count[label[v]] >= min_triangles, the kept vertices' block sums, and the two sums of root flags {components, kept}
//   6. k_sf_triangle_sums   a triangle stays iff its first vertex does (all three agree): block sums
//   7. k_sf_scan_sums both arrays of block sums, one workgroup each
//   8. k_sf_scatter_vertices / _triangles   packed rows move as ONE 8- or 16-byte load and store, triangles are remapped; the order is the scan's, no atomic
//   9. k_sf_header    one lane: the slot's final header (the raw one with the filtered counts) and the four filter words
// Integer sums and atomicMin over a forest whose roots are defined: two runs give identical bytes.
//
// The tile-local triangle format (F.raw_table != nullptr; the header's "mesh streaming: compact triangles").  The raw frame is the same uint32 frame, with
// its tile table beside it.  6 also leaves, per four triangles, the kept triangles before them in their block (tri_local); 8's vertex scatter leaves the
// scan's value for EVERY vertex, kept or not, so "kept vertices before old index i" is new_index[i]; then
//   8a. k_sf_table    one workgroup over the raw rows: a row stays iff it keeps a vertex; its first_vertex is new_index[old first_vertex], its triangle
//                     range the triangle scan's values at the old range's ends; the rows that stay are numbered by a running block scan and written
//                     behind the kept vertices (padded to 16); words[2] = their number
//   8b. k_sf_scatter_triangles_compact   a kept triangle's row by bisection in the raw first_triangle column, each corner's owner row by bisection in
//                     the first_vertex column from that row on; code = new offset inside the owner's row | the owner tile's place from the cell's << 12
#include "tsdf_common.hpp"
#include "scan_dev.hpp"
#include "mesh_cc_dev.hpp"

#ifndef RR_SF_GRID_CAP
#define RR_SF_GRID_CAP 0                                               // 0: one workgroup per piece of the capacity
#endif

namespace rr {

constexpr int kSfScanPerThread = 4, kSfScanPerBlock = kCcThreads * kSfScanPerThread;
constexpr int kSfCountPerThread = 8, kSfCountPerBlock = kCcThreads * kSfCountPerThread;
constexpr uint32_t kSfGridCap = RR_SF_GRID_CAP;

__device__ __forceinline__ uint32_t sf_scan_blocks(uint32_t n) { return (n + (uint32_t)kSfScanPerBlock - 1u) / (uint32_t)kSfScanPerBlock; }   // (n <= a capacity, and a slot holds at most 4 GiB: no wrap)
__device__ __forceinline__ const uint32_t* sf_raw_triangles(const MeshStreamHeader* __restrict__ raw, uint32_t nv, uint32_t stride) {
  return (const uint32_t*)((const uint8_t*)(raw + 1) + (size_t)nv * stride);
}

__global__ __launch_bounds__(kCcThreads) void k_sf_init(const MeshStreamHeader* __restrict__ raw, uint32_t* __restrict__ parent, uint32_t* __restrict__ count,
                                                        uint32_t* __restrict__ words) {
  if (blockIdx.x == 0 && threadIdx.x < 2) words[threadIdx.x] = 0u;
  const uint32_t nv = (uint32_t)raw->n_vertices;
  for (size_t v = (size_t)blockIdx.x * kCcThreads + threadIdx.x; v < nv; v += (size_t)gridDim.x * kCcThreads) { parent[v] = (uint32_t)v; count[v] = 0u; }
}
__global__ __launch_bounds__(kCcThreads) void k_sf_hook(const MeshStreamHeader* __restrict__ raw, uint32_t stride, uint32_t* parent) {
  __shared__ uint32_t s_parent[kCcWindow];
  __shared__ uint32_t s_min[kCcThreads / 64];
  const uint32_t nv = (uint32_t)raw->n_vertices;
  const size_t nt = (size_t)raw->n_triangles;
  const uint32_t* __restrict__ tri = sf_raw_triangles(raw, nv, stride);
  for (size_t first = (size_t)blockIdx.x * kCcChunk; first < nt; first += (size_t)gridDim.x * kCcChunk) {   // (uniform: the barriers inside are met by all)
    cc_hook_chunk(tri, nt, parent, nv, first, s_parent, s_min);
    __syncthreads();
  }
}
__global__ __launch_bounds__(kCcThreads) void k_sf_flatten(const MeshStreamHeader* __restrict__ raw, const uint32_t* __restrict__ parent, uint32_t* __restrict__ label) {
  const uint32_t nv = (uint32_t)raw->n_vertices;
  for (size_t v = (size_t)blockIdx.x * kCcThreads + threadIdx.x; v < nv; v += (size_t)gridDim.x * kCcThreads) label[v] = cc_root(parent, (uint32_t)v);
}
__global__ __launch_bounds__(kCcThreads) void k_sf_count(const MeshStreamHeader* __restrict__ raw, uint32_t stride, const uint32_t* __restrict__ label,
                                                         uint32_t* __restrict__ count) {
  __shared__ CcRun s_run[kCcThreads / 64];
  const uint32_t nv = (uint32_t)raw->n_vertices;
  const size_t nt = (size_t)raw->n_triangles;
  const uint32_t* __restrict__ tri = sf_raw_triangles(raw, nv, stride);
  CcRun run{0u, 0u};
  for (size_t first = (size_t)blockIdx.x * kSfCountPerBlock; first < nt; first += (size_t)gridDim.x * kSfCountPerBlock)
    for (int k = 0; k < kSfCountPerThread; ++k) {
      const size_t t = first + (size_t)k * kCcThreads + threadIdx.x;
      const bool valid = t < nt;
      uint32_t c = 0;
      if (valid) { const uint32_t v0 = tri[t * 3]; c = v0 < nv ? label[v0] : 0u; }
      cc_run_add<1>(count, run, c, valid);
    }
  cc_run_finish<1>(count, run, s_run);                                  // (a workgroup without a triangle holds an empty run: it adds nothing)
}
// four consecutive vertices per lane, the scan's layout: the kept vertices' block sums come from the same pass.  keep[] is read and written four bytes at
// a time (its allocation is rounded up to 4).
__global__ __launch_bounds__(kCcThreads) void k_sf_keep(const MeshStreamHeader* __restrict__ raw, const uint32_t* __restrict__ label, const uint32_t* __restrict__ count,
                                                        uint32_t min_triangles, uint8_t* __restrict__ keep, unsigned long long* __restrict__ vertex_sums,
                                                        uint32_t* __restrict__ words) {
  __shared__ uint32_t s_wave[kCcThreads / 64];
  const uint32_t nv = (uint32_t)raw->n_vertices, nb = sf_scan_blocks(nv);
  uint32_t roots = 0, kept_roots = 0;
  for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const size_t first = ((size_t)b * kCcThreads + threadIdx.x) * kSfScanPerThread;
    uint32_t sum = 0, flags = 0;
#pragma unroll
    for (int k = 0; k < kSfScanPerThread; ++k) {
      if (first + k >= nv) continue;
      const uint32_t l = label[first + k], kept = count[l] >= min_triangles ? 1u : 0u;
      flags |= kept << (8 * k); sum += kept;
      if (l == (uint32_t)(first + k)) { ++roots; kept_roots += kept; }
    }
    if (first < nv) *(uint32_t*)(keep + first) = flags;
    uint32_t total;
    block_exclusive_sum<kCcThreads / 64>(sum, s_wave, &total);
    if (threadIdx.x == 0) vertex_sums[b] = total;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { roots += (uint32_t)__shfl_xor((int)roots, o); kept_roots += (uint32_t)__shfl_xor((int)kept_roots, o); }
  if ((threadIdx.x & 63) == 0) {                                        // (roots are few: most waves add nothing)
    if (roots) atomicAdd(words + 0, roots);
    if (kept_roots) atomicAdd(words + 1, kept_roots);
  }
}
__device__ __forceinline__ uint32_t sf_keep_word(const uint8_t* __restrict__ keep, size_t first, uint32_t n) {   // the four flags from `first` on, 0 past n
  if (first >= n) return 0u;
  const uint32_t w = *(const uint32_t*)(keep + first);
  const size_t left = n - first;
  return left >= 4 ? w : (w & ((1u << (8 * (uint32_t)left)) - 1u));
}
template <bool kLocal>
__global__ __launch_bounds__(kCcThreads) void k_sf_triangle_sums(const MeshStreamHeader* __restrict__ raw, uint32_t stride, const uint8_t* __restrict__ keep,
                                                                 unsigned long long* __restrict__ triangle_sums, uint16_t* __restrict__ tri_local) {
  __shared__ uint32_t s_wave[kCcThreads / 64];
  const uint32_t nv = (uint32_t)raw->n_vertices, nt = (uint32_t)raw->n_triangles, nb = sf_scan_blocks(nt);
  const uint32_t* __restrict__ tri = sf_raw_triangles(raw, nv, stride);
  for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const size_t first = ((size_t)b * kCcThreads + threadIdx.x) * kSfScanPerThread;
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < kSfScanPerThread; ++k)
      if (first + k < nt) { const uint32_t v0 = tri[(first + k) * 3]; sum += v0 < nv ? (uint32_t)keep[v0] : 0u; }
    uint32_t total;
    const uint32_t before = block_exclusive_sum<kCcThreads / 64>(sum, s_wave, &total);
    if (kLocal && first < nt) tri_local[first / kSfScanPerThread] = (uint16_t)before;   // (< kSfScanPerBlock; first / 4 < (max_triangles + 3) / 4)
    if (threadIdx.x == 0) triangle_sums[b] = total;
  }
}
// workgroup 0: the vertices' block sums, workgroup 1: the triangles'.  sums[0 .. nb) become exclusive prefixes, sums[nb] the total (k_cc_scan_sums' text).
__global__ __launch_bounds__(kCcThreads) void k_sf_scan_sums(const MeshStreamHeader* __restrict__ raw, unsigned long long* __restrict__ vertex_sums,
                                                             unsigned long long* __restrict__ triangle_sums) {
  __shared__ unsigned long long s_run[kCcThreads];
  unsigned long long* __restrict__ sums = blockIdx.x == 0 ? vertex_sums : triangle_sums;
  const uint32_t nb = sf_scan_blocks((uint32_t)(blockIdx.x == 0 ? raw->n_vertices : raw->n_triangles));
  const uint32_t per = (nb + kCcThreads - 1) / kCcThreads, b0 = min(threadIdx.x * per, nb), b1 = min(b0 + per, nb);
  unsigned long long run = 0;
  for (uint32_t b = b0; b < b1; ++b) run += sums[b];
  s_run[threadIdx.x] = run;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long acc = 0;
    for (int k = 0; k < kCcThreads; ++k) { const unsigned long long s = s_run[k]; s_run[k] = acc; acc += s; }
    sums[nb] = acc;
  }
  __syncthreads();
  unsigned long long acc = s_run[threadIdx.x];
  for (uint32_t b = b0; b < b1; ++b) { const unsigned long long s = sums[b]; sums[b] = acc; acc += s; }
}
// Row: uint2 (8-byte vertices) or uint4 (16).  new_index may be the forest's array: nothing reads a parent behind the flatten.  kAll: new_index is
// written for the dropped vertices too (the kept vertices before them).
template <typename Row, bool kAll>
__global__ __launch_bounds__(kCcThreads) void k_sf_scatter_vertices(const MeshStreamHeader* __restrict__ raw, const uint8_t* __restrict__ keep,
                                                                    const unsigned long long* __restrict__ vertex_sums, uint32_t* __restrict__ new_index,
                                                                    Row* __restrict__ dst) {
  __shared__ uint32_t s_wave[kCcThreads / 64];
  const uint32_t nv = (uint32_t)raw->n_vertices, nb = sf_scan_blocks(nv);
  const Row* __restrict__ src = (const Row*)(raw + 1);
  for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const size_t first = ((size_t)b * kCcThreads + threadIdx.x) * kSfScanPerThread;
    const uint32_t flags = sf_keep_word(keep, first, nv);
    uint32_t total;
    uint32_t at = (uint32_t)vertex_sums[b] + block_exclusive_sum<kCcThreads / 64>((uint32_t)__popc(flags), s_wave, &total);   // (kept <= nv < 2^32)
#pragma unroll
    for (int k = 0; k < kSfScanPerThread; ++k)
      if (flags & (1u << (8 * k))) { new_index[first + k] = at; dst[at] = src[first + k]; ++at; }
      else if (kAll && first + k < nv) new_index[first + k] = at;
  }
}
// the filtered triangles follow the filtered vertices directly: payload + kept vertices * stride
__global__ __launch_bounds__(kCcThreads) void k_sf_scatter_triangles(const MeshStreamHeader* __restrict__ raw, uint32_t stride, const uint8_t* __restrict__ keep,
                                                                     const unsigned long long* __restrict__ vertex_sums, const unsigned long long* __restrict__ triangle_sums,
                                                                     const uint32_t* __restrict__ new_index, uint8_t* __restrict__ payload) {
  __shared__ uint32_t s_wave[kCcThreads / 64];
  const uint32_t nv = (uint32_t)raw->n_vertices, nt = (uint32_t)raw->n_triangles, nb = sf_scan_blocks(nt);
  if (blockIdx.x >= nb) return;
  const uint32_t* __restrict__ tri = sf_raw_triangles(raw, nv, stride);
  uint32_t* __restrict__ dst = (uint32_t*)(payload + (size_t)vertex_sums[sf_scan_blocks(nv)] * stride);
  for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const size_t first = ((size_t)b * kCcThreads + threadIdx.x) * kSfScanPerThread;
    uint32_t v0[kSfScanPerThread], flags = 0;
#pragma unroll
    for (int k = 0; k < kSfScanPerThread; ++k) {
      v0[k] = first + k < nt ? tri[(first + k) * 3] : 0xffffffffu;
      if (v0[k] < nv && keep[v0[k]]) flags |= 1u << k;
    }
    uint32_t total;
    size_t at = (size_t)triangle_sums[b] + block_exclusive_sum<kCcThreads / 64>((uint32_t)__popc(flags), s_wave, &total);
#pragma unroll
    for (int k = 0; k < kSfScanPerThread; ++k)
      if (flags & (1u << k)) {                                           // (all three vertices are kept: they are of the first one's component)
        const uint32_t* __restrict__ s = tri + (first + k) * 3;
        dst[at * 3 + 0] = new_index[v0[k]]; dst[at * 3 + 1] = new_index[s[1]]; dst[at * 3 + 2] = new_index[s[2]];
        ++at;
      }
  }
}
// ---- the tile-local format
constexpr int kSfTableThreads = 1024;
__device__ __forceinline__ size_t sf_align16(size_t n) { return (n + 15u) & ~(size_t)15u; }
// kept triangles before old triangle t (t <= nt): the block's prefix, the lane's inside the block, then at most three flags
__device__ __forceinline__ uint32_t sf_triangles_before(uint32_t t, uint32_t nv, uint32_t nt, const uint32_t* __restrict__ tri, const uint8_t* __restrict__ keep,
                                                        const unsigned long long* __restrict__ triangle_sums, const uint16_t* __restrict__ tri_local) {
  if (t >= nt) return (uint32_t)triangle_sums[sf_scan_blocks(nt)];
  const uint32_t g = t / kSfScanPerThread;
  uint32_t n = (uint32_t)triangle_sums[t / kSfScanPerBlock] + tri_local[g];
  for (uint32_t u = g * kSfScanPerThread; u < t; ++u) { const uint32_t v0 = tri[(size_t)u * 3]; n += v0 < nv ? (uint32_t)keep[v0] : 0u; }
  return n;
}
__global__ __launch_bounds__(kSfTableThreads) void k_sf_table(const MeshStreamHeader* __restrict__ raw, uint32_t stride, const MeshTileRow* __restrict__ raw_table,
                                                              const uint8_t* __restrict__ keep, const uint32_t* __restrict__ new_index,
                                                              const unsigned long long* __restrict__ vertex_sums, const unsigned long long* __restrict__ triangle_sums,
                                                              const uint16_t* __restrict__ tri_local, uint8_t* __restrict__ payload, uint32_t* __restrict__ words) {
  __shared__ uint32_t s_wave[kSfTableThreads / 64];
  const uint32_t nv = (uint32_t)raw->n_vertices, nt = (uint32_t)raw->n_triangles, rows = nv ? (uint32_t)raw->needed_tiles : 0u;   // (an overflowed frame emitted no row)
  uint32_t base = 0;
  if (rows) {
    const uint32_t kept_vertices = (uint32_t)vertex_sums[sf_scan_blocks(nv)];
    const uint32_t* __restrict__ tri = sf_raw_triangles(raw, nv, stride);
    uint4* __restrict__ out = (uint4*)(payload + sf_align16((size_t)kept_vertices * stride));
    if (threadIdx.x == 0 && (((size_t)kept_vertices * stride) & 8u)) *(uint2*)(payload + (size_t)kept_vertices * stride) = make_uint2(0u, 0u);   // the padding
    for (uint32_t r0 = 0; r0 < rows; r0 += kSfTableThreads) {          // (uniform: the barriers inside are met by all)
      const uint32_t r = r0 + threadIdx.x;
      MeshTileRow row{0u, 0u, 0u, 0u};
      uint32_t first = 0, end = 0;
      if (r < rows) {                                                  // (every row owns a vertex: first_vertex < nv)
        row = raw_table[r];
        first = new_index[row.first_vertex];
        end = r + 1 < rows ? new_index[raw_table[r + 1].first_vertex] : kept_vertices;
      }
      uint32_t total;
      const uint32_t at = base + block_exclusive_sum<kSfTableThreads / 64>(end > first ? 1u : 0u, s_wave, &total);
      if (end > first) {                                               // (at < rows <= max_tiles)
        const uint32_t t0 = sf_triangles_before(row.first_triangle, nv, nt, tri, keep, triangle_sums, tri_local);
        const uint32_t t1 = sf_triangles_before(row.first_triangle + row.n_triangles, nv, nt, tri, keep, triangle_sums, tri_local);
        out[at] = make_uint4(row.tile, first, t0, t1 - t0);
      }
      base += total;
    }
  }
  if (threadIdx.x == 0) words[2] = base;
}
// the last row of table[from .. rows) whose column (first_triangle / first_vertex) is <= key; the caller knows that row `from`'s is
template <bool kByTriangle>
__device__ __forceinline__ uint32_t sf_row_of(const MeshTileRow* __restrict__ table, uint32_t from, uint32_t rows, uint32_t key) {
  uint32_t lo = from, hi = rows;
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1, c = kByTriangle ? table[mid].first_triangle : table[mid].first_vertex;
    if (c <= key) lo = mid; else hi = mid;
  }
  return lo;
}
__global__ __launch_bounds__(kCcThreads) void k_sf_scatter_triangles_compact(const MeshStreamHeader* __restrict__ raw, uint32_t stride, const MeshTileRow* __restrict__ raw_table,
                                                                             int ntx, int nty, const uint8_t* __restrict__ keep,
                                                                             const unsigned long long* __restrict__ vertex_sums, const unsigned long long* __restrict__ triangle_sums,
                                                                             const uint32_t* __restrict__ new_index, const uint32_t* __restrict__ words, uint8_t* __restrict__ payload) {
  __shared__ uint32_t s_wave[kCcThreads / 64];
  const uint32_t nv = (uint32_t)raw->n_vertices, nt = (uint32_t)raw->n_triangles, nb = sf_scan_blocks(nt), rows = (uint32_t)raw->needed_tiles;
  if (blockIdx.x >= nb) return;
  const uint32_t* __restrict__ tri = sf_raw_triangles(raw, nv, stride);
  uint16_t* __restrict__ dst = (uint16_t*)(payload + sf_align16((size_t)vertex_sums[sf_scan_blocks(nv)] * stride) + (size_t)words[2] * sizeof(MeshTileRow));
  for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const size_t first = ((size_t)b * kCcThreads + threadIdx.x) * kSfScanPerThread;
    uint32_t v0[kSfScanPerThread], flags = 0;
#pragma unroll
    for (int k = 0; k < kSfScanPerThread; ++k) {
      v0[k] = first + k < nt ? tri[(first + k) * 3] : 0xffffffffu;
      if (v0[k] < nv && keep[v0[k]]) flags |= 1u << k;
    }
    uint32_t total;
    size_t at = (size_t)triangle_sums[b] + block_exclusive_sum<kCcThreads / 64>((uint32_t)__popc(flags), s_wave, &total);
    for (int k = 0; k < kSfScanPerThread; ++k)
      if (flags & (1u << k)) {
        const uint32_t* __restrict__ s = tri + (first + k) * 3;
        const uint32_t r = sf_row_of<true>(raw_table, 0u, rows, (uint32_t)(first + k)), cell = raw_table[r].tile;
        const int cx = (int)(cell % (uint32_t)ntx), cy = (int)(cell / (uint32_t)ntx % (uint32_t)nty), cz = (int)(cell / (uint32_t)(ntx * nty));
        for (int c = 0; c < 3; ++c) {                                    // (the owner's tile is the cell's or a +x / +y / +z neighbour: its row is r or behind it)
          const uint32_t i = s[c];
          const MeshTileRow owner = raw_table[sf_row_of<false>(raw_table, r, rows, i)];
          const int ox = (int)(owner.tile % (uint32_t)ntx), oy = (int)(owner.tile / (uint32_t)ntx % (uint32_t)nty), oz = (int)(owner.tile / (uint32_t)(ntx * nty));
          const uint32_t code = (uint32_t)((ox - cx) | ((oy - cy) << 1) | ((oz - cz) << 2));
          dst[at * 3 + c] = (uint16_t)((new_index[i] - new_index[owner.first_vertex]) | (code << 12));
        }
        ++at;
      }
  }
}
// one lane: needs, capacities and overflow from the raw header, the counts from the scans' totals (compact: the filtered rows' number from k_sf_table)
__global__ void k_sf_header(const MeshStreamHeader* __restrict__ raw, const unsigned long long* __restrict__ vertex_sums, const unsigned long long* __restrict__ triangle_sums,
                            const uint32_t* __restrict__ words, uint32_t compact, MeshStreamHeader* __restrict__ H, MeshStreamFilterRecord* __restrict__ record) {
  MeshStreamHeader h = *raw;
  const uint32_t nv = (uint32_t)h.n_vertices, nt = (uint32_t)h.n_triangles;
  MeshStreamFilterRecord r{};
  if (nv) {
    h.n_vertices = vertex_sums[sf_scan_blocks(nv)]; h.n_triangles = triangle_sums[sf_scan_blocks(nt)];
    r.components = words[0]; r.kept = words[1]; r.vertices_removed = nv - h.n_vertices; r.triangles_removed = nt - h.n_triangles;
    r.table_rows = compact ? words[2] : 0u;
  }
  *H = h; *record = r;
}

// ---- launchers
static dim3 sf_grid(size_t capacity, int per_block) {
  size_t n = (capacity + (size_t)per_block - 1) / (size_t)per_block;
  if (kSfGridCap && n > kSfGridCap) n = kSfGridCap;
  return dim3((unsigned)(n ? n : 1));
}
size_t mesh_stream_filter_scan_words(uint32_t capacity) { return ((size_t)capacity + kSfScanPerBlock - 1) / kSfScanPerBlock + 1; }
void launch_mesh_stream_filter(hipStream_t st, const MeshStreamFilter& F, void* payload) {
  const dim3 b(kCcThreads);
  const MeshStreamHeader* raw = F.raw;
  hipLaunchKernelGGL(k_sf_init, sf_grid(F.max_vertices, kCcThreads), b, 0, st, raw, F.parent, F.count, F.words);
  hipLaunchKernelGGL(k_sf_hook, sf_grid(F.max_triangles, kCcChunk), b, 0, st, raw, F.stride, F.parent);
  hipLaunchKernelGGL(k_sf_flatten, sf_grid(F.max_vertices, kCcThreads), b, 0, st, raw, F.parent, F.label);
  hipLaunchKernelGGL(k_sf_count, sf_grid(F.max_triangles, kSfCountPerBlock), b, 0, st, raw, F.stride, F.label, F.count);
  hipLaunchKernelGGL(k_sf_keep, sf_grid(F.max_vertices, kSfScanPerBlock), b, 0, st, raw, F.label, F.count, F.min_triangles, F.keep, F.vertex_sums, F.words);
  if (F.raw_table) {                                                     // the tile-local format: the same scans, then rows and codes
    hipLaunchKernelGGL(k_sf_triangle_sums<true>, sf_grid(F.max_triangles, kSfScanPerBlock), b, 0, st, raw, F.stride, F.keep, F.triangle_sums, F.tri_local);
    hipLaunchKernelGGL(k_sf_scan_sums, dim3(2), b, 0, st, raw, F.vertex_sums, F.triangle_sums);
    if (F.stride == 8u) hipLaunchKernelGGL((k_sf_scatter_vertices<uint2, true>), sf_grid(F.max_vertices, kSfScanPerBlock), b, 0, st, raw, F.keep, F.vertex_sums, F.parent, (uint2*)payload);
    else hipLaunchKernelGGL((k_sf_scatter_vertices<uint4, true>), sf_grid(F.max_vertices, kSfScanPerBlock), b, 0, st, raw, F.keep, F.vertex_sums, F.parent, (uint4*)payload);
    hipLaunchKernelGGL(k_sf_table, dim3(1), dim3(kSfTableThreads), 0, st, raw, F.stride, F.raw_table, F.keep, F.parent, F.vertex_sums, F.triangle_sums, F.tri_local, (uint8_t*)payload, F.words);
    hipLaunchKernelGGL(k_sf_scatter_triangles_compact, sf_grid(F.max_triangles, kSfScanPerBlock), b, 0, st, raw, F.stride, F.raw_table, F.ntx, F.nty, F.keep, F.vertex_sums,
                       F.triangle_sums, F.parent, F.words, (uint8_t*)payload);
    return;
  }
  hipLaunchKernelGGL(k_sf_triangle_sums<false>, sf_grid(F.max_triangles, kSfScanPerBlock), b, 0, st, raw, F.stride, F.keep, F.triangle_sums, (uint16_t*)nullptr);
  hipLaunchKernelGGL(k_sf_scan_sums, dim3(2), b, 0, st, raw, F.vertex_sums, F.triangle_sums);
  if (F.stride == 8u) hipLaunchKernelGGL((k_sf_scatter_vertices<uint2, false>), sf_grid(F.max_vertices, kSfScanPerBlock), b, 0, st, raw, F.keep, F.vertex_sums, F.parent, (uint2*)payload);
  else hipLaunchKernelGGL((k_sf_scatter_vertices<uint4, false>), sf_grid(F.max_vertices, kSfScanPerBlock), b, 0, st, raw, F.keep, F.vertex_sums, F.parent, (uint4*)payload);
  hipLaunchKernelGGL(k_sf_scatter_triangles, sf_grid(F.max_triangles, kSfScanPerBlock), b, 0, st, raw, F.stride, F.keep, F.vertex_sums, F.triangle_sums, F.parent, (uint8_t*)payload);
}
void launch_mesh_stream_filter_header(hipStream_t st, const MeshStreamFilter& F, MeshStreamHeader* H, MeshStreamFilterRecord* record) {
  hipLaunchKernelGGL(k_sf_header, dim3(1), dim3(1), 0, st, F.raw, F.vertex_sums, F.triangle_sums, F.words, F.raw_table ? 1u : 0u, H, record);
}

}  // namespace rr
