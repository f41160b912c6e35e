// Mesh extraction: the fused surface as an indexed triangle mesh (tsdf_mesh_extract, include/rgbd_recon_hip.h has the definition).
// The reference has no counterpart; the entry is built on what the raymarch already restates: the hit test f > 0
// (tsdf_raymarch.fs:96), get_gradient (:140-149), blendColors (:295-330) and vol_to_world (recon_integration.cpp:66-72,199).
//
// Marching tetrahedra on the voxel-centre lattice, Kuhn's six tetrahedra per cell.  One workgroup per 8^3 storage tile, one lane per
// lattice point: a lattice point p owns the seven edges p -> p + d (d = 1..7 as a bit offset) and, where it is the origin of a cell,
// that cell's triangles.  Five launches, each a plain function of its inputs -- no atomic decides a position and no workgroup waits
// for another, so the output order (tile, lattice point, d / tetrahedron, triangle) is the same on every run:
//   k_mesh_count      per tile: vertices and triangles (a tile whose own class and whose +x/+y/+z neighbours' are kTileMinus reads nothing)
//   k_mesh_block_sums / k_mesh_scan_sums / k_mesh_scan_apply   exclusive scan of the per-tile counts (64-bit totals) and a compact
//                     record slot for every tile with surface
//   k_mesh_vertices   per tile with surface: a record per lattice point {edge mask, inside bit, vertex offset in the tile} and the
//                     vertices (position, optionally normal and colour), one lane per vertex
//   k_mesh_triangles  per tile with triangles: reads the records only (never the volume); the index of an edge owned by lattice point
//                     q is tile_vbase[tile of q] + record(q).offset + popcount(record(q).mask below d)
// Level of detail (tsdf_mesh_extract_lod, level 1 and 2): the same launches on the lattice of every 2nd / 4th voxel.  "Tile" and "lattice point" above
// then mean a tile of 8^3 LATTICE points ((8 << level)^3 voxels) and its points; MeshLattice holds that geometry.  Every kernel that knows the lattice is
// instantiated per level; level 0 is the text it was, the lattice being the voxel grid.  A vertex of a coarse edge is the level-0 vertex of the voxel edge a
// bisection along the edge ends on (mesh_descend: `level` voxel reads), so no position is interpolated over more than one voxel.
#include "tsdf_common.hpp"

namespace rr {
// Kuhn's six tetrahedra along the diagonal c0 - c7 (corner b = bx + 2 by + 4 bz).  Every vertex list is a chain of bit sets, so every
// tetrahedron edge runs from a corner to one that contains it: the edge (x, y), x < y, is edge d = y - x of lattice point p + x.
__constant__ uint8_t c_tet[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
// Winding: bit `case` of row `tetrahedron` set = emit the triangle(s) of that case reversed.  case = sum of 1 << k over the inside
// vertices v_k.  Tetrahedra 0, 3, 4 are positively oriented, 1, 2, 5 negatively; generated from the rule "the geometric normal points
// from the inside corners to the outside corners" (tests/mesh_reference.py: winding_table(), which the CPU tests compare with these words).
__constant__ uint16_t c_mesh_flip[6] = {0x4d24, 0x32da, 0x32da, 0x4d24, 0x4d24, 0x32da};
}  // namespace rr
#define RR_MESH_TABLES_DEFINED   // (mesh_dev.hpp asks for it: its functions read the two tables)

#include "mesh_dev.hpp"
#include "scan_dev.hpp"

namespace rr {

constexpr int kScanThreads = 256, kScanPerThread = 4, kScanPerBlock = kScanThreads * kScanPerThread;

// every stage's body is mesh_dev.hpp's; the kernels here name the whole volume's tiles (WholeTiles)
// ---- 1. count
template <bool kSparse, int kLevel>
__global__ __launch_bounds__(kMeshThreads) void k_mesh_count(Volume V, uint2* __restrict__ tile_cnt, uint8_t* __restrict__ tile_skip) {
  mesh_tile_count<kSparse, kLevel>(V, WholeTiles{}, tile_cnt, tile_skip);
}

// ---- 2. scan of the per-tile counts: block sums, scan of the block sums, add.  Four quantities: vertices, triangles, tiles with
// surface, tiles skipped by class.  A block covers kScanPerBlock tiles, so its own sums fit 32 bits; everything across blocks is 64-bit.
__device__ __forceinline__ void scan_load(const uint2* __restrict__ tile_cnt, const uint8_t* __restrict__ tile_skip, int n, uint2 c[kScanPerThread], uint32_t sk[kScanPerThread]) {
  const int first = ((int)blockIdx.x * kScanThreads + (int)threadIdx.x) * kScanPerThread;
#pragma unroll
  for (int k = 0; k < kScanPerThread; ++k) {
    const bool in = first + k < n;
    c[k] = in ? tile_cnt[first + k] : make_uint2(0u, 0u);
    sk[k] = in ? (uint32_t)tile_skip[first + k] : 0u;
  }
}
__global__ __launch_bounds__(kScanThreads) void k_mesh_block_sums(const uint2* __restrict__ tile_cnt, const uint8_t* __restrict__ tile_skip, int n, MeshSums* __restrict__ sums) {
  __shared__ uint32_t s_wave[kScanThreads / 64];
  uint2 c[kScanPerThread]; uint32_t sk[kScanPerThread];
  scan_load(tile_cnt, tile_skip, n, c, sk);
  uint32_t nv = 0, nt = 0, flags = 0;
#pragma unroll
  for (int k = 0; k < kScanPerThread; ++k) { nv += c[k].x; nt += c[k].y; flags += (c[k].x ? 1u : 0u) | (sk[k] << 16); }
  uint32_t tv, tt, tf;
  block_exclusive_sum<kScanThreads / 64>(nv, s_wave, &tv);
  block_exclusive_sum<kScanThreads / 64>(nt, s_wave, &tt);
  block_exclusive_sum<kScanThreads / 64>(flags, s_wave, &tf);
  if (threadIdx.x == 0) sums[blockIdx.x] = MeshSums{tv, tt, tf & 0xffffu, tf >> 16};
}
// one workgroup: sums[0 .. nb) become exclusive prefixes, sums[nb] the totals.  Every lane takes a contiguous run of blocks.
__global__ __launch_bounds__(kScanThreads) void k_mesh_scan_sums(MeshSums* __restrict__ sums, int nb) {
  __shared__ MeshSums s_run[kScanThreads];
  const int per = (nb + kScanThreads - 1) / kScanThreads, b0 = min((int)threadIdx.x * per, nb), b1 = min(b0 + per, nb);
  MeshSums run{0, 0, 0, 0};
  for (int b = b0; b < b1; ++b) { const MeshSums s = sums[b]; run.nv += s.nv; run.nt += s.nt; run.surface += s.surface; run.skipped += s.skipped; }
  s_run[threadIdx.x] = run;
  __syncthreads();
  if (threadIdx.x == 0) {
    MeshSums acc{0, 0, 0, 0};
    for (int k = 0; k < kScanThreads; ++k) {
      const MeshSums s = s_run[k];
      s_run[k] = acc;
      acc.nv += s.nv; acc.nt += s.nt; acc.surface += s.surface; acc.skipped += s.skipped;
    }
    sums[nb] = acc;
  }
  __syncthreads();
  MeshSums acc = s_run[threadIdx.x];
  for (int b = b0; b < b1; ++b) {
    const MeshSums s = sums[b];
    sums[b] = acc;
    acc.nv += s.nv; acc.nt += s.nt; acc.surface += s.surface; acc.skipped += s.skipped;
  }
}
__global__ __launch_bounds__(kScanThreads) void k_mesh_scan_apply(const uint2* __restrict__ tile_cnt, const uint8_t* __restrict__ tile_skip, int n, const MeshSums* __restrict__ sums,
                                                                  uint32_t* __restrict__ tile_vbase, unsigned long long* __restrict__ tile_tbase, uint32_t* __restrict__ tile_rec) {
  __shared__ uint32_t s_wave[kScanThreads / 64];
  uint2 c[kScanPerThread]; uint32_t sk[kScanPerThread];
  scan_load(tile_cnt, tile_skip, n, c, sk);
  uint32_t nv = 0, nt = 0, ns = 0;
#pragma unroll
  for (int k = 0; k < kScanPerThread; ++k) { nv += c[k].x; nt += c[k].y; ns += c[k].x ? 1u : 0u; }
  uint32_t total;
  const MeshSums base = sums[blockIdx.x];
  unsigned long long v = base.nv + block_exclusive_sum<kScanThreads / 64>(nv, s_wave, &total);
  unsigned long long t = base.nt + block_exclusive_sum<kScanThreads / 64>(nt, s_wave, &total);
  unsigned long long s = base.surface + block_exclusive_sum<kScanThreads / 64>(ns, s_wave, &total);
  const int first = ((int)blockIdx.x * kScanThreads + (int)threadIdx.x) * kScanPerThread;
#pragma unroll
  for (int k = 0; k < kScanPerThread; ++k)
    if (first + k < n) {
      tile_vbase[first + k] = (uint32_t)v;                             // (the host refuses a mesh whose vertices do not fit 32 bits before anything reads this)
      tile_tbase[first + k] = t;
      tile_rec[first + k] = c[k].x ? (uint32_t)s : kNoSlot;
      v += c[k].x; t += c[k].y; s += c[k].x ? 1u : 0u;
    }
}

// ---- 3. records and vertices
template <bool kSparse, int kLevel>
__global__ __launch_bounds__(kMeshThreads) void k_mesh_vertices(Volume V, StreamTable T, FrameImages F, MeshGeometry G, const uint2* __restrict__ tile_cnt,
                                                                const uint32_t* __restrict__ tile_vbase, const uint32_t* __restrict__ tile_rec, uint32_t* __restrict__ records,
                                                                float* __restrict__ out_pos, float* __restrict__ out_nrm, float4* __restrict__ out_col) {
  __shared__ MeshVertexStage s;
  const LatticeOf<kLevel> L(V);
  const MeshTile t = mesh_tile(L, WholeTiles{});
  const uint32_t nv = tile_cnt[t.id].x;
  if (nv == 0 || !mesh_tile_records<kSparse, kLevel>(V, L, WholeTiles{}, t, tile_rec, records, s)) return;
  mesh_tile_vertices<kSparse, kLevel>(V, T, F, G, t, nv, s.f, s.edge, (size_t)tile_vbase[t.id], out_pos, out_nrm, out_col);
}

// ... and the streamed form (tsdf_mesh_stream): the same records, then the tile's vertices quantised in registers and written with ONE 8- or 16-byte
// store each (mesh_tile_vertices_packed).  H is the frame's header in device memory (k_mesh_stream_header): when a need exceeds its capacity every
// workgroup of both emit kernels returns before it reads anything else, so nothing is ever written past a capacity.
template <bool kSparse, uint32_t kFlags, int kLevel>
__global__ __launch_bounds__(kMeshThreads, 4) void k_mesh_vertices_packed(Volume V, StreamTable T, FrameImages F, MeshGeometry G, const MeshStreamHeader* __restrict__ H,
                                                                          const uint2* __restrict__ tile_cnt, const uint32_t* __restrict__ tile_vbase,
                                                                          const uint32_t* __restrict__ tile_rec, uint32_t* __restrict__ records, void* __restrict__ out) {
  __shared__ MeshVertexStage s;
  const LatticeOf<kLevel> L(V);
  const MeshTile t = mesh_tile(L, WholeTiles{});
  const uint32_t nv = tile_cnt[t.id].x;                                // (read beside the header, not behind it: one wait for both; tile_cnt is valid on overflow too)
  if (mesh_stream_overflow(H) || nv == 0 || !mesh_tile_records<kSparse, kLevel>(V, L, WholeTiles{}, t, tile_rec, records, s)) return;
  mesh_tile_vertices_packed<kSparse, kFlags, kLevel>(V, T, F, G, t, nv, s.f, s.edge, (size_t)tile_vbase[t.id], out);   // (< needed_vertices <= max_vertices)
}

// ---- 4. triangles, from the records alone
template <int kLevel>
__global__ __launch_bounds__(kMeshThreads) void k_mesh_triangles(Volume V, const uint2* __restrict__ tile_cnt, const uint32_t* __restrict__ tile_vbase,
                                                                 const unsigned long long* __restrict__ tile_tbase, const uint32_t* __restrict__ tile_rec,
                                                                 const uint32_t* __restrict__ records, uint32_t* __restrict__ out_tri) {
  mesh_tile_triangles<kLevel>(V, WholeTiles{}, tile_cnt, tile_vbase, tile_tbase, tile_rec, records, MeshSlabLink{}, out_tri);
}
// the streamed form: the triangle array follows the frame's vertices directly (payload + needed_vertices * stride: one copy takes both)
template <int kLevel>
__global__ __launch_bounds__(kMeshThreads) void k_mesh_triangles_stream(Volume V, const MeshStreamHeader* __restrict__ H, const uint2* __restrict__ tile_cnt,
                                                                        const uint32_t* __restrict__ tile_vbase, const unsigned long long* __restrict__ tile_tbase,
                                                                        const uint32_t* __restrict__ tile_rec, const uint32_t* __restrict__ records,
                                                                        uint8_t* __restrict__ payload, uint32_t stride) {
  if (mesh_stream_overflow(H)) return;
  mesh_tile_triangles<kLevel>(V, WholeTiles{}, tile_cnt, tile_vbase, tile_tbase, tile_rec, records, MeshSlabLink{}, (uint32_t*)(payload + (size_t)H->needed_vertices * stride));
}
// The tile-local format (launch_mesh_stream_emit_compact, and a slab's part of it: launch_mesh_part_emit): the tile table, one lane per tile of the frame
// -- the whole volume's n lattice tiles, or a part's n owned ones, the first of which is first_tile in the WHOLE level's grid (the two bases stay
// part-local).  A tile with a vertex writes its row at its surface ordinal (tile_rec: the rows are the surface tiles in tile order) as one 16-byte store;
// the row area begins at a multiple of 16 bytes -- in the payload behind the vertices and their zero padding, or at raw_table (the filter's raw frame, whose
// payload is the uint32 one).  In a launch of its own: folded into the triangle launch (lane 0 of a tile's workgroup) it measured slower at level 0.
__global__ __launch_bounds__(kScanThreads) void k_mesh_stream_table(const MeshStreamHeader* __restrict__ H, const uint2* __restrict__ tile_cnt, const uint32_t* __restrict__ tile_vbase,
                                                                    const unsigned long long* __restrict__ tile_tbase, const uint32_t* __restrict__ tile_rec, int n,
                                                                    uint32_t first_tile, uint8_t* __restrict__ payload, uint32_t stride, MeshTileRow* __restrict__ raw_table) {
  const int t = (int)(blockIdx.x * kScanThreads + threadIdx.x);
  if (mesh_stream_overflow(H) || t >= n) return;
  const size_t vertex_bytes = (size_t)H->needed_vertices * stride;
  if (!raw_table && t == 0 && (vertex_bytes & 8u)) *(uint2*)(payload + vertex_bytes) = make_uint2(0u, 0u);   // the padding
  const uint2 cnt = tile_cnt[t];
  if (cnt.x)                                                             // (tile_rec < needed_tiles <= max_tiles)
    *(uint4*)((raw_table ? raw_table : mesh_stream_table(H, payload, stride)) + tile_rec[t]) = make_uint4(first_tile + (uint32_t)t, tile_vbase[t], (uint32_t)tile_tbase[t], cnt.y);
}
// ... and the 6-byte triangles, behind the vertices, the padding and the needed_tiles table rows -- all inside the slot, as none of the three needs exceeds
// its capacity
template <int kLevel>
__global__ __launch_bounds__(kMeshThreads) void k_mesh_triangles_stream_compact(Volume V, const MeshStreamHeader* __restrict__ H, const uint2* __restrict__ tile_cnt,
                                                                                const uint32_t* __restrict__ tile_vbase, const unsigned long long* __restrict__ tile_tbase,
                                                                                const uint32_t* __restrict__ tile_rec, const uint32_t* __restrict__ records,
                                                                                uint8_t* __restrict__ payload, uint32_t stride) {
  if (mesh_stream_overflow(H)) return;
  mesh_tile_triangles<kLevel>(V, WholeTiles{}, tile_cnt, tile_vbase, tile_tbase, tile_rec, records, MeshSlabLink{}, (uint16_t*)(mesh_stream_table(H, payload, stride) + H->needed_tiles));
}
// one lane: the frame's header from the scan's totals (sums[nb]) and the ring's capacities
__global__ void k_mesh_stream_header(const MeshSums* __restrict__ totals, MeshStreamHeader* __restrict__ H, uint32_t max_vertices, uint32_t max_triangles, uint32_t max_tiles) {
  const MeshSums s = *totals;
  *H = mesh_stream_header(s.nv, s.nt, s.surface, s.skipped, max_vertices, max_triangles, max_tiles);
}

// ---- launchers.  S.level picks the instantiation; the caller has checked it (0 .. kMeshMaxLevel) and sized S by mesh_lattice(res, level).
int mesh_scan_blocks(int n_tiles) { return (n_tiles + kScanPerBlock - 1) / kScanPerBlock; }
void launch_mesh_count(hipStream_t st, const Volume& V, const MeshScratch& S) {
  mesh_instantiation(V, S, [&](auto sparse, auto level) {
    hipLaunchKernelGGL((k_mesh_count<decltype(sparse)::value, decltype(level)::value>), dim3(S.n_tiles), dim3(kMeshThreads), 0, st, V, S.tile_cnt, S.tile_skip);
  });
}
void launch_mesh_scan(hipStream_t st, const MeshScratch& S) {
  const int nb = mesh_scan_blocks(S.n_tiles);
  MeshSums* sums = (MeshSums*)S.sums;
  hipLaunchKernelGGL(k_mesh_block_sums, dim3(nb), dim3(kScanThreads), 0, st, S.tile_cnt, S.tile_skip, S.n_tiles, sums);
  hipLaunchKernelGGL(k_mesh_scan_sums, dim3(1), dim3(kScanThreads), 0, st, sums, nb);
  hipLaunchKernelGGL(k_mesh_scan_apply, dim3(nb), dim3(kScanThreads), 0, st, S.tile_cnt, S.tile_skip, S.n_tiles, sums, S.tile_vbase, S.tile_tbase, S.tile_rec);
}
void launch_mesh_emit(hipStream_t st, const Volume& V, const StreamTable& T, const FrameImages& F, const MeshGeometry& G, const MeshScratch& S, uint32_t* records,
                      float* pos, float* nrm, float* col, uint32_t* tri) {
  mesh_instantiation(V, S, [&](auto sparse, auto level) {
    constexpr bool kSparse = decltype(sparse)::value;
    constexpr int kLevel = decltype(level)::value;
    hipLaunchKernelGGL((k_mesh_vertices<kSparse, kLevel>), dim3(S.n_tiles), dim3(kMeshThreads), 0, st, V, T, F, G, S.tile_cnt, S.tile_vbase, S.tile_rec, records, pos, nrm, (float4*)col);
    hipLaunchKernelGGL(k_mesh_triangles<kLevel>, dim3(S.n_tiles), dim3(kMeshThreads), 0, st, V, S.tile_cnt, S.tile_vbase, S.tile_tbase, S.tile_rec, records, tri);
  });
}

// the streamed form's emit: header, packed vertices, triangles.  payload: max_vertices * stride + max_triangles * 12 bytes; records: 512 words for each
// of max_tiles tiles.  A lattice thinner than 2 on an axis has no cell: the caller launches nothing but the header then (S.n_tiles == 0 is not a case).
void launch_mesh_stream_header(hipStream_t st, const MeshScratch& S, MeshStreamHeader* H, uint32_t max_vertices, uint32_t max_triangles, uint32_t max_tiles) {
  hipLaunchKernelGGL(k_mesh_stream_header, dim3(1), dim3(1), 0, st, (const MeshSums*)S.sums + mesh_scan_blocks(S.n_tiles), H, max_vertices, max_triangles, max_tiles);
}
void launch_mesh_stream_table(hipStream_t st, const MeshScratch& S, const MeshStreamHeader* H, int n, uint32_t first_tile, void* payload, uint32_t stride, MeshTileRow* raw_table) {
  hipLaunchKernelGGL(k_mesh_stream_table, dim3((n + kScanThreads - 1) / kScanThreads), dim3(kScanThreads), 0, st, H, S.tile_cnt, S.tile_vbase, S.tile_tbase, S.tile_rec, n, first_tile,
                     (uint8_t*)payload, stride, raw_table);
}
// compact: the tile-local format -- the same packed vertices (the same kernel), the table, then the 6-byte triangles, or, with raw_table (the filter's raw
// frame), the uint32 triangles of the plain ring
static void mesh_stream_emit(hipStream_t st, const Volume& V, const StreamTable& T, const FrameImages& F, const MeshGeometry& G, const MeshScratch& S, uint32_t flags,
                             const MeshStreamHeader* H, uint32_t* records, void* payload, bool compact, MeshTileRow* raw_table) {
  mesh_packed_instantiation(V, S, flags, [&](auto sparse, auto level, auto vertex_flags) {
    constexpr int kLevel = decltype(level)::value;
    const dim3 g(S.n_tiles), b(kMeshThreads);
    const uint32_t stride = flags ? 16u : 8u;
    hipLaunchKernelGGL((k_mesh_vertices_packed<decltype(sparse)::value, decltype(vertex_flags)::value, kLevel>), g, b, 0, st, V, T, F, G, H, S.tile_cnt, S.tile_vbase, S.tile_rec,
                       records, payload);
    if (compact) launch_mesh_stream_table(st, S, H, S.n_tiles, 0u, payload, stride, raw_table);
    if (compact && !raw_table) hipLaunchKernelGGL(k_mesh_triangles_stream_compact<kLevel>, g, b, 0, st, V, H, S.tile_cnt, S.tile_vbase, S.tile_tbase, S.tile_rec, records, (uint8_t*)payload, stride);
    else hipLaunchKernelGGL(k_mesh_triangles_stream<kLevel>, g, b, 0, st, V, H, S.tile_cnt, S.tile_vbase, S.tile_tbase, S.tile_rec, records, (uint8_t*)payload, stride);
  });
}
void launch_mesh_stream_emit(hipStream_t st, const Volume& V, const StreamTable& T, const FrameImages& F, const MeshGeometry& G, const MeshScratch& S, uint32_t flags,
                             const MeshStreamHeader* H, uint32_t* records, void* payload) {
  mesh_stream_emit(st, V, T, F, G, S, flags, H, records, payload, false, nullptr);
}
void launch_mesh_stream_emit_compact(hipStream_t st, const Volume& V, const StreamTable& T, const FrameImages& F, const MeshGeometry& G, const MeshScratch& S, uint32_t flags,
                                     const MeshStreamHeader* H, uint32_t* records, void* payload, MeshTileRow* raw_table) {
  mesh_stream_emit(st, V, T, F, G, S, flags, H, records, payload, true, raw_table);
}

}  // namespace rr
