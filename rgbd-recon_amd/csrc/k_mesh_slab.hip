// Mesh extraction on a Z-slab context: the slab's part of the whole volume's mesh (tsdf_mesh_slab_extract / _link, include/rgbd_recon_hip.h has the
// definition).  The whole mesh is ordered by lattice tile with the tile layer outermost and slabs are tile aligned, so it is the concatenation of the
// slabs' parts; what k_mesh.hip does per tile is done here per OWNED tile: every stage's body is mesh_dev.hpp's, instantiated for SlabTiles, and the scan
// is k_mesh.hip's.
//
// Tiles.  Workgroup b is slab-local tile b: the owned lattice tile layers [layer0, layer0 + n_own / (ntx nty)) first, then -- unless the slab reaches the
// volume's top -- the n_seam = ntx nty tiles of the SEAM layer, the first lattice tile layer of the slab above.  MeshTile::tz is the layer in the whole
// lattice (every voxel read goes through the volume's own tz0), MeshTile::id the slab-local index into the scratch.
// Seam layer.  The cells of the top owned cell layer have corners in plane 0 of the seam layer, whose vertices the slab above emits.  Their indices need
// that plane's lattice-point records {edge mask, inside bit, offset in the tile}: plane 0 comes first in a tile's order, so its offsets depend on
// lattice planes 0 and 1 alone (voxel planes z1 and z1 + stride, inside the halo).  A seam tile is counted and recorded by its 64 plane-0 lanes; it takes
// a record slot from the same scan, counts no triangle, and its vertices are subtracted from the slab's total by the host.
// Link.  k_mesh_slab_triangles reads the records alone.  The first vertex of an owned tile is base + tile_vbase[tile], of a seam tile
// base + (the slab's vertices) + above[tile]: the slab above follows directly in the concatenation and `above` is its tsdf_mesh_slab_seam table.
// As in k_mesh.hip no atomic decides a position and no workgroup waits for another.
// Streamed parts (tsdf_mesh_stream on a ring of tsdf_mesh_stream_config_part; "mesh streaming: slab parts" in the header): the same count and scan, then
// k_mesh_part_header, k_mesh_part_vertices_packed, k_mesh.hip's table launch and k_mesh_part_triangles below -- the slab's part of the tile-local frame,
// whose corner codes name no vertex of another slab by index, so that nothing of the link is needed.
#include "tsdf_common.hpp"

namespace rr {
// k_mesh.hip's two tables, word for word (a __constant__ array belongs to one code object: this file's kernels need their own).  Private to this file;
// tests/test_gpu_mesh_slab.py compares what they produce with k_mesh.hip's output byte for byte.
static __constant__ uint8_t c_tet[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
static __constant__ uint16_t c_mesh_flip[6] = {0x4d24, 0x32da, 0x32da, 0x4d24, 0x4d24, 0x32da};
}  // namespace rr
#define RR_MESH_TABLES_DEFINED   // (mesh_dev.hpp asks for it: its functions read the two tables)

#include "mesh_dev.hpp"

namespace rr {

// ---- count: per slab-local tile, seam tiles included
template <bool kSparse, int kLevel>
__global__ __launch_bounds__(kMeshThreads) void k_mesh_slab_count(Volume V, MeshSlab B, uint2* __restrict__ tile_cnt, uint8_t* __restrict__ tile_skip) {
  mesh_tile_count<kSparse, kLevel>(V, SlabTiles{B}, tile_cnt, tile_skip);
}

// ---- records and vertices: per slab-local tile; a seam tile leaves its records and emits nothing
template <bool kSparse, int kLevel>
__global__ __launch_bounds__(kMeshThreads) void k_mesh_slab_vertices(Volume V, StreamTable T, FrameImages F, MeshGeometry G, MeshSlab B, const uint2* __restrict__ tile_cnt,
                                                                     const uint32_t* __restrict__ tile_vbase, const uint32_t* __restrict__ tile_rec,
                                                                     uint32_t* __restrict__ records, float* __restrict__ out_pos, float* __restrict__ out_nrm,
                                                                     float4* __restrict__ out_col) {
  __shared__ MeshVertexStage s;
  const LatticeOf<kLevel> L(V);
  const MeshTile t = mesh_tile(L, SlabTiles{B});
  const uint32_t nv = tile_cnt[t.id].x;
  if (nv == 0 || !mesh_tile_records<kSparse, kLevel>(V, L, SlabTiles{B}, t, tile_rec, records, s)) return;
  mesh_tile_vertices<kSparse, kLevel>(V, T, F, G, t, nv, s.f, s.edge, (size_t)tile_vbase[t.id], out_pos, out_nrm, out_col);
}

// ---- triangles of the owned tiles (the launch covers them only), with global indices: the link
template <int kLevel>
__global__ __launch_bounds__(kMeshThreads) void k_mesh_slab_triangles(Volume V, MeshSlab B, const uint2* __restrict__ tile_cnt, const uint32_t* __restrict__ tile_vbase,
                                                                      const unsigned long long* __restrict__ tile_tbase, const uint32_t* __restrict__ tile_rec,
                                                                      const uint32_t* __restrict__ records, uint32_t base, uint32_t slab_vertices,
                                                                      const uint32_t* __restrict__ above, uint32_t* __restrict__ out_tri) {
  mesh_tile_triangles<kLevel>(V, SlabTiles{B}, tile_cnt, tile_vbase, tile_tbase, tile_rec, records, MeshSlabLink{base, slab_vertices, above}, out_tri);
}

// ---- the streamed part (tsdf_mesh_stream on a ring of tsdf_mesh_stream_config_part): the slab's part of the tile-local frame, complete without a number
// from another slab.  Count and scan are the extract's, over owned + seam tiles.  Seam tiles sit last in the slab-local scan: the owned tiles' record
// slots are [0, owned tiles with surface) -- the row ordinals --, their vertex and triangle bases part-local, and a seam tile's slot lies behind them, in
// the n_seam slots the ring allocates beyond max_tiles.
// The header: the scan's totals without the seam tiles' vertices and surface count, subtracted HERE (the extract does it on the host; the ring waits for
// nothing).  One workgroup, a reduction over the n_seam counts, lane 0 writes; the record in front of the header carries what was subtracted.
constexpr int kPartHeaderThreads = 256;
__global__ __launch_bounds__(kPartHeaderThreads) void k_mesh_part_header(const MeshSums* __restrict__ totals, const uint2* __restrict__ tile_cnt, MeshSlab B,
                                                                         MeshStreamPartRecord* __restrict__ record, MeshStreamHeader* __restrict__ H, uint32_t max_vertices,
                                                                         uint32_t max_triangles, uint32_t max_tiles) {
  __shared__ uint32_t s_wave[kPartHeaderThreads / 64];
  uint32_t nv = 0, ns = 0;                                             // (a seam tile counts at most 64 * 7 vertices: the sums fit 32 bits at any resolution)
  for (int k = threadIdx.x; k < B.n_seam; k += kPartHeaderThreads) { const uint32_t n = tile_cnt[B.n_own + k].x; nv += n; ns += n ? 1u : 0u; }
  uint32_t seam_vertices, seam_tiles;
  block_exclusive_sum<kPartHeaderThreads / 64>(nv, s_wave, &seam_vertices);
  block_exclusive_sum<kPartHeaderThreads / 64>(ns, s_wave, &seam_tiles);
  if (threadIdx.x != 0) return;
  const MeshSums s = *totals;
  *H = mesh_stream_header(s.nv - seam_vertices, s.nt, s.surface - seam_tiles, s.skipped, max_vertices, max_triangles, max_tiles);   // (a seam tile counts no triangle and no skip)
  MeshStreamPartRecord r{};
  r.seam_tiles = seam_tiles; r.seam_vertices = seam_vertices;
  *record = r;
}
// records of every tile with surface, packed vertices of the owned ones (they come first: < needed_vertices <= max_vertices)
template <bool kSparse, uint32_t kFlags, int kLevel>
__global__ __launch_bounds__(kMeshThreads, 4) void k_mesh_part_vertices_packed(Volume V, StreamTable T, FrameImages F, MeshGeometry G, MeshSlab B,
                                                                               const MeshStreamHeader* __restrict__ H, const uint2* __restrict__ tile_cnt,
                                                                               const uint32_t* __restrict__ tile_vbase, const uint32_t* __restrict__ tile_rec,
                                                                               uint32_t* __restrict__ records, void* __restrict__ out) {
  __shared__ MeshVertexStage s;
  const LatticeOf<kLevel> L(V);
  const MeshTile t = mesh_tile(L, SlabTiles{B});
  const uint32_t nv = tile_cnt[t.id].x;                                // (read beside the header, as in k_mesh_vertices_packed; tile_rec < needed_tiles + seam tiles <= max_tiles + n_seam)
  if (mesh_stream_overflow(H) || nv == 0 || !mesh_tile_records<kSparse, kLevel>(V, L, SlabTiles{B}, t, tile_rec, records, s)) return;
  mesh_tile_vertices_packed<kSparse, kFlags, kLevel>(V, T, F, G, t, nv, s.f, s.edge, (size_t)tile_vbase[t.id], out);
}
// ... and the 6-byte triangles behind the rows: exactly the codes of the whole volume's compact frame (a code names no part)
template <int kLevel>
__global__ __launch_bounds__(kMeshThreads) void k_mesh_part_triangles(Volume V, MeshSlab B, const MeshStreamHeader* __restrict__ H, const uint2* __restrict__ tile_cnt,
                                                                      const uint32_t* __restrict__ tile_vbase, const unsigned long long* __restrict__ tile_tbase,
                                                                      const uint32_t* __restrict__ tile_rec, const uint32_t* __restrict__ records,
                                                                      uint8_t* __restrict__ payload, uint32_t stride) {
  if (mesh_stream_overflow(H)) return;
  mesh_tile_triangles<kLevel>(V, SlabTiles{B}, tile_cnt, tile_vbase, tile_tbase, tile_rec, records, MeshSlabLink{}, (uint16_t*)(mesh_stream_table(H, payload, stride) + H->needed_tiles));
}

// ---- launchers.  S: the scratch over B.n_own + B.n_seam tiles, S.level the instantiation (the caller has checked it)
void launch_mesh_slab_count(hipStream_t st, const Volume& V, const MeshScratch& S, const MeshSlab& B) {
  mesh_instantiation(V, S, [&](auto sparse, auto level) {
    hipLaunchKernelGGL((k_mesh_slab_count<decltype(sparse)::value, decltype(level)::value>), dim3(S.n_tiles), dim3(kMeshThreads), 0, st, V, B, S.tile_cnt, S.tile_skip);
  });
}
void launch_mesh_slab_vertices(hipStream_t st, const Volume& V, const StreamTable& T, const FrameImages& F, const MeshGeometry& G, const MeshScratch& S, const MeshSlab& B,
                               uint32_t* records, float* pos, float* nrm, float* col) {
  mesh_instantiation(V, S, [&](auto sparse, auto level) {
    hipLaunchKernelGGL((k_mesh_slab_vertices<decltype(sparse)::value, decltype(level)::value>), dim3(S.n_tiles), dim3(kMeshThreads), 0, st, V, T, F, G, B, S.tile_cnt,
                       S.tile_vbase, S.tile_rec, records, pos, nrm, (float4*)col);
  });
}
void launch_mesh_slab_triangles(hipStream_t st, const Volume& V, const MeshScratch& S, const MeshSlab& B, const uint32_t* records, uint32_t base, uint32_t slab_vertices,
                                const uint32_t* above, uint32_t* tri) {
  mesh_instantiation(V, S, [&](auto, auto level) {
    hipLaunchKernelGGL(k_mesh_slab_triangles<decltype(level)::value>, dim3(B.n_own), dim3(kMeshThreads), 0, st, V, B, S.tile_cnt, S.tile_vbase, S.tile_tbase, S.tile_rec,
                       records, base, slab_vertices, above, tri);
  });
}
// the streamed part: header (behind launch_mesh_slab_count and launch_mesh_scan), then the emit.  record: 64 bytes in front of H; records: 512 words for
// each of max_tiles + B.n_seam tiles; payload: the tile-local format's capacity (result_paths.hpp: MeshFrameLayout)
void launch_mesh_part_header(hipStream_t st, const MeshScratch& S, const MeshSlab& B, MeshStreamPartRecord* record, MeshStreamHeader* H, uint32_t max_vertices,
                             uint32_t max_triangles, uint32_t max_tiles) {
  hipLaunchKernelGGL(k_mesh_part_header, dim3(1), dim3(kPartHeaderThreads), 0, st, (const MeshSums*)S.sums + mesh_scan_blocks(S.n_tiles), S.tile_cnt, B, record, H, max_vertices,
                     max_triangles, max_tiles);
}
void launch_mesh_part_emit(hipStream_t st, const Volume& V, const StreamTable& T, const FrameImages& F, const MeshGeometry& G, const MeshScratch& S, const MeshSlab& B,
                           uint32_t flags, const MeshStreamHeader* H, uint32_t* records, void* payload) {
  mesh_packed_instantiation(V, S, flags, [&](auto sparse, auto level, auto vertex_flags) {
    constexpr int kLevel = decltype(level)::value;
    const dim3 g(S.n_tiles), own(B.n_own), b(kMeshThreads);
    const uint32_t stride = flags ? 16u : 8u;
    hipLaunchKernelGGL((k_mesh_part_vertices_packed<decltype(sparse)::value, decltype(vertex_flags)::value, kLevel>), g, b, 0, st, V, T, F, G, B, H, S.tile_cnt, S.tile_vbase,
                       S.tile_rec, records, payload);
    const MeshLattice lat = mesh_lattice(V.res, kLevel);               // the rows: one per OWNED tile, `tile` its id in the WHOLE level's grid
    launch_mesh_stream_table(st, S, H, B.n_own, (uint32_t)(B.layer0 * lat.ntx * lat.nty), payload, stride, nullptr);
    hipLaunchKernelGGL(k_mesh_part_triangles<kLevel>, own, b, 0, st, V, B, H, S.tile_cnt, S.tile_vbase, S.tile_tbase, S.tile_rec, records, (uint8_t*)payload, stride);
  });
}

}  // namespace rr
