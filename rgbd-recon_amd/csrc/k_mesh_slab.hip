// Mesh extraction on a Z-slab context: the slab's part of the whole volume's mesh (tsdf_mesh_slab_extract / _link, include/rgbd_recon_hip.h has the
// definition).  The whole mesh is ordered by lattice tile with the tile layer outermost and slabs are tile aligned, so it is the concatenation of the
// slabs' parts; what k_mesh.hip does per tile is done here per OWNED tile, with the same device text (mesh_dev.hpp), and the scan is k_mesh.hip's.
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
// k_mesh_part_header, k_mesh_part_vertices_packed, k_mesh_part_table and k_mesh_part_triangles below -- the slab's part of the tile-local frame, whose
// corner codes name no vertex of another slab by index, so that nothing of the link is needed.
#include "tsdf_common.hpp"

namespace rr {
// k_mesh.hip's two tables, word for word (a __constant__ array belongs to one code object: this file's kernels need their own).  Private to this file;
// tests/test_gpu_mesh_slab.py compares what they produce with k_mesh.hip's output byte for byte.
static __constant__ uint8_t c_tet[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
static __constant__ uint16_t c_mesh_flip[6] = {0x4d24, 0x32da, 0x32da, 0x4d24, 0x4d24, 0x32da};
}  // namespace rr
#define RR_MESH_TABLES_DEFINED   // (mesh_dev.hpp asks for it: its functions read the two tables)

#include "mesh_dev.hpp"
#include "scan_dev.hpp"

namespace rr {

template <int kLevel>
__device__ __forceinline__ MeshTile mesh_slab_tile(const LatticeOf<kLevel>& L, const MeshSlab& B) {
  MeshTile t;
  t.id = (int)blockIdx.x;
  const int per_layer = L.ntx() * L.nty(), layer = t.id / per_layer, in_layer = t.id - layer * per_layer;
  t.tz = B.layer0 + layer; t.ty = in_layer / L.ntx(); t.tx = in_layer - t.ty * L.ntx();
  return t;
}
// a seam tile's stage: lattice planes 0 and 1 only (nothing beyond them is stored for certain, and nothing beyond them is read by the plane-0 lanes)
template <bool kSparse, int kLevel>
__device__ __forceinline__ void mesh_stage_seam(const Volume& V, const LatticeOf<kLevel>& L, const MeshTile& t, float* s_f) {
  for (int i = threadIdx.x; i < 2 * 81; i += kMeshThreads) {
    const int lx = i % 9, ly = (i / 9) % 9, lz = i / 81;
    const int x = t.tx * 8 + lx, y = t.ty * 8 + ly, z = t.tz * 8 + lz;
    float f = -V.limit;
    if (x < L.cr(0) && y < L.cr(1) && z < L.cr(2)) f = mesh_voxel<kSparse>(V, x << kLevel, y << kLevel, z << kLevel);
    s_f[i] = f;
  }
}
// an owned tile: every lattice point; a seam tile: plane 0 (the other lanes own nothing here)
template <int kLevel>
__device__ __forceinline__ MeshPoint mesh_slab_point(const LatticeOf<kLevel>& L, const MeshTile& t, const float* s_f, bool seam) {
  if (seam && threadIdx.x >= 64) return MeshPoint{0u, 0u, 0u};
  MeshPoint p = mesh_point(L, t, s_f, threadIdx.x);
  if (seam) p.ntri = 0u;
  return p;
}

// ---- count: k_mesh_count per slab-local tile.  The class test walks the stored tiles the lattice tile reads, indexed from the first STORED layer; a
// seam tile reads storage layer (tz << level) only.  tile_skip stays 0 for a seam tile: the slab's statistics count owned tiles.
template <bool kSparse, int kLevel>
__global__ __launch_bounds__(kMeshThreads) void k_mesh_slab_count(Volume V, MeshSlab B, uint2* __restrict__ tile_cnt, uint8_t* __restrict__ tile_skip) {
  __shared__ float s_f[kMeshCorners];
  __shared__ uint32_t s_wave[kMeshWaves];
  const LatticeOf<kLevel> L(V);
  const MeshTile t = mesh_slab_tile(L, B);
  const bool seam = t.id >= B.n_own;
  constexpr uint32_t kN = (1u << kLevel) + 1u;
  int mixed = 0;
  if (threadIdx.x < kN * kN * (seam ? 1u : kN)) {
    const int nx = (t.tx << kLevel) + (int)(threadIdx.x % kN), ny = (t.ty << kLevel) + (int)((threadIdx.x / kN) % kN), nz = (t.tz << kLevel) + (int)(threadIdx.x / (kN * kN));
    if (nx < V.ntx && ny < V.nty && nz < V.tz1) {                       // (nz >= tz0: an owned layer, or the first one above them)
      const uint32_t id = (uint32_t)(((nz - V.tz0) * V.nty + ny) * V.ntx + nx);
      mixed = kSparse ? V.slot[id] != kNoSlot : V.cls[id] != kTileMinus;
    }
  }
  if (!__syncthreads_or(mixed)) {
    if (threadIdx.x == 0) { tile_cnt[t.id] = make_uint2(0u, 0u); tile_skip[t.id] = seam ? 0 : 1; }
    return;
  }
  if (seam) mesh_stage_seam<kSparse, kLevel>(V, L, t, s_f); else mesh_stage<kSparse, kLevel>(V, L, t, s_f);
  __syncthreads();
  const MeshPoint p = mesh_slab_point(L, t, s_f, seam);
  uint32_t total;
  block_exclusive_sum<kMeshWaves>((uint32_t)__popc(p.mask) | (p.ntri << 16), s_wave, &total);
  if (threadIdx.x == 0) { tile_cnt[t.id] = make_uint2(total & 0xffffu, total >> 16); tile_skip[t.id] = 0; }
}

// ---- records and vertices: k_mesh_vertices per slab-local tile; a seam tile leaves its records and emits nothing
template <bool kSparse, int kLevel>
__global__ __launch_bounds__(kMeshThreads) void k_mesh_slab_vertices(Volume V, StreamTable T, FrameImages F, MeshGeometry G, MeshSlab B, const uint2* __restrict__ tile_cnt,
                                                                     const uint32_t* __restrict__ tile_vbase, const uint32_t* __restrict__ tile_rec,
                                                                     uint32_t* __restrict__ records, float* __restrict__ out_pos, float* __restrict__ out_nrm,
                                                                     float4* __restrict__ out_col) {
  __shared__ float s_f[kMeshCorners];
  __shared__ uint32_t s_wave[kMeshWaves];
  __shared__ uint16_t s_edge[kMeshThreads * 7];                        // per vertex of the tile: lattice point << 3 | d
  const LatticeOf<kLevel> L(V);
  const MeshTile t = mesh_slab_tile(L, B);
  const bool seam = t.id >= B.n_own;
  const uint32_t nv = tile_cnt[t.id].x;
  if (nv == 0) return;
  if (seam) mesh_stage_seam<kSparse, kLevel>(V, L, t, s_f); else mesh_stage<kSparse, kLevel>(V, L, t, s_f);
  __syncthreads();
  const MeshPoint p = mesh_slab_point(L, t, s_f, seam);
  uint32_t total;
  const uint32_t off = block_exclusive_sum<kMeshWaves>((uint32_t)__popc(p.mask), s_wave, &total);
  records[(size_t)tile_rec[t.id] * kMeshThreads + threadIdx.x] = p.mask | (p.inside << 7) | (off << 8);
  if (seam) return;                                                    // (its vertices are the slab above's)
  {
    uint32_t k = off;
#pragma unroll
    for (int d = 1; d < 8; ++d)
      if (p.mask & (1u << (d - 1))) s_edge[k++] = (uint16_t)((threadIdx.x << 3) | d);
  }
  __syncthreads();
  mesh_tile_vertices<kSparse, kLevel>(V, T, F, G, t, nv, s_f, s_edge, (size_t)tile_vbase[t.id], out_pos, out_nrm, out_col);
}

// ---- triangles of the owned tiles: k_mesh_triangles' text, the tile of a corner taken relative to the slab's first layer.  Out = uint32_t: global
// indices (the link); Out = uint16_t: the streamed tile-local corner codes (the part ring), which name a corner by its offset inside its owner tile and
// where that tile lies from this one -- nothing of base, slab_vertices and above is read then, a seam tile's records serve as an owned tile's do
template <int kLevel, typename Out>
__device__ __forceinline__ void mesh_slab_tile_triangles(const Volume& V, const MeshSlab& B, const uint2* __restrict__ tile_cnt, const uint32_t* __restrict__ tile_vbase,
                                                         const unsigned long long* __restrict__ tile_tbase, const uint32_t* __restrict__ tile_rec,
                                                         const uint32_t* __restrict__ records, uint32_t base, uint32_t slab_vertices,
                                                         const uint32_t* __restrict__ above, Out* __restrict__ out_tri) {
  constexpr bool kLocal = std::is_same<Out, uint16_t>::value;
  __shared__ uint32_t s_first[kMeshCorners];                           // per corner: the mesh index of the first vertex it owns
  __shared__ uint8_t s_mask[kMeshCorners];                             // ... and its record's low byte (edge mask, inside bit)
  __shared__ uint32_t s_wave[kMeshWaves];
  const LatticeOf<kLevel> L(V);
  const MeshTile t = mesh_slab_tile(L, B);                             // (the launch covers the owned tiles only)
  if (tile_cnt[t.id].y == 0) return;
  for (int i = threadIdx.x; i < kMeshCorners; i += kMeshThreads) {
    const int lx = i % 9, ly = (i / 9) % 9, lz = i / 81;
    const int x = t.tx * 8 + lx, y = t.ty * 8 + ly, z = t.tz * 8 + lz;
    uint32_t first = 0, mask = 0;
    if (x < L.cr(0) && y < L.cr(1) && z < L.cr(2)) {                   // (z inside the lattice and above the owned layers: the slab has a seam layer)
      const int tile = (((z >> 3) - B.layer0) * L.nty() + (y >> 3)) * L.ntx() + (x >> 3);
      const uint32_t slot = tile_rec[tile];
      if (slot != kNoSlot) {                                           // (a tile without surface owns no crossed edge: nothing is looked up in it)
        const uint32_t r = records[(size_t)slot * kMeshThreads + (((z & 7) << 6) | ((y & 7) << 3) | (x & 7))];
        if constexpr (kLocal) first = (r >> 8) | ((uint32_t)((lx >> 3) | ((ly >> 3) << 1) | ((lz >> 3) << 2)) << 12);
        else first = base + (tile < B.n_own ? tile_vbase[tile] : slab_vertices + above[tile - B.n_own]) + (r >> 8);
        mask = r & 0xffu;
      }
    }
    s_first[i] = first; s_mask[i] = (uint8_t)mask;
  }
  __syncthreads();
  const int lx = threadIdx.x & 7, ly = (threadIdx.x >> 3) & 7, lz = threadIdx.x >> 6;
  const int x = t.tx * 8 + lx, y = t.ty * 8 + ly, z = t.tz * 8 + lz;
  // the cell's corner bits from its origin's record: corner b is inside iff the origin is, unless the edge origin -> b is crossed
  uint32_t corners = 0, ntri = 0;
  if (x + 1 < L.cr(0) && y + 1 < L.cr(1) && z + 1 < L.cr(2)) {
    const uint32_t m = s_mask[corner_index(lx, ly, lz)];
    corners = ((m & 0x7fu) << 1) ^ ((m & 0x80u) ? 0xffu : 0u);
    ntri = cell_triangles(corners);
  }
  uint32_t total;
  const uint32_t off = block_exclusive_sum<kMeshWaves>(ntri, s_wave, &total);
  if (ntri == 0) return;
  mesh_cell_triangles(corners, s_first, s_mask, lx, ly, lz, out_tri + (size_t)(tile_tbase[t.id] + off) * 3);
}
template <int kLevel>
__global__ __launch_bounds__(kMeshThreads) void k_mesh_slab_triangles(Volume V, MeshSlab B, const uint2* __restrict__ tile_cnt, const uint32_t* __restrict__ tile_vbase,
                                                                      const unsigned long long* __restrict__ tile_tbase, const uint32_t* __restrict__ tile_rec,
                                                                      const uint32_t* __restrict__ records, uint32_t base, uint32_t slab_vertices,
                                                                      const uint32_t* __restrict__ above, uint32_t* __restrict__ out_tri) {
  mesh_slab_tile_triangles<kLevel>(V, B, tile_cnt, tile_vbase, tile_tbase, tile_rec, records, base, slab_vertices, above, out_tri);
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
  const unsigned long long own_vertices = s.nv - seam_vertices, own_tiles = s.surface - seam_tiles;
  MeshStreamHeader h{};
  h.needed_vertices = own_vertices; h.needed_triangles = s.nt; h.needed_tiles = own_tiles; h.tiles_skipped = s.skipped;   // (a seam tile counts no triangle and no skip)
  h.max_vertices = max_vertices; h.max_triangles = max_triangles; h.max_tiles = max_tiles;
  h.overflow = (own_vertices > max_vertices ? 1u : 0u) | (s.nt > max_triangles ? 2u : 0u) | (own_tiles > max_tiles ? 4u : 0u);
  h.n_vertices = h.overflow ? 0ull : own_vertices; h.n_triangles = h.overflow ? 0ull : s.nt;
  *H = h;
  MeshStreamPartRecord r{};
  r.seam_tiles = seam_tiles; r.seam_vertices = seam_vertices;
  *record = r;
}
// records of every tile with surface, packed vertices of the owned ones: k_mesh_vertices_packed per slab-local tile, the seam tile as in k_mesh_slab_vertices
template <bool kSparse, uint32_t kFlags, int kLevel>
__global__ __launch_bounds__(kMeshThreads, 4) void k_mesh_part_vertices_packed(Volume V, StreamTable T, FrameImages F, MeshGeometry G, MeshSlab B,
                                                                               const MeshStreamHeader* __restrict__ H, const uint2* __restrict__ tile_cnt,
                                                                               const uint32_t* __restrict__ tile_vbase, const uint32_t* __restrict__ tile_rec,
                                                                               uint32_t* __restrict__ records, void* __restrict__ out) {
  __shared__ float s_f[kMeshCorners];
  __shared__ uint32_t s_wave[kMeshWaves];
  __shared__ uint16_t s_edge[kMeshThreads * 7];                        // per vertex of the tile: lattice point << 3 | d
  const LatticeOf<kLevel> L(V);
  const MeshTile t = mesh_slab_tile(L, B);
  const bool seam = t.id >= B.n_own;
  const uint32_t nv = tile_cnt[t.id].x;
  if (mesh_stream_overflow(H) || nv == 0) return;
  if (seam) mesh_stage_seam<kSparse, kLevel>(V, L, t, s_f); else mesh_stage<kSparse, kLevel>(V, L, t, s_f);
  __syncthreads();
  const MeshPoint p = mesh_slab_point(L, t, s_f, seam);
  uint32_t total;
  const uint32_t off = block_exclusive_sum<kMeshWaves>((uint32_t)__popc(p.mask), s_wave, &total);
  records[(size_t)tile_rec[t.id] * kMeshThreads + threadIdx.x] = p.mask | (p.inside << 7) | (off << 8);   // (tile_rec < needed_tiles + seam tiles <= max_tiles + n_seam)
  if (seam) return;                                                    // (its vertices are the part above's)
  {
    uint32_t k = off;
#pragma unroll
    for (int d = 1; d < 8; ++d)
      if (p.mask & (1u << (d - 1))) s_edge[k++] = (uint16_t)((threadIdx.x << 3) | d);
  }
  __syncthreads();
  mesh_tile_vertices_packed<kSparse, kFlags, kLevel>(V, T, F, G, t, nv, s_f, s_edge, (size_t)tile_vbase[t.id], out);   // (owned tiles come first: < needed_vertices <= max_vertices)
}
// the table: one lane per OWNED tile, one 16-byte store at the tile's surface ordinal; `tile` is the id in the WHOLE level's grid, the two bases part-local
__global__ __launch_bounds__(kPartHeaderThreads) void k_mesh_part_table(const MeshStreamHeader* __restrict__ H, const uint2* __restrict__ tile_cnt, const uint32_t* __restrict__ tile_vbase,
                                                                        const unsigned long long* __restrict__ tile_tbase, const uint32_t* __restrict__ tile_rec, int n_own,
                                                                        uint32_t first_tile, uint8_t* __restrict__ payload, uint32_t stride) {
  const int t = (int)(blockIdx.x * kPartHeaderThreads + threadIdx.x);
  if (mesh_stream_overflow(H) || t >= n_own) return;
  const size_t vertex_bytes = (size_t)H->needed_vertices * stride;
  if (t == 0 && (vertex_bytes & 8u)) *(uint2*)(payload + vertex_bytes) = make_uint2(0u, 0u);   // the padding
  const uint2 cnt = tile_cnt[t];
  if (cnt.x)                                                           // (tile_rec < needed_tiles <= max_tiles)
    *(uint4*)(mesh_stream_table(H, payload, stride) + tile_rec[t]) = make_uint4(first_tile + (uint32_t)t, tile_vbase[t], (uint32_t)tile_tbase[t], cnt.y);
}
// ... and the 6-byte triangles behind the rows: exactly the codes of the whole volume's compact frame (a code names no part)
template <int kLevel>
__global__ __launch_bounds__(kMeshThreads) void k_mesh_part_triangles(Volume V, MeshSlab B, const MeshStreamHeader* __restrict__ H, const uint2* __restrict__ tile_cnt,
                                                                      const uint32_t* __restrict__ tile_vbase, const unsigned long long* __restrict__ tile_tbase,
                                                                      const uint32_t* __restrict__ tile_rec, const uint32_t* __restrict__ records,
                                                                      uint8_t* __restrict__ payload, uint32_t stride) {
  if (mesh_stream_overflow(H)) return;
  mesh_slab_tile_triangles<kLevel, uint16_t>(V, B, tile_cnt, tile_vbase, tile_tbase, tile_rec, records, 0u, 0u, nullptr,
                                             (uint16_t*)(mesh_stream_table(H, payload, stride) + H->needed_tiles));
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
  mesh_instantiation(V, S, [&](auto sparse, auto level) {
    constexpr bool kSparse = decltype(sparse)::value;
    constexpr int kLevel = decltype(level)::value;
    const dim3 g(S.n_tiles), own(B.n_own), b(kMeshThreads);
    const uint32_t stride = flags ? 16u : 8u;
    switch (flags & 3u) {
      case 0u: hipLaunchKernelGGL((k_mesh_part_vertices_packed<kSparse, 0u, kLevel>), g, b, 0, st, V, T, F, G, B, H, S.tile_cnt, S.tile_vbase, S.tile_rec, records, payload); break;
      case 1u: hipLaunchKernelGGL((k_mesh_part_vertices_packed<kSparse, 1u, kLevel>), g, b, 0, st, V, T, F, G, B, H, S.tile_cnt, S.tile_vbase, S.tile_rec, records, payload); break;
      case 2u: hipLaunchKernelGGL((k_mesh_part_vertices_packed<kSparse, 2u, kLevel>), g, b, 0, st, V, T, F, G, B, H, S.tile_cnt, S.tile_vbase, S.tile_rec, records, payload); break;
      default: hipLaunchKernelGGL((k_mesh_part_vertices_packed<kSparse, 3u, kLevel>), g, b, 0, st, V, T, F, G, B, H, S.tile_cnt, S.tile_vbase, S.tile_rec, records, payload); break;
    }
    const MeshLattice lat = mesh_lattice(V.res, kLevel);
    hipLaunchKernelGGL(k_mesh_part_table, dim3((B.n_own + kPartHeaderThreads - 1) / kPartHeaderThreads), dim3(kPartHeaderThreads), 0, st, H, S.tile_cnt, S.tile_vbase, S.tile_tbase,
                       S.tile_rec, B.n_own, (uint32_t)(B.layer0 * lat.ntx * lat.nty), (uint8_t*)payload, stride);
    hipLaunchKernelGGL(k_mesh_part_triangles<kLevel>, own, b, 0, st, V, B, H, S.tile_cnt, S.tile_vbase, S.tile_tbase, S.tile_rec, records, (uint8_t*)payload, stride);
  });
}

}  // namespace rr
