// The device text of the mesh extraction: every stage's body once -- count, records, vertices, triangles, the streamed header -- for k_mesh.hip (a whole
// volume) and k_mesh_slab.hip (a Z-slab's part), whose kernels are wrappers that name a tile policy (WholeTiles / SlabTiles below).  All of it speaks of a
// tile through MeshTile: (tx, ty, tz) is the tile in the WHOLE volume's lattice, id its index in the caller's per-tile arrays.
// The two tables are NOT here: a __constant__ array belongs to one code object, so the file that includes this header defines c_tet and c_mesh_flip
// in namespace rr first and says so with RR_MESH_TABLES_DEFINED (an `extern` declaration here cannot stand in for that: k_mesh_slab.hip's copy has
// internal linkage, and two external definitions of one name would collide in the library's host symbols).  k_mesh.hip holds the definition
// (tests/test_mesh_reference.py compares its words with the generated ones), with external linkage as it always had -- a table private to the translation unit is folded into k_mesh_triangles' code and costs that kernel 7 VGPRs.
#pragma once
#ifndef RR_MESH_TABLES_DEFINED
#error "define rr::c_tet[6][4] and rr::c_mesh_flip[6] (__constant__), then RR_MESH_TABLES_DEFINED, before including mesh_dev.hpp"
#endif
#include <cfloat>
#include <type_traits>

#include "blend_dev.hpp"
#include "scan_dev.hpp"

namespace rr {

constexpr int kMeshThreads = 512;            // one lane per lattice point of a tile
constexpr int kMeshWaves = kMeshThreads / 64;
constexpr int kMeshCorners = 9 * 9 * 9;      // a tile's lattice points and their +x/+y/+z neighbours

// f(sparse, level), both as compile-time constants: the one place that turns the volume's storage and the scratch's level into template arguments
template <typename F>
static void mesh_instantiation(const Volume& V, const MeshScratch& S, F&& f) {
  auto at = [&](auto sparse) {
    switch (S.level) {
      case 0: f(sparse, std::integral_constant<int, 0>{}); break;
      case 1: f(sparse, std::integral_constant<int, 1>{}); break;
      default: f(sparse, std::integral_constant<int, 2>{}); break;
    }
  };
  if (V.slot) at(std::true_type{}); else at(std::false_type{});
}
// f(sparse, level, vertex flags): the packed-vertex kernels' instantiation (flags: 1 normals, 2 colours)
template <typename F>
static void mesh_packed_instantiation(const Volume& V, const MeshScratch& S, uint32_t flags, F&& f) {
  mesh_instantiation(V, S, [&](auto sparse, auto level) {
    switch (flags & 3u) {
      case 0u: f(sparse, level, std::integral_constant<uint32_t, 0u>{}); break;
      case 1u: f(sparse, level, std::integral_constant<uint32_t, 1u>{}); break;
      case 2u: f(sparse, level, std::integral_constant<uint32_t, 2u>{}); break;
      default: f(sparse, level, std::integral_constant<uint32_t, 3u>{}); break;
    }
  });
}

// a voxel as the mesh reads it: NaN and +-inf read as -limit (NaN voxels exist, tsdf_integration.vs:52)
__device__ __forceinline__ float mesh_value(float f, float limit) { return fabsf(f) <= FLT_MAX ? f : -limit; }

struct MeshTile { int tx, ty, tz, id; };
// The lattice inside a kernel.  A level holds the MeshLattice of the volume's resolution (tsdf_common.hpp: the one definition, the host sizes the launch
// by it).  Level 0 is the voxel grid and its storage tiles and reads the volume's own fields where they are used: the kernels' text before there were
// levels (a copy made at the kernel's head costs k_mesh_triangles a scalar register and another block layout).
template <int kLevel>
struct LatticeOf {
  MeshLattice g;
  __device__ __forceinline__ explicit LatticeOf(const Volume& V) : g(mesh_lattice(V.res, kLevel)) {}
  __device__ __forceinline__ int cr(int a) const { return g.cr[a]; }
  __device__ __forceinline__ int ntx() const { return g.ntx; }
  __device__ __forceinline__ int nty() const { return g.nty; }
};
template <>
struct LatticeOf<0> {
  const Volume& V;
  __device__ __forceinline__ explicit LatticeOf(const Volume& v) : V(v) {}
  __device__ __forceinline__ int cr(int a) const { return V.res[a]; }
  __device__ __forceinline__ int ntx() const { return V.ntx; }
  __device__ __forceinline__ int nty() const { return V.nty; }
};
__device__ __forceinline__ int corner_index(int lx, int ly, int lz) { return (lz * 9 + ly) * 9 + lx; }

// The tile policy: which tiles a launch's workgroups are.  WholeTiles: workgroup b is lattice tile b of the whole volume, stored from layer 0 on -- an
// empty type of constants, so that a whole-volume kernel takes no MeshSlab, reads no V.tz0 and holds no seam branch.  SlabTiles: workgroup b is
// slab-local tile b of the slab B (k_mesh_slab.hip's head: the owned layers from B.layer0 on, then the seam layer), stored from layer V.tz0 on.
struct WholeTiles {
  static constexpr bool kSlab = false;
  __device__ __forceinline__ int layer0() const { return 0; }
  __device__ __forceinline__ bool seam(int) const { return false; }
  __device__ __forceinline__ int first_stored_layer(const Volume&) const { return 0; }
};
struct SlabTiles {
  static constexpr bool kSlab = true;
  const MeshSlab& B;
  __device__ __forceinline__ int layer0() const { return B.layer0; }
  __device__ __forceinline__ bool seam(int id) const { return id >= B.n_own; }
  __device__ __forceinline__ int first_stored_layer(const Volume& V) const { return V.tz0; }
};
// a slab's link (tsdf_mesh_slab_link): where the part's vertices begin in the whole mesh, how many it has, and the first vertex of each tile of the slab above
struct MeshSlabLink { uint32_t base, slab_vertices; const uint32_t* __restrict__ above; };
// the tile of this workgroup
template <int kLevel, typename Tiles>
__device__ __forceinline__ MeshTile mesh_tile(const LatticeOf<kLevel>& L, const Tiles& tiles) {
  MeshTile t;
  t.id = (int)blockIdx.x;
  const int per_layer = L.ntx() * L.nty(), layer = t.id / per_layer, in_layer = t.id - layer * per_layer;
  t.tz = tiles.layer0() + layer; t.ty = in_layer / L.ntx(); t.tx = in_layer - t.ty * L.ntx();
  return t;
}

// one voxel, sanitised; (x, y, z) inside the grid
template <bool kSparse>
__device__ __forceinline__ float mesh_voxel(const Volume& V, int x, int y, int z) {
  return mesh_value(kSparse ? tsdf_tap_sparse(V, x, y, z) : V.data[vol_index(V, x, y, z)], V.limit);
}
// the tile's 9 x 9 x 9 corner values -> LDS; a corner outside the lattice reads -limit (no edge and no cell reaches it: see mesh_point).  Lattice point
// (x, y, z) is voxel (x, y, z) << level: a point sample (the last lattice point times the stride is below the resolution, cr = ceil(res / stride)).
// kCorners: the stage's first corners only (mesh_stage_tile)
template <bool kSparse, int kLevel, int kCorners = kMeshCorners>
__device__ __forceinline__ void mesh_stage(const Volume& V, const LatticeOf<kLevel>& L, const MeshTile& t, float* s_f) {
  for (int i = threadIdx.x; i < kCorners; i += kMeshThreads) {
    const int lx = i % 9, ly = (i / 9) % 9, lz = i / 81;
    const int x = t.tx * 8 + lx, y = t.ty * 8 + ly, z = t.tz * 8 + lz;
    float f = -V.limit;
    if (x < L.cr(0) && y < L.cr(1) && z < L.cr(2)) f = mesh_voxel<kSparse>(V, x << kLevel, y << kLevel, z << kLevel);
    s_f[i] = f;
  }
}
// ... of an owned tile, or of a seam tile: lattice planes 0 and 1 only (nothing beyond them is stored for certain, and nothing beyond them is read by
// the plane-0 lanes)
template <bool kSparse, int kLevel>
__device__ __forceinline__ void mesh_stage_tile(const Volume& V, const LatticeOf<kLevel>& L, const MeshTile& t, float* s_f, bool seam) {
  if (seam) mesh_stage<kSparse, kLevel, 2 * 81>(V, L, t, s_f); else mesh_stage<kSparse, kLevel>(V, L, t, s_f);
}
// Descent of a crossed lattice edge P -> P + (d << level) to the voxel edge that carries its vertex: bisection, the end on the midpoint's side of the
// surface moves to the midpoint (a midpoint is a voxel read, never the LDS stage: it is no lattice point).  In: (x, y, z) = P as a voxel, a = f(P),
// b = f(other end).  Out: neighbouring voxels (x, y, z), (x, y, z) + d with their values, exactly one of them inside, as on entry.
template <bool kSparse, int kLevel>
__device__ __forceinline__ void mesh_descend(const Volume& V, int bx, int by, int bz, int& x, int& y, int& z, float& a, float& b) {
  const bool inside = a > 0.0f;
#pragma unroll
  for (int h = (1 << kLevel) >> 1; h >= 1; h >>= 1) {
    const int mx = x + h * bx, my = y + h * by, mz = z + h * bz;
    const float m = mesh_voxel<kSparse>(V, mx, my, mz);
    if ((m > 0.0f) == inside) { a = m; x = mx; y = my; z = mz; } else b = m;
  }
}

// What lattice point `lane` of the tile owns: its edge mask (bit d - 1: the edge p -> p + d lies inside the lattice and exactly one
// of its ends is inside the surface), whether p itself is inside, and the triangles of the cell whose origin it is.
struct MeshPoint { uint32_t mask, inside, ntri; };
__device__ __forceinline__ uint32_t tet_triangles(uint32_t corners, int k) {   // corners: bit b = corner b is inside
  const uint32_t n = ((corners >> c_tet[k][0]) & 1u) + ((corners >> c_tet[k][1]) & 1u) + ((corners >> c_tet[k][2]) & 1u) + ((corners >> c_tet[k][3]) & 1u);
  return n == 2u ? 2u : ((n == 1u || n == 3u) ? 1u : 0u);
}
__device__ __forceinline__ uint32_t cell_triangles(uint32_t corners) {
  uint32_t n = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) n += tet_triangles(corners, k);
  return n;
}
template <int kLevel>
__device__ __forceinline__ MeshPoint mesh_point(const LatticeOf<kLevel>& L, const MeshTile& t, const float* s_f, int lane) {
  const int lx = lane & 7, ly = (lane >> 3) & 7, lz = lane >> 6;
  const int x = t.tx * 8 + lx, y = t.ty * 8 + ly, z = t.tz * 8 + lz;
  MeshPoint p{0u, 0u, 0u};
  if (x >= L.cr(0) || y >= L.cr(1) || z >= L.cr(2)) return p;
  p.inside = s_f[corner_index(lx, ly, lz)] > 0.0f ? 1u : 0u;          // the raymarch's hit test, tsdf_raymarch.fs:96: zero and -0 are outside
  uint32_t corners = p.inside;
#pragma unroll
  for (int d = 1; d < 8; ++d) {
    const int bx = d & 1, by = (d >> 1) & 1, bz = d >> 2;
    if (x + bx < L.cr(0) && y + by < L.cr(1) && z + bz < L.cr(2)) {
      const uint32_t in = s_f[corner_index(lx + bx, ly + by, lz + bz)] > 0.0f ? 1u : 0u;
      corners |= in << d;
      if (in != p.inside) p.mask |= 1u << (d - 1);
    }
  }
  if (x + 1 < L.cr(0) && y + 1 < L.cr(1) && z + 1 < L.cr(2)) p.ntri = cell_triangles(corners);
  return p;
}
// ... what this lane owns: in an owned tile its lattice point, in a seam tile the plane-0 lanes theirs, without the cell (the other lanes own nothing there)
template <int kLevel>
__device__ __forceinline__ MeshPoint mesh_tile_point(const LatticeOf<kLevel>& L, const MeshTile& t, const float* s_f, bool seam) {
  if (seam && threadIdx.x >= 64) return MeshPoint{0u, 0u, 0u};
  MeshPoint p = mesh_point(L, t, s_f, threadIdx.x);
  if (seam) p.ntri = 0u;
  return p;
}

// ---- 1. count: a tile's vertices and triangles.  The class test walks the stored tiles the lattice tile reads, indexed from the first STORED layer; a
// seam tile reads storage layer (tz << level) only, and its tile_skip stays 0: a slab's statistics count owned tiles.
template <bool kSparse, int kLevel, typename Tiles>
__device__ __forceinline__ void mesh_tile_count(const Volume& V, const Tiles& tiles, uint2* __restrict__ tile_cnt, uint8_t* __restrict__ tile_skip) {
  __shared__ float s_f[kMeshCorners];
  __shared__ uint32_t s_wave[kMeshWaves];
  const LatticeOf<kLevel> L(V);
  const MeshTile t = mesh_tile(L, tiles);
  const bool seam = tiles.seam(t.id);
  // the tile and its seven +x/+y/+z neighbours hold the clear value only (-limit: outside): no edge of this tile can cross the surface.  At a level the
  // lattice tile's corners and the midpoints of its edges lie in storage tiles [t << level, (t << level) + (1 << level)] per axis: 27 / 125 lanes
  constexpr uint32_t kN = (1u << kLevel) + 1u;
  int mixed = 0;
  if (threadIdx.x < kN * kN * (seam ? 1u : kN)) {
    const int nx = (t.tx << kLevel) + (int)(threadIdx.x % kN), ny = (t.ty << kLevel) + (int)((threadIdx.x / kN) % kN), nz = (t.tz << kLevel) + (int)(threadIdx.x / (kN * kN));
    if (nx < V.ntx && ny < V.nty && nz < V.tz1) {                       // (a slab: nz >= tz0, an owned layer or the first one above them)
      const uint32_t id = (uint32_t)(((nz - tiles.first_stored_layer(V)) * V.nty + ny) * V.ntx + nx);
      mixed = kSparse ? V.slot[id] != kNoSlot : V.cls[id] != kTileMinus;
    }
  }
  if (!__syncthreads_or(mixed)) {
    if (threadIdx.x == 0) { tile_cnt[t.id] = make_uint2(0u, 0u); tile_skip[t.id] = seam ? 0 : 1; }
    return;
  }
  mesh_stage_tile<kSparse, kLevel>(V, L, t, s_f, seam);
  __syncthreads();
  const MeshPoint p = mesh_tile_point(L, t, s_f, seam);
  uint32_t total;
  block_exclusive_sum<kMeshWaves>((uint32_t)__popc(p.mask) | (p.ntri << 16), s_wave, &total);   // both counts in one word: at most 3584 and 6144 per tile
  if (threadIdx.x == 0) { tile_cnt[t.id] = make_uint2(total & 0xffffu, total >> 16); tile_skip[t.id] = 0; }
}

// ---- 2. records and vertices.  What the four vertex kernels stage in LDS, and what they all begin with: the record of every lattice point of the tile
// (bits 0..6 edge mask, bit 7 inside, bits 8.. the offset of its first vertex inside the tile) into the tile's record slot, and per vertex of the tile
// its lattice point << 3 | d in s.edge, in the defined order.  False: a seam tile, which leaves its records and emits nothing (its vertices are the
// slab above's).  The caller has found the tile to have a vertex (and, streamed, read the header: tile_rec < needed tiles <= the record slots).
struct MeshVertexStage {                                               // (the order and the 16-byte alignment the compiler gives three __shared__ arrays of their own)
  alignas(16) uint16_t edge[kMeshThreads * 7];                         // per vertex of the tile: lattice point << 3 | d
  alignas(16) float f[kMeshCorners];                                   // the tile's corner stage
  alignas(16) uint32_t wave[kMeshWaves];
};
template <bool kSparse, int kLevel, typename Tiles>
__device__ __forceinline__ bool mesh_tile_records(const Volume& V, const LatticeOf<kLevel>& L, const Tiles& tiles, const MeshTile& t, const uint32_t* __restrict__ tile_rec,
                                                  uint32_t* __restrict__ records, MeshVertexStage& s) {
  const bool seam = tiles.seam(t.id);
  mesh_stage_tile<kSparse, kLevel>(V, L, t, s.f, seam);
  __syncthreads();
  const MeshPoint p = mesh_tile_point(L, t, s.f, seam);
  uint32_t total;
  const uint32_t off = block_exclusive_sum<kMeshWaves>((uint32_t)__popc(p.mask), s.wave, &total);
  records[(size_t)tile_rec[t.id] * kMeshThreads + threadIdx.x] = p.mask | (p.inside << 7) | (off << 8);
  if (seam) return false;
  {
    uint32_t k = off;
#pragma unroll
    for (int d = 1; d < 8; ++d)
      if (p.mask & (1u << (d - 1))) s.edge[k++] = (uint16_t)((threadIdx.x << 3) | d);
  }
  __syncthreads();
  return true;
}
// the unit-cube position of the vertex e = lattice point << 3 | d of the tile
template <bool kSparse, int kLevel>
__device__ __forceinline__ float3 mesh_vertex_position(const Volume& V, const MeshTile& t, const float* s_f, int e) {
  const int lane = e >> 3, d = e & 7;
  const int lx = lane & 7, ly = (lane >> 3) & 7, lz = lane >> 6;
  const int bx = d & 1, by = (d >> 1) & 1, bz = d >> 2;
  float a = s_f[corner_index(lx, ly, lz)], b = s_f[corner_index(lx + bx, ly + by, lz + bz)];
  float w;
  int x, y, z;
  if constexpr (kLevel == 0) {
    w = a / (a - b);
    x = t.tx * 8 + lx; y = t.ty * 8 + ly; z = t.tz * 8 + lz;
  } else {                                                             // the voxel edge of the vertex: every level's vertex is a level-0 vertex
    x = (t.tx * 8 + lx) << kLevel; y = (t.ty * 8 + ly) << kLevel; z = (t.tz * 8 + lz) << kLevel;
    mesh_descend<kSparse, kLevel>(V, bx, by, bz, x, y, z, a, b);
    w = a / (a - b);
  }
  const float upx = ((float)x + 0.5f) / (float)V.res[0], uqx = ((float)(x + bx) + 0.5f) / (float)V.res[0];
  const float upy = ((float)y + 0.5f) / (float)V.res[1], uqy = ((float)(y + by) + 0.5f) / (float)V.res[1];
  const float upz = ((float)z + 0.5f) / (float)V.res[2], uqz = ((float)(z + bz) + 0.5f) / (float)V.res[2];
  return make_float3(upx + w * (uqx - upx), upy + w * (uqy - upy), upz + w * (uqz - upz));
}
// The tile's nv vertices, one lane per vertex, into the arrays from `first` on: s_f the tile's corner stage, s_edge per vertex of the tile its
// lattice point << 3 | d (in the defined order).  out_nrm / out_col may be null.
template <bool kSparse, int kLevel>
__device__ __forceinline__ void mesh_tile_vertices(const Volume& V, const StreamTable& T, const FrameImages& F, const MeshGeometry& G, const MeshTile& t, uint32_t nv,
                                                   const float* s_f, const uint16_t* s_edge, size_t first, float* __restrict__ out_pos, float* __restrict__ out_nrm,
                                                   float4* __restrict__ out_col) {
  const float ex = G.bbox_max[0] - G.bbox_min[0], ey = G.bbox_max[1] - G.bbox_min[1], ez = G.bbox_max[2] - G.bbox_min[2];
  const float limit = V.limit, sd = limit * 0.5f;
  for (uint32_t v = threadIdx.x; v < nv; v += kMeshThreads) {
    const float3 u = mesh_vertex_position<kSparse, kLevel>(V, t, s_f, s_edge[v]);
    const size_t o = first + v;
    const float3 w = vol_to_world(G.bbox_min, u, ex, ey, ez);
    out_pos[o * 3 + 0] = w.x; out_pos[o * 3 + 1] = w.y; out_pos[o * 3 + 2] = w.z;
    if (out_nrm) {
      const float3 n = world_normal(tsdf_gradient<kSparse>(V, u, sd), ex, ey, ez);
      out_nrm[o * 3 + 0] = n.x; out_nrm[o * 3 + 1] = n.y; out_nrm[o * 3 + 2] = n.z;
    }
    if (out_col) out_col[o] = blend_colors(T, F, limit, u);           // all four components: alpha +1 valid, -1 fallback
  }
}

// ---- the streamed form (tsdf_mesh_stream): what the emit kernels of a whole volume (k_mesh.hip) and of a slab's part (k_mesh_slab.hip) share.
// H is the frame's header in device memory: when a need exceeds its capacity every workgroup of the emit kernels returns before it reads anything else,
// so nothing is ever written past a capacity.
struct MeshSums { unsigned long long nv, nt, surface, skipped; };      // the scan's four quantities (k_mesh.hip: launch_mesh_scan); S.sums[blocks] the totals
__device__ __forceinline__ bool mesh_stream_overflow(const MeshStreamHeader* __restrict__ H) {
  return H->needed_vertices > H->max_vertices || H->needed_triangles > H->max_triangles || H->needed_tiles > H->max_tiles;
}
// a frame's header from what the frame needs (the scan's totals; a slab's part: without its seam tiles) and the ring's capacities
__device__ __forceinline__ MeshStreamHeader mesh_stream_header(unsigned long long nv, unsigned long long nt, unsigned long long surface, unsigned long long skipped,
                                                               uint32_t max_vertices, uint32_t max_triangles, uint32_t max_tiles) {
  MeshStreamHeader h{};
  h.needed_vertices = nv; h.needed_triangles = nt; h.needed_tiles = surface; h.tiles_skipped = skipped;
  h.max_vertices = max_vertices; h.max_triangles = max_triangles; h.max_tiles = max_tiles;
  h.overflow = (nv > max_vertices ? 1u : 0u) | (nt > max_triangles ? 2u : 0u) | (surface > max_tiles ? 4u : 0u);
  h.n_vertices = h.overflow ? 0ull : nv; h.n_triangles = h.overflow ? 0ull : nt;
  return h;
}
// the tile-local format's row area: behind the vertices and their zero padding, at a multiple of 16 bytes
__device__ __forceinline__ MeshTileRow* mesh_stream_table(const MeshStreamHeader* __restrict__ H, uint8_t* __restrict__ payload, uint32_t stride) {
  return (MeshTileRow*)(payload + (((size_t)H->needed_vertices * stride + 15u) & ~(size_t)15u));
}
__device__ __forceinline__ uint32_t unorm16(float u) { return (uint32_t)__float2int_rn(fminf(fmaxf(u, 0.0f), 1.0f) * 65535.0f); }
__device__ __forceinline__ uint32_t snorm16(float p) { return (uint32_t)__float2int_rn(fminf(fmaxf(p, -1.0f), 1.0f) * 32767.0f) & 0xffffu; }
// tsdf_present's RGBA8 rule (k_present.hip: unorm8): the clamp maps NaN to 0
__device__ __forceinline__ uint32_t mesh_unorm8(float v) { return (uint32_t)__float2int_rn(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f); }
// octahedral code of a unit normal, two int16; a NaN component: (-32768, -32768)
__device__ __forceinline__ uint32_t mesh_oct_normal(float3 n) {
  if (n.x != n.x || n.y != n.y || n.z != n.z) return 0x80008000u;
  const float s = (fabsf(n.x) + fabsf(n.y)) + fabsf(n.z);
  float px = n.x / s, py = n.y / s;
  if (n.z < 0.0f) {
    const float fx = (1.0f - fabsf(py)) * (px >= 0.0f ? 1.0f : -1.0f), fy = (1.0f - fabsf(px)) * (py >= 0.0f ? 1.0f : -1.0f);
    px = fx; py = fy;
  }
  return snorm16(px) | (snorm16(py) << 16);
}
// The tile's nv vertices, packed: the same vertex as mesh_tile_vertices', quantised in registers and written with ONE 8- or 16-byte store -- no fp32
// position, normal or colour exists in memory.  `first`: the tile's first vertex in `out` (first + nv <= needed_vertices <= max_vertices: the caller has
// read the header).
template <bool kSparse, uint32_t kFlags, int kLevel>
__device__ __forceinline__ void mesh_tile_vertices_packed(const Volume& V, const StreamTable& T, const FrameImages& F, const MeshGeometry& G, const MeshTile& t, uint32_t nv,
                                                          const float* s_f, const uint16_t* s_edge, size_t first, void* __restrict__ out) {
  const float ex = G.bbox_max[0] - G.bbox_min[0], ey = G.bbox_max[1] - G.bbox_min[1], ez = G.bbox_max[2] - G.bbox_min[2];
  const float limit = V.limit, sd = limit * 0.5f;
  for (uint32_t v = threadIdx.x; v < nv; v += kMeshThreads) {
    const float3 u = mesh_vertex_position<kSparse, kLevel>(V, t, s_f, s_edge[v]);
    const size_t o = first + v;
    const uint2 pos = make_uint2(unorm16(u.x) | (unorm16(u.y) << 16), unorm16(u.z));
    if (kFlags == 0u) { ((uint2*)out)[o] = pos; continue; }
    uint32_t nrm = 0u, col = 0u;
    if (kFlags & 1u) {
      nrm = mesh_oct_normal(world_normal(tsdf_gradient<kSparse>(V, u, sd), ex, ey, ez));
    }
    if (kFlags & 2u) {
      const float4 c = blend_colors(T, F, limit, u);
      col = mesh_unorm8(c.x) | (mesh_unorm8(c.y) << 8) | (mesh_unorm8(c.z) << 16) | (mesh_unorm8(c.w) << 24);
    }
    ((uint4*)out)[o] = make_uint4(pos.x, pos.y, nrm, col);
  }
}

// the mesh index of the vertex on the edge between corners x < y of the cell at (lx, ly, lz): s_first / s_mask hold, per corner of the tile, the index
// of the first vertex it owns and its record's low byte
__device__ __forceinline__ uint32_t edge_vertex(const uint32_t* s_first, const uint8_t* s_mask, int lx, int ly, int lz, int x, int y) {
  const int i = corner_index(lx + (x & 1), ly + ((x >> 1) & 1), lz + (x >> 2)), d = y - x;
  return s_first[i] + (uint32_t)__popc((uint32_t)s_mask[i] & ((1u << (d - 1)) - 1u));
}
// the triangles of the cell at (lx, ly, lz) with the corner bits `corners`, written from o on in (tetrahedron, triangle) order.  Out: uint32_t, or
// uint16_t for the streamed tile-local codes (s_first then holds, per corner, the offset inside the owner tile with the neighbour code from bit 12 up:
// offset + rank stays below 3584, so the sum never reaches the code)
template <typename Out>
__device__ __forceinline__ void mesh_cell_triangles(uint32_t corners, const uint32_t* s_first, const uint8_t* s_mask, int lx, int ly, int lz, Out* __restrict__ o) {
  for (int k = 0; k < 6; ++k) {
    const int v[4] = {c_tet[k][0], c_tet[k][1], c_tet[k][2], c_tet[k][3]};
    uint32_t cs = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) cs |= ((corners >> v[j]) & 1u) << j;
    if (cs == 0u || cs == 15u) continue;
    const bool flip = (c_mesh_flip[k] >> cs) & 1u;
    const int n_in = __popc(cs);
    if (n_in != 2) {                                                   // one vertex apart from the other three: one triangle over its three edges, in vertex order
      const uint32_t lone = n_in == 1 ? cs : (cs ^ 15u);
      const int a = __ffs((int)lone) - 1;
      uint32_t e[3]; int n = 0;
      for (int j = 0; j < 4; ++j)
        if (j != a) { e[n++] = edge_vertex(s_first, s_mask, lx, ly, lz, min(v[a], v[j]), max(v[a], v[j])); }
      o[0] = (Out)e[0]; o[1] = (Out)(flip ? e[2] : e[1]); o[2] = (Out)(flip ? e[1] : e[2]);
      o += 3;
    } else {                                                           // inside A before B, outside C before D: the quad AC, AD, BD, BC as (AC, AD, BD), (AC, BD, BC)
      int in[2], out[2], ni = 0, no = 0;
      for (int j = 0; j < 4; ++j) { if ((cs >> j) & 1u) in[ni++] = v[j]; else out[no++] = v[j]; }
      const uint32_t ac = edge_vertex(s_first, s_mask, lx, ly, lz, min(in[0], out[0]), max(in[0], out[0]));
      const uint32_t ad = edge_vertex(s_first, s_mask, lx, ly, lz, min(in[0], out[1]), max(in[0], out[1]));
      const uint32_t bd = edge_vertex(s_first, s_mask, lx, ly, lz, min(in[1], out[1]), max(in[1], out[1]));
      const uint32_t bc = edge_vertex(s_first, s_mask, lx, ly, lz, min(in[1], out[0]), max(in[1], out[0]));
      o[0] = (Out)ac; o[1] = (Out)(flip ? bd : ad); o[2] = (Out)(flip ? ad : bd);
      o[3] = (Out)ac; o[4] = (Out)(flip ? bc : bd); o[5] = (Out)(flip ? bd : bc);
      o += 6;
    }
  }
}

#ifndef RR_MESH_COMPACT_LDS
#define RR_MESH_COMPACT_LDS 0                                          // 1: the measured alternative of the 6-byte rows' stores (below; DESIGN.md has both)
#endif
// ---- 3. a tile's triangles, from the records alone (never the volume); a slab's launch covers its owned tiles only.  Out = uint32_t: mesh indices -- of
// a whole volume tile_vbase[tile of the corner] + its offset, of a slab's part (the link) base + tile_vbase[tile] for an owned tile and
// base + slab_vertices + above[tile] for a seam tile, the slab above following directly in the concatenation.  Out = uint16_t: the streamed tile-local
// corner codes (bits 0..11 the vertex's offset inside its owner tile, bits 12..14 where that tile lies from this one: a corner whose local coordinate is 8
// belongs to the +x / +y / +z neighbour), which name no vertex by index -- nothing of tile_vbase and the link is read, a seam tile's records serve as an
// owned tile's do.
template <int kLevel, typename Out, typename Tiles>
__device__ __forceinline__ void mesh_tile_triangles(const Volume& V, const Tiles& tiles, const uint2* __restrict__ tile_cnt, const uint32_t* __restrict__ tile_vbase,
                                                    const unsigned long long* __restrict__ tile_tbase, const uint32_t* __restrict__ tile_rec,
                                                    const uint32_t* __restrict__ records, const MeshSlabLink& link, Out* __restrict__ out_tri) {
  constexpr bool kLocal = std::is_same<Out, uint16_t>::value;
  __shared__ uint32_t s_first[kMeshCorners];                           // per corner: the mesh index of the first vertex it owns
  __shared__ uint8_t s_mask[kMeshCorners];                             // ... and its record's low byte (edge mask, inside bit)
  __shared__ uint32_t s_wave[kMeshWaves];
  const LatticeOf<kLevel> L(V);
  const MeshTile t = mesh_tile(L, tiles);
  if (tile_cnt[t.id].y == 0) return;
  for (int i = threadIdx.x; i < kMeshCorners; i += kMeshThreads) {
    const int lx = i % 9, ly = (i / 9) % 9, lz = i / 81;
    const int x = t.tx * 8 + lx, y = t.ty * 8 + ly, z = t.tz * 8 + lz;
    uint32_t first = 0, mask = 0;
    if (x < L.cr(0) && y < L.cr(1) && z < L.cr(2)) {                   // (a slab: z inside the lattice and above the owned layers means it has a seam layer)
      const int tile = (((z >> 3) - tiles.layer0()) * L.nty() + (y >> 3)) * L.ntx() + (x >> 3);
      const uint32_t slot = tile_rec[tile];
      if (slot != kNoSlot) {                                           // (a tile without surface owns no crossed edge: nothing is looked up in it)
        const uint32_t r = records[(size_t)slot * kMeshThreads + (((z & 7) << 6) | ((y & 7) << 3) | (x & 7))];
        if constexpr (kLocal) first = (r >> 8) | ((uint32_t)((lx >> 3) | ((ly >> 3) << 1) | ((lz >> 3) << 2)) << 12);
        else if constexpr (Tiles::kSlab) first = link.base + (!tiles.seam(tile) ? tile_vbase[tile] : link.slab_vertices + link.above[tile - tiles.B.n_own]) + (r >> 8);
        else first = tile_vbase[tile] + (r >> 8);
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
  if constexpr (kLocal && !Tiles::kSlab && RR_MESH_COMPACT_LDS) {
    // The alternative: a tile's rows are contiguous, so they are staged in LDS at the destination's offset inside its 16-byte line and leave as
    // aligned 16-byte stores, the ragged head and tail as shorts.
    __shared__ __attribute__((aligned(16))) uint16_t s_rows[kMeshThreads * 12 * 3 + 8];
    Out* __restrict__ g = out_tri + (size_t)tile_tbase[t.id] * 3;
    const uint32_t shift = (uint32_t)(((size_t)g & 15u) >> 1), n16 = total * 3u;
    if (ntri) mesh_cell_triangles(corners, s_first, s_mask, lx, ly, lz, s_rows + shift + off * 3u);
    __syncthreads();
    const uint32_t head = min(n16, (8u - shift) & 7u), body = (n16 - head) >> 3, tail = head + (body << 3);
    for (uint32_t i = threadIdx.x; i < head; i += kMeshThreads) g[i] = s_rows[shift + i];
    for (uint32_t i = threadIdx.x; i < body; i += kMeshThreads) ((uint4*)(g + head))[i] = ((const uint4*)(s_rows + shift + head))[i];
    for (uint32_t i = tail + threadIdx.x; i < n16; i += kMeshThreads) g[i] = s_rows[shift + i];
  } else {
    if (ntri == 0) return;
    mesh_cell_triangles(corners, s_first, s_mask, lx, ly, lz, out_tri + (size_t)(tile_tbase[t.id] + off) * 3);
  }
}

}  // namespace rr
