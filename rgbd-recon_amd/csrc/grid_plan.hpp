// The grid set-up's arithmetic: what a context's geometry comes to before anything is allocated -- the voxel grid of a box, the ViewLod atlas of a
// view size, the brick grid with its voxel <-> brick <-> tile tables, the tile layers of a Z-slab, the LUT texel box of a volume's tiles.  Host only, free
// of HIP: values in, plain structs out, no context, no device pointer, no environment.  Every plan carries an error class instead of a message: abi.cpp
// plans first, refuses (with its message) while the context is untouched, and only then releases, allocates, uploads and binds.  fp32 throughout where the
// reference computes in fp32: every rounding below is the reference's (the library and tests/test_grid_plan.py are built with -ffp-contract=off).
// tests/test_grid_plan.py walks all of it on a CPU: against the statements it replaced, against the oracle's literal divideBox, against the hole
// filling's reference tables.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace rr {

// n / d == (n * m) >> k for every n < 2^27: with l = ceil(log2 d), k = 27 + l and m = floor(2^k / d) + 1 = (2^k + e) / d, 0 < e <= d <= 2^l,
// the product is n / d + n e / (d 2^k) with n e < 2^27 2^l = 2^k, i.e. less than 1 / d above the true quotient: the floor is the same.
// (tile ids stay below 2^27: resolutions are capped at 4096 = 512 tiles per axis)   {m, k}: the members of tsdf_common.hpp's FastDiv
struct DivPlan { uint32_t m, k; };
inline DivPlan make_fast_div(uint32_t d) {
  uint32_t l = 0;
  while ((1ull << l) < d) ++l;
  DivPlan f;
  f.k = 27 + l;
  f.m = (uint32_t)(((1ull << f.k) / d) + 1);
  return f;
}

// ---- setVoxelSize(), recon_integration.cpp:340-347: res = ceil(bbox / size) in fp32 -- or, with res_in[0] != 0, the resolution as given and the voxel
// size that follows from it.  Planes per axis in [1, 4096] (decided on the float and on the unsigned value: nothing out of range is converted)
struct VoxelGrid {
  enum Error { kOk, kVoxelSize, kResolution };
  int res[3];
  float vox[3];
  Error error;
  static VoxelGrid of(const float bbox_min[3], const float bbox_max[3], float voxel_size, const uint32_t res_in[3]) {
    VoxelGrid G{};
    for (int a = 0; a < 3; ++a) {
      const float ext = bbox_max[a] - bbox_min[a];
      if (res_in[0] == 0) {
        if (!(voxel_size > 0.0f)) { G.error = kVoxelSize; return G; }
        const float planes = ceilf(ext / voxel_size);
        if (!(planes >= 1.0f && planes <= 4096.0f)) { G.error = kResolution; return G; }
        G.res[a] = (int)planes;
        G.vox[a] = voxel_size;
      } else {
        if (res_in[a] < 1 || res_in[a] > 4096) { G.error = kResolution; return G; }
        G.res[a] = (int)res_in[a];
        G.vox[a] = ext / (float)res_in[a];
      }
    }
    return G;
  }
};

// ---- ViewLod::setResolution, view_lod.cpp:24-50: the pyramid levels of a w x h view beside each other in one (int)(1.5 w) x h atlas
constexpr int kAtlasMaxLods = 20;                                        // TSDF_MAX_LODS (abi.cpp asserts it)
struct AtlasPlan {
  bool ok;                                                               // false: a side below 2 or above 16384
  int num_lods, aw, h;
  int off[kAtlasMaxLods][2], res[kAtlasMaxLods][2];                      // (levels past num_lods: 0)
  static AtlasPlan of(uint32_t w, uint32_t h) {
    AtlasPlan A{};
    if (w < 2 || h < 2 || w > 16384 || h > 16384) return A;
    A.ok = true;
    A.num_lods = 1 + (int)floorf(log2f((float)std::min(w, h)));          // :25
    if (A.num_lods > kAtlasMaxLods) A.num_lods = kAtlasMaxLods;
    A.aw = (int)((float)w * 1.5f);                                       // :29 uvec2{width * 1.5f, height}
    A.h = (int)h;
    int ox = (int)w, oy = (int)h;                                        // :37
    for (int i = 0; i < A.num_lods; ++i) {
      A.res[i][0] = (int)floorf((float)w / powf(2.0f, (float)i));        // :39
      A.res[i][1] = (int)floorf((float)h / powf(2.0f, (float)i));
      if (i > 0) { oy -= A.res[i][1]; A.off[i][0] = ox; A.off[i][1] = oy; }   // :42-45
    }
    return A;
  }
};

// ---- setBrickSize + divideBox, recon_integration.cpp:462-472, :360-406, with the per-brick voxel lists of VolumeSampler::containedVoxels
// (volume_sampler.cpp:50-62) kept as per-axis ranges: along axis a voxel v lies in bricks [vox_first[a][v], vox_first[a][v] + vox_count[a][v]).
// From them, per storage tile index along an axis the first / last brick whose voxel list reaches into it (tile_b0 > tile_b1: none) and whether
// every voxel coordinate of the tile is in some brick's list (tile_full), and the inverse: per brick index the first / last storage tile its list
// reaches into (brick_t0 > brick_t1: the brick holds no voxel -- the fp32 sliver at the end of divideBox's loop).
struct BrickPlan {
  enum Error { kOk, kNotPositive, kRoundsToZero, kTooManyBricks, kDegenerateOverlap };
  Error error;
  int error_axis;
  float size[3];                                                         // snapped to whole voxels
  int res[3], n;                                                         // brick grid
  std::vector<uint16_t> vox_first[3], tile_b0[3], tile_b1[3], brick_t0[3], brick_t1[3];
  std::vector<uint8_t> vox_count[3], tile_full[3];
  bool uniform;                                                          // tiles == bricks structurally: every voxel in exactly one brick per axis, and a tile never straddles two
  size_t counter_words;                                                  // per-brick counters, padded: one aligned fill kernel; k_update_occupied reads whole quads

  static BrickPlan of(const float bbox_min[3], const float bbox_max[3], const int vres[3], const float vox[3], const float req[3]) {
    BrickPlan P{};
    auto refuse = [&P](Error e, int axis) -> BrickPlan& { P.error = e; P.error_axis = axis; return P; };
    for (int a = 0; a < 3; ++a) if (!(req[a] > 0.0f)) return refuse(kNotPositive, a);
    const float* bmin = bbox_min;
    float ext[3];
    for (int a = 0; a < 3; ++a) {
      ext[a] = bbox_max[a] - bbox_min[a];
      P.size[a] = vox[a] * roundf(req[a] / vox[a]);                     // :463
      if (!(P.size[a] > 0.0f)) return refuse(kRoundsToZero, a);
    }
    // the three nested while loops of divideBox() are separable: per axis, the sequence of brick starts
    std::vector<float> starts[3];
    for (int a = 0; a < 3; ++a) {
      float s = bmin[a];
      while (ext[a] - s + bmin[a] > 0.0f) {                             // :366-368
        starts[a].push_back(s);
        s += P.size[a];                                                 // :373,:379,:385
        if (starts[a].size() > 65535) return refuse(kTooManyBricks, a);
      }
      P.res[a] = (int)starts[a].size();
    }
    P.n = P.res[0] * P.res[1] * P.res[2];
    for (int a = 0; a < 3; ++a) {
      // containedVoxels(): for (v = pos/step; v < (pos+size)/step; ++v), all in float
      std::vector<uint16_t>& first = P.vox_first[a];
      std::vector<uint8_t>& count = P.vox_count[a];
      const float step = 1.0f / (float)vres[a];
      first.assign(vres[a], 0); count.assign(vres[a], 0);
      for (size_t b = 0; b < starts[a].size(); ++b) {
        const float bs = std::min(P.size[a], ext[a] - starts[a][b] + bmin[a]);   // :369 glm::min(brick, size - start + min)
        const float pos = (starts[a][b] - bmin[a]) / ext[a], sz = bs / ext[a];   // :371
        unsigned v = (unsigned)(pos / step);
        for (; (float)v < (pos + sz) / step; ++v) {
          if (v >= (unsigned)vres[a]) break;
          if (count[v] == 0) first[v] = (uint16_t)b;
          if (count[v] == 255 || (unsigned)first[v] + count[v] != b) return refuse(kDegenerateOverlap, a);
          count[v]++;
        }
      }
      const int nt = (vres[a] + 7) / 8;
      P.tile_b0[a].assign(nt, 1); P.tile_b1[a].assign(nt, 0); P.tile_full[a].assign(nt, 1);
      for (int t = 0; t < nt; ++t) {
        int lo = 0x7fffffff, hi = -1;
        for (int v = t * 8; v < std::min(t * 8 + 8, vres[a]); ++v) {
          if (count[v]) { lo = std::min(lo, (int)first[v]); hi = std::max(hi, (int)first[v] + count[v] - 1); }
          else P.tile_full[a][t] = 0;
        }
        if (hi >= 0) { P.tile_b0[a][t] = (uint16_t)lo; P.tile_b1[a][t] = (uint16_t)hi; }
      }
      // and the inverse: the storage tiles a brick's voxel list reaches into
      const int nb = P.res[a];
      P.brick_t0[a].assign(nb, 1); P.brick_t1[a].assign(nb, 0);
      std::vector<int> blo(nb, 0x7fffffff), bhi(nb, -1);
      for (int v = 0; v < vres[a]; ++v)
        for (int k = 0; k < count[v]; ++k) { const int b = first[v] + k; blo[b] = std::min(blo[b], v >> 3); bhi[b] = std::max(bhi[b], v >> 3); }
      for (int b = 0; b < nb; ++b) if (bhi[b] >= 0) { P.brick_t0[a][b] = (uint16_t)blo[b]; P.brick_t1[a][b] = (uint16_t)bhi[b]; }
    }
    P.uniform = true;
    for (int a = 0; a < 3 && P.uniform; ++a)
      for (int v = 0; v < vres[a] && P.uniform; ++v)
        P.uniform = P.vox_count[a][v] == 1 && P.vox_first[a][v] == P.vox_first[a][v & ~7];
    P.counter_words = (((size_t)P.n + 3 + 63) / 64) * 64;
    return P;
  }

  // ---- the table blob: all 21 tables in one buffer, table t of axis a at offset(t, a), every table on a multiple of 256 bytes (what a device
  // allocation of its own is aligned to at the least: whatever width a kernel loads a table with stays valid)
  enum Table { kVoxFirst, kVoxCount, kTileB0, kTileB1, kTileFull, kBrickT0, kBrickT1, kTables };
  static constexpr size_t kTableAlign = 256;
  struct Span { const void* data; size_t bytes; };
  Span table(int t, int a) const {
    auto u16 = [](const std::vector<uint16_t>& v) { return Span{v.data(), v.size() * sizeof(uint16_t)}; };
    auto u8 = [](const std::vector<uint8_t>& v) { return Span{v.data(), v.size()}; };
    switch (t) {
      case kVoxFirst: return u16(vox_first[a]);
      case kVoxCount: return u8(vox_count[a]);
      case kTileB0: return u16(tile_b0[a]);
      case kTileB1: return u16(tile_b1[a]);
      case kTileFull: return u8(tile_full[a]);
      case kBrickT0: return u16(brick_t0[a]);
      default: return u16(brick_t1[a]);
    }
  }
  // (tables in order, x y z of each; offset(kTables, 0) is the blob's size)
  size_t offset(int t, int a) const {
    size_t at = 0;
    for (int i = 0; i < t * 3 + a; ++i) at += (table(i / 3, i % 3).bytes + kTableAlign - 1) / kTableAlign * kTableAlign;
    return at;
  }
  std::vector<uint8_t> blob() const {
    std::vector<uint8_t> out(offset(kTables, 0), 0);
    for (int t = 0; t < kTables; ++t)
      for (int a = 0; a < 3; ++a) { const Span s = table(t, a); if (s.bytes) memcpy(out.data() + offset(t, a), s.data, s.bytes); }
    return out;
  }
};

// ---- the tile layers of a Z-slab [slab_z0, slab_z1) of voxel planes ((0, 0): the whole volume) in a volume of res voxels, 8 x 8 x 8 storage tiles.
// How far past a slab face an owned sample can make a context read (x = limit / 2 * res_z voxels = one sampleDistance): the refined hit position
// lies up to one step behind the owned sample (tsdf_raymarch.fs:99-101), its gradient taps another sampleDistance further (:140-149), and the
// trilinear footprint of that tap half a voxel + one plane beyond: ceil(2x + 0.5) planes below the face, floor(2x + 0.5) + 1 above.
// (limit * res_z + 2) planes cover both.
inline int halo_layers_for(float limit, int res_z) { return (int)ceilf((limit * (float)res_z + 2.0f) / 8.0f); }

struct SlabPlan {
  enum Error { kOk, kRange, kThinnerThanHalo, kStorageTiles, kSparseNeedsRecompute, kSparsePool, kVoxels };
  Error error;
  int ntx, nty;                    // tiles per axis (x, y)
  DivPlan div_layer, div_row;      // tile id / (ntx * nty), (tile id within a layer) / ntx
  int own_tz0, own_tz1;            // owned tile layers
  int tz0, tz1;                    // stored: owned + halo
  int int_tz0, int_tz1;            // integrated: the owned ones, plus the halo when it is recomputed locally
  int zlo, zhi;                    // stored voxel planes [zlo, zhi]
  int n_stored_tiles;
  uint32_t pool_tiles;             // sparse storage: the pool's tiles (0: dense)
  int halo_layers;
  int tiles_n;                     // integrated tiles
  uint64_t nvox;                   // voxels of storage: the pool's, or the stored tiles'

  static SlabPlan of(const int res[3], uint32_t slab_z0, uint32_t slab_z1, float limit, bool recompute_halo, uint32_t sparse_pool_tiles) {
    SlabPlan S{};
    auto refuse = [&S](Error e) -> SlabPlan& { S.error = e; return S; };
    S.ntx = (res[0] + 7) / 8; S.nty = (res[1] + 7) / 8;
    S.div_layer = make_fast_div((uint32_t)(S.ntx * S.nty)); S.div_row = make_fast_div((uint32_t)S.ntx);
    const int ntz = (res[2] + 7) / 8;
    uint32_t z0 = slab_z0, z1 = slab_z1;
    if (z0 == 0 && z1 == 0) z1 = (uint32_t)res[2];
    if (z1 > (uint32_t)res[2] || z0 >= z1 || (z0 % 8) != 0 || (z1 % 8 != 0 && z1 != (uint32_t)res[2])) return refuse(kRange);
    S.own_tz0 = (int)z0 / 8; S.own_tz1 = ((int)z1 + 7) / 8;
    S.halo_layers = halo_layers_for(limit, res[2]);
    const bool whole = (S.own_tz0 == 0 && S.own_tz1 == ntz);
    S.tz0 = whole ? 0 : std::max(0, S.own_tz0 - S.halo_layers);
    S.tz1 = whole ? ntz : std::min(ntz, S.own_tz1 + S.halo_layers);
    S.zlo = S.tz0 * 8; S.zhi = std::min(S.tz1 * 8, res[2]) - 1;
    const bool recompute = !whole && recompute_halo;
    S.int_tz0 = recompute ? S.tz0 : S.own_tz0;
    S.int_tz1 = recompute ? S.tz1 : S.own_tz1;
    if (!whole && S.own_tz1 - S.own_tz0 < S.halo_layers) return refuse(kThinnerThanHalo);
    const bool sparse = sparse_pool_tiles > 0;
    const uint64_t stored = (uint64_t)(S.tz1 - S.tz0) * S.nty * S.ntx;
    if (stored >= (1ull << 31)) return refuse(kStorageTiles);
    S.n_stored_tiles = (int)stored;
    if (sparse && !whole && !recompute) return refuse(kSparseNeedsRecompute);
    if (sparse && sparse_pool_tiles >= (1u << 23)) return refuse(kSparsePool);
    S.nvox = (sparse ? (uint64_t)sparse_pool_tiles : stored) * 512;      // (TILE_VOX)
    if (S.nvox >= (1ull << 32)) return refuse(kVoxels);
    S.pool_tiles = sparse_pool_tiles;
    S.tiles_n = (S.int_tz1 - S.int_tz0) * S.nty * S.ntx;
    return S;
  }
};

// ---- the largest LUT texel box any 8^3 tile of a volume of res voxels touches in an inverse LUT of inv_res texels, with the integrate kernel's own
// fp32 index arithmetic, against the LDS budget of the integrate kernels (box_cap texels, row_cap floats: k_integrate.hip's kBoxCap / kRowCap):
// cls 0 = the box does not fit (global-memory kernel), 1 = it fits (direct 8-tap form), 2 = the separable passes' rows and planes fit as well
struct LutFit {
  int dz;                          // the most z-planes of the LUT any tile touches
  int cls;
  // the texel left of voxel v's sample position, clamped like the kernel's tap (+ up: the one right of it)
  static int texel(int v, float step, int n, int up) {
    const float f = ((float)v + 0.5f) * step * (float)n - 0.5f;
    const int k = (int)fminf(fmaxf(floorf(f), -1.0f), (float)n);
    return std::min(std::max(k + up, 0), n - 1);
  }
  static LutFit of(const int res[3], const int inv_res[3], int box_cap, int row_cap) {
    int w[3] = {1, 1, 1};                                                // texels per axis of the worst tile
    for (int a = 0; a < 3; ++a) {
      const float step = 1.0f / (float)res[a];
      const int n = inv_res[a];
      for (int t = 0; t * 8 < res[a]; ++t) w[a] = std::max(w[a], texel(std::min(t * 8 + 7, res[a] - 1), step, n, 1) - texel(t * 8, step, n, 0) + 1);
    }
    return LutFit{w[2], w[0] * w[1] * w[2] > box_cap ? 0 : ((w[1] * w[2] * 8 <= row_cap && w[2] * 64 <= box_cap) ? 2 : 1)};
  }
};

}  // namespace rr
