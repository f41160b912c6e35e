"""CPU: the grid set-up's arithmetic (rgbd-recon_amd/csrc/grid_plan.hpp, HIP-free) as a stand-alone program with its own main, built with
-ffp-contract=off like the library and with the host address and undefined-behaviour sanitizers.  Three parts.
(a) Against the statements it replaced -- setup_view, setup_bricks, setup_volume, fit_lut_to_volume and the two copies of "resolution from voxel size" as
they stood in abi.cpp, restated below with the HIP calls left out: every output field, every table element and the error class, row by row.
(b) Against the oracle, whose divide_box is the reference's literal three nested loops: for the grids tests/test_oracle_bricks.py and
tests/test_gpu_round2.py pin, the voxels whose [first, first + count) holds a brick's index along an axis are the oracle's [lo, hi) of that brick.
(c) AtlasPlan against tests/fill_reference.lod_tables."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from fill_reference import lod_tables
from helpers import tiny_scene
from oracle.oracle import OracleRecon

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbd-recon_amd", "csrc")
f32 = np.float32

MAIN = r'''
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>
#include "grid_plan.hpp"
using namespace rr;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #x); std::exit(1); } } while (0)

// ================================================================ (a) the statements grid_plan.hpp replaced, as they stood in abi.cpp (the HIP calls
// between them left out; `c->` fields are members of the Old* structs; a FAIL is `return <class>`)

// ---- tsdf_create's "setVoxelSize(), :340-347" and tsdf_set_voxel_size's copy of it.  0 ok, 1 "voxel_size must be > 0 ...", 2 "... out of range [1, 4096]"
struct OldGrid { int res[3]; float vox[3]; };
static int old_create_grid(const float bbox_min[3], const float bbox_max[3], float voxel_size, const uint32_t cfg_res[3], OldGrid* c) {
  for (int a = 0; a < 3; ++a) {
    const float ext = bbox_max[a] - bbox_min[a];
    if (cfg_res[0] == 0) {
      if (!(voxel_size > 0.0f)) return 1;
      c->res[a] = (int)ceilf(ext / voxel_size);
      c->vox[a] = voxel_size;
    } else {
      c->res[a] = (int)cfg_res[a];
      c->vox[a] = ext / (float)cfg_res[a];
    }
    if (c->res[a] < 1 || c->res[a] > 4096) return 2;
  }
  return 0;
}
static int old_set_voxel_size(const float bbox_min[3], const float bbox_max[3], float size, OldGrid* c) {
  int res[3];
  for (int a = 0; a < 3; ++a) {
    res[a] = (int)ceilf((bbox_max[a] - bbox_min[a]) / size);
    if (res[a] < 1 || res[a] > 4096) return 2;
  }
  for (int a = 0; a < 3; ++a) { c->res[a] = res[a]; c->vox[a] = size; }
  return 0;
}

// ---- make_fast_div
struct OldFastDiv { uint32_t m, k; };
static OldFastDiv old_make_fast_div(uint32_t d) {
  uint32_t l = 0;
  while ((1ull << l) < d) ++l;
  OldFastDiv f;
  f.k = 27 + l;
  f.m = (uint32_t)(((1ull << f.k) / d) + 1);
  return f;
}

// ---- setup_view.  false: "view size %ux%u out of range"
static const int OLD_MAX_LODS = 20;                       // TSDF_MAX_LODS
struct OldAtlas { int aw, h, num_lods, off[OLD_MAX_LODS][2], res[OLD_MAX_LODS][2]; };
static bool old_setup_view(uint32_t w, uint32_t h, OldAtlas& A) {
  if (w < 2 || h < 2 || w > 16384 || h > 16384) return false;
  A.num_lods = 1 + (int)floorf(log2f((float)std::min(w, h)));
  if (A.num_lods > OLD_MAX_LODS) A.num_lods = OLD_MAX_LODS;
  A.aw = (int)((float)w * 1.5f);
  A.h = (int)h;
  int ox = (int)w, oy = (int)h;
  for (int i = 0; i < OLD_MAX_LODS; ++i) { A.off[i][0] = A.off[i][1] = A.res[i][0] = A.res[i][1] = 0; }
  for (int i = 0; i < A.num_lods; ++i) {
    A.res[i][0] = (int)floorf((float)w / powf(2.0f, (float)i));
    A.res[i][1] = (int)floorf((float)h / powf(2.0f, (float)i));
    if (i > 0) { oy -= A.res[i][1]; A.off[i][0] = ox; A.off[i][1] = oy; }
  }
  return true;
}
// ... and tsdf_draw_textures' second copy of the atlas width
static float old_draw_textures_rf_x(int vw) { return (float)(uint32_t)(1.5f * (float)vw); }

// ---- setup_bricks.  0 ok, 1 "brick size must be > 0", 2 "... rounds to zero voxels", 3 "more than 65535 bricks ...", 4 "degenerate ... on axis %d"
struct OldBricks {
  float size[3]; int res[3], n; int fail_axis;
  std::vector<uint16_t> first[3], t0[3], t1[3], bt0[3], bt1[3];
  std::vector<uint8_t> count[3], full[3];
  int uniform; size_t counter_words;
};
static int old_setup_bricks(const float cfg_bbox_min[3], const float cfg_bbox_max[3], const int c_res[3], const float c_vox[3], const float req[3], OldBricks& B) {
  for (int a = 0; a < 3; ++a) if (!(req[a] > 0.0f)) { B.fail_axis = a; return 1; }
  const float bmin[3] = {cfg_bbox_min[0], cfg_bbox_min[1], cfg_bbox_min[2]};
  float ext[3];
  for (int a = 0; a < 3; ++a) {
    ext[a] = cfg_bbox_max[a] - cfg_bbox_min[a];
    B.size[a] = c_vox[a] * roundf(req[a] / c_vox[a]);                 // :463
    if (!(B.size[a] > 0.0f)) { B.fail_axis = a; return 2; }
  }
  std::vector<float> starts[3];
  for (int a = 0; a < 3; ++a) {
    float s = bmin[a];
    while (ext[a] - s + bmin[a] > 0.0f) {                               // :366-368
      starts[a].push_back(s);
      s += B.size[a];                                                   // :373,:379,:385
      if (starts[a].size() > 65535) { B.fail_axis = a; return 3; }
    }
    B.res[a] = (int)starts[a].size();
  }
  B.n = B.res[0] * B.res[1] * B.res[2];
  std::vector<uint16_t>* first = B.first;
  std::vector<uint8_t>* count = B.count;
  for (int a = 0; a < 3; ++a) {
    const float step = 1.0f / (float)c_res[a];
    first[a].assign(c_res[a], 0); count[a].assign(c_res[a], 0);
    for (size_t b = 0; b < starts[a].size(); ++b) {
      const float bs = std::min(B.size[a], ext[a] - starts[a][b] + bmin[a]);   // :369
      const float pos = (starts[a][b] - bmin[a]) / ext[a], sz = bs / ext[a];   // :371
      unsigned v = (unsigned)(pos / step);
      for (; (float)v < (pos + sz) / step; ++v) {
        if (v >= (unsigned)c_res[a]) break;
        if (count[a][v] == 0) first[a][v] = (uint16_t)b;
        if (count[a][v] == 255 || (unsigned)first[a][v] + count[a][v] != b) { B.fail_axis = a; return 4; }
        count[a][v]++;
      }
    }
    const int nt = (c_res[a] + 7) / 8;
    std::vector<uint16_t> t0(nt, 1), t1(nt, 0);
    for (int t = 0; t < nt; ++t) {
      int lo = 0x7fffffff, hi = -1;
      for (int v = t * 8; v < std::min(t * 8 + 8, c_res[a]); ++v)
        if (count[a][v]) { lo = std::min(lo, (int)first[a][v]); hi = std::max(hi, (int)first[a][v] + count[a][v] - 1); }
      if (hi >= 0) { t0[t] = (uint16_t)lo; t1[t] = (uint16_t)hi; }
    }
    B.t0[a] = t0; B.t1[a] = t1;
    std::vector<uint8_t> full(nt, 1);
    for (int t = 0; t < nt; ++t)
      for (int v = t * 8; v < std::min(t * 8 + 8, c_res[a]); ++v) if (!count[a][v]) full[t] = 0;
    B.full[a] = full;
    const int nb = (int)starts[a].size();
    std::vector<uint16_t> bt0(nb, 1), bt1(nb, 0);
    std::vector<int> blo(nb, 0x7fffffff), bhi(nb, -1);
    for (int v = 0; v < c_res[a]; ++v)
      for (int k = 0; k < count[a][v]; ++k) { const int b = first[a][v] + k; blo[b] = std::min(blo[b], v >> 3); bhi[b] = std::max(bhi[b], v >> 3); }
    for (int b = 0; b < nb; ++b) if (bhi[b] >= 0) { bt0[b] = (uint16_t)blo[b]; bt1[b] = (uint16_t)bhi[b]; }
    B.bt0[a] = bt0; B.bt1[a] = bt1;
  }
  bool uniform = true;
  for (int a = 0; a < 3 && uniform; ++a)
    for (int v = 0; v < c_res[a] && uniform; ++v)
      uniform = count[a][v] == 1 && first[a][v] == first[a][v & ~7];
  B.uniform = uniform ? 1 : 0;
  B.counter_words = (((size_t)B.n + 3 + 63) / 64) * 64;
  return 0;
}

// ---- setup_volume.  0 ok, then the six FAILs in the order they stood
static const int OLD_TILE_VOX = 512;
static int old_halo_layers_for(float limit, int res_z) { return (int)ceilf((limit * (float)res_z + 2.0f) / 8.0f); }
struct OldVolume {
  int res[3], ntx, nty; OldFastDiv div_layer, div_row; int tz0, tz1, own_tz0, own_tz1, int_tz0, int_tz1, zlo, zhi; uint32_t pool_tiles; int n_stored_tiles; float limit;
  int halo_layers, tiles_n; size_t nvox;                  // c->halo_layers, c->tiles.n, the local nvox
};
static int old_setup_volume(const int c_res[3], uint32_t cfg_slab_z0, uint32_t cfg_slab_z1, float cfg_limit, int cfg_slab_recompute_halo, uint32_t cfg_sparse_pool_tiles, OldVolume& V) {
  for (int a = 0; a < 3; ++a) V.res[a] = c_res[a];
  V.ntx = (c_res[0] + 7) / 8; V.nty = (c_res[1] + 7) / 8;
  V.div_layer = old_make_fast_div((uint32_t)(V.ntx * V.nty)); V.div_row = old_make_fast_div((uint32_t)V.ntx);
  const int ntz = (c_res[2] + 7) / 8;
  if (!(V.limit > 0.0f)) V.limit = cfg_limit;
  uint32_t z0 = cfg_slab_z0, z1 = cfg_slab_z1;
  if (z0 == 0 && z1 == 0) z1 = (uint32_t)c_res[2];
  if (z1 > (uint32_t)c_res[2] || z0 >= z1 || (z0 % 8) != 0 || (z1 % 8 != 0 && z1 != (uint32_t)c_res[2])) return 1;
  V.own_tz0 = (int)z0 / 8; V.own_tz1 = ((int)z1 + 7) / 8;
  V.halo_layers = old_halo_layers_for(V.limit, c_res[2]);
  const bool whole = (V.own_tz0 == 0 && V.own_tz1 == ntz);
  V.tz0 = whole ? 0 : std::max(0, V.own_tz0 - V.halo_layers);
  V.tz1 = whole ? ntz : std::min(ntz, V.own_tz1 + V.halo_layers);
  V.zlo = V.tz0 * 8; V.zhi = std::min(V.tz1 * 8, c_res[2]) - 1;
  const bool recompute = !whole && cfg_slab_recompute_halo != 0;
  V.int_tz0 = recompute ? V.tz0 : V.own_tz0;
  V.int_tz1 = recompute ? V.tz1 : V.own_tz1;
  if (!whole && V.own_tz1 - V.own_tz0 < V.halo_layers) return 2;
  const bool sparse = cfg_sparse_pool_tiles > 0;
  // (the parent assigned V.n_stored_tiles in front of this check, in int: beyond 2^31 tiles -- which the library's resolution cap keeps it from, and this
  //  walk does not -- that product overflows; here it follows the check, the one place where this restatement departs from the parent's order)
  if ((uint64_t)(V.tz1 - V.tz0) * V.nty * V.ntx >= (1ull << 31)) return 3;
  V.n_stored_tiles = (V.tz1 - V.tz0) * V.nty * V.ntx;
  if (sparse && !whole && !recompute) return 4;
  if (sparse && cfg_sparse_pool_tiles >= (1u << 23)) return 5;
  const size_t nvox = sparse ? (size_t)cfg_sparse_pool_tiles * OLD_TILE_VOX : (size_t)(V.tz1 - V.tz0) * V.nty * V.ntx * OLD_TILE_VOX;
  if (nvox >= (1ull << 32)) return 6;
  V.nvox = nvox;
  V.pool_tiles = 0;
  if (sparse) V.pool_tiles = cfg_sparse_pool_tiles;
  V.tiles_n = (V.int_tz1 - V.int_tz0) * V.nty * V.ntx;
  return 0;
}

// ---- fit_lut_to_volume
struct OldFit { int lut_dz, lds_ok; };
static OldFit old_fit_lut_to_volume(const int c_res[3], const int L_inv_res[3], int integrate_box_cap, int integrate_row_cap) {
  int worst[3] = {1, 1, 1};
  for (int a = 0; a < 3; ++a) {
    const float step = 1.0f / (float)c_res[a];
    const int n = L_inv_res[a];
    auto idx0 = [&](int v) { float f = ((float)v + 0.5f) * step * (float)n - 0.5f; int k = (int)fminf(fmaxf(floorf(f), -1.0f), (float)n); return std::min(std::max(k, 0), n - 1); };
    auto idx1 = [&](int v) { float f = ((float)v + 0.5f) * step * (float)n - 0.5f; int k = (int)fminf(fmaxf(floorf(f), -1.0f), (float)n); return std::min(std::max(k + 1, 0), n - 1); };
    for (int t = 0; t * 8 < c_res[a]; ++t) worst[a] = std::max(worst[a], idx1(std::min(t * 8 + 7, c_res[a] - 1)) - idx0(t * 8) + 1);
  }
  OldFit F;
  F.lut_dz = worst[2];
  F.lds_ok = worst[0] * worst[1] * worst[2] > integrate_box_cap ? 0 : ((worst[1] * worst[2] * 8 <= integrate_row_cap && worst[2] * 64 <= integrate_box_cap) ? 2 : 1);
  return F;
}

// ================================================================ the walks
static bool same_bits(float a, float b) { return memcmp(&a, &b, sizeof(float)) == 0; }
template <class T> static bool same_vec(const std::vector<T>& a, const std::vector<T>& b) { return a == b; }

static const float kExtents[4][2] = {{0.0f, 1.0f}, {-1.0f, 1.0f}, {0.0f, 2.2f}, {-0.35f, 0.85f}};

// one brick row: the old statements and the plan on the same values; the blob's layout on every accepted plan
static void bricks_row(const float bmin[3], const float bmax[3], const int res[3], const float vox[3], const float req[3], int want_error) {
  OldBricks O; const int oe = old_setup_bricks(bmin, bmax, res, vox, req, O);
  const BrickPlan P = BrickPlan::of(bmin, bmax, res, vox, req);
  bool ok = oe == (int)P.error && (want_error < 0 || oe == want_error);
  if (ok && oe) ok = O.fail_axis == P.error_axis;
  if (ok && !oe) {
    ok = O.n == P.n && O.uniform == (P.uniform ? 1 : 0) && O.counter_words == P.counter_words;
    for (int a = 0; a < 3 && ok; ++a)
      ok = same_bits(O.size[a], P.size[a]) && O.res[a] == P.res[a] && same_vec(O.first[a], P.vox_first[a]) && same_vec(O.count[a], P.vox_count[a]) &&
           same_vec(O.t0[a], P.tile_b0[a]) && same_vec(O.t1[a], P.tile_b1[a]) && same_vec(O.full[a], P.tile_full[a]) && same_vec(O.bt0[a], P.brick_t0[a]) &&
           same_vec(O.bt1[a], P.brick_t1[a]);
  }
  if (!ok) {
    std::fprintf(stderr, "bricks: box [%a %a %a, %a %a %a] res %d %d %d vox %a %a %a req %a %a %a: old class %d, plan %d\n", bmin[0], bmin[1], bmin[2], bmax[0], bmax[1],
                 bmax[2], res[0], res[1], res[2], vox[0], vox[1], vox[2], req[0], req[1], req[2], oe, (int)P.error);
    std::exit(1);
  }
  if (oe) return;
  // the blob: 21 tables, each on a multiple of 256 bytes, in order, none overlapping the next, each holding its table
  const std::vector<uint8_t> blob = P.blob();
  CHECK(blob.size() == P.offset(BrickPlan::kTables, 0) && blob.size() % BrickPlan::kTableAlign == 0);
  size_t end = 0;
  for (int t = 0; t < BrickPlan::kTables; ++t)
    for (int a = 0; a < 3; ++a) {
      const size_t at = P.offset(t, a), n = P.table(t, a).bytes;
      CHECK(at % 256 == 0 && at >= end && at + n <= blob.size());
      CHECK(n == 0 || memcmp(blob.data() + at, P.table(t, a).data, n) == 0);
      end = at + n;
    }
  CHECK(P.table(BrickPlan::kVoxFirst, 1).bytes == (size_t)res[1] * 2 && P.table(BrickPlan::kVoxCount, 2).bytes == (size_t)res[2] &&
        P.table(BrickPlan::kTileFull, 0).bytes == (size_t)(res[0] + 7) / 8 && P.table(BrickPlan::kBrickT1, 2).bytes == (size_t)P.res[2] * 2);
}
static unsigned long walk_bricks(unsigned long* grid_rows) {
  unsigned long rows = 0;
  // mode 0: explicit res 1..96 on every axis; modes 1, 2: res from the voxel sizes 0.01 and 0.04.  Axis a takes extent (e + a) % 4
  for (int mode = 0; mode < 3; ++mode)
    for (int e = 0; e < 4; ++e)
      for (int r = 1; r <= (mode == 0 ? 96 : 1); ++r) {
        float bmin[3], bmax[3];
        for (int a = 0; a < 3; ++a) { bmin[a] = kExtents[(e + a) % 4][0]; bmax[a] = kExtents[(e + a) % 4][1]; }
        const uint32_t res_in[3] = {mode == 0 ? (uint32_t)r : 0u, (uint32_t)r, (uint32_t)r};
        const float voxel_size = mode == 2 ? 0.04f : 0.01f;
        // resolution from voxel size: tsdf_create's statements, tsdf_set_voxel_size's, the plan
        OldGrid og{}; const int ge = old_create_grid(bmin, bmax, voxel_size, res_in, &og);
        const VoxelGrid G = VoxelGrid::of(bmin, bmax, voxel_size, res_in);
        CHECK(ge == 0 && G.error == VoxelGrid::kOk);
        for (int a = 0; a < 3; ++a) CHECK(og.res[a] == G.res[a] && same_bits(og.vox[a], G.vox[a]));
        if (mode) {
          OldGrid os{}; CHECK(old_set_voxel_size(bmin, bmax, voxel_size, &os) == 0);
          for (int a = 0; a < 3; ++a) CHECK(os.res[a] == G.res[a] && same_bits(os.vox[a], G.vox[a]));
        }
        ++*grid_rows;
        const int kmax = std::max(G.res[0], std::max(G.res[1], G.res[2])) + 1;
        for (int k = 1; k <= kmax; ++k)
          for (int half = 0; half < 2; ++half) {
            float req[3];
            for (int a = 0; a < 3; ++a) req[a] = half ? G.vox[a] * ((float)k + 0.49f) : G.vox[a] * (float)k;
            bricks_row(bmin, bmax, G.res, G.vox, req, 0);
            ++rows;
          }
      }
  // the refusals: a size that is not positive, one that rounds to zero voxels (on the last axis), more than 65535 bricks along an axis (the middle one:
  // voxels of 2^-20 under a resolution of 4096, which no VoxelGrid hands out), and their order when two axes fail differently
  {
    const float bmin[3] = {0.0f, 0.0f, 0.0f}, bmax[3] = {1.0f, 1.0f, 1.0f};
    const int res[3] = {32, 4096, 32};
    const float vox[3] = {1.0f / 32.0f, 1.0f / 32.0f, 1.0f / 32.0f}, fine[3] = {1.0f / 32.0f, 0x1p-20f, 1.0f / 32.0f};
    const float zero[3] = {0.25f, 0.25f, 0.0f}, nan[3] = {0.25f, NAN, 0.25f}, tiny[3] = {0.25f, 0.25f, 0.49f / 32.0f}, one[3] = {0.25f, 0x1p-20f, 0.25f};
    const float tiny_and_many[3] = {0.25f, 0x1p-20f, 0x1p-22f};
    bricks_row(bmin, bmax, res, vox, zero, BrickPlan::kNotPositive); bricks_row(bmin, bmax, res, vox, nan, BrickPlan::kNotPositive);
    bricks_row(bmin, bmax, res, vox, tiny, BrickPlan::kRoundsToZero);
    bricks_row(bmin, bmax, res, fine, one, BrickPlan::kTooManyBricks);
    bricks_row(bmin, bmax, res, fine, tiny_and_many, BrickPlan::kRoundsToZero);
    rows += 5;
  }
  return rows;
}

static unsigned long walk_slab() {
  unsigned long rows = 0, refused[7] = {0, 0, 0, 0, 0, 0, 0};
  const float limits[4] = {0.01f, 0.04f, 0.3f, 1.0f};
  const uint32_t pools[3] = {0u, 1u, 1u << 23};
  // (ntx, nty): 1 x 1, 3 x 2, 1024 x 1024 (2^32 voxels from 8 layers on), 16384 x 16384 (2^31 tiles from 8 layers on)
  const int xy[4][2] = {{8, 8}, {20, 13}, {8192, 8192}, {131072, 131072}};
  for (int rz = 1; rz <= 136; ++rz) {
    std::vector<std::pair<uint32_t, uint32_t>> ranges;
    const uint32_t top = (uint32_t)((rz + 7) / 8 * 8);
    for (uint32_t z0 = 0; z0 <= top; z0 += 8) {
      for (uint32_t z1 = 0; z1 <= top; z1 += 8) ranges.emplace_back(z0, z1);         // every tile-aligned pair ((0, 0): the default; z0 >= z1 and z1 > res_z: refused)
      ranges.emplace_back(z0, (uint32_t)rz);                                         // z1 = res_z, aligned or not
    }
    ranges.emplace_back(4u, (uint32_t)rz); ranges.emplace_back(0u, (uint32_t)rz - 1);  // not aligned
    for (const auto& z : ranges)
      for (float limit : limits)
        for (int recompute = 0; recompute < 2; ++recompute)
          for (uint32_t pool : pools)
            for (const auto& s : xy) {
              const int res[3] = {s[0], s[1], rz};
              OldVolume V{}; const int oe = old_setup_volume(res, z.first, z.second, limit, recompute, pool, V);
              const SlabPlan P = SlabPlan::of(res, z.first, z.second, limit, recompute != 0, pool);
              bool ok = oe == (int)P.error;
              if (ok && !oe)
                ok = V.ntx == P.ntx && V.nty == P.nty && V.div_layer.m == P.div_layer.m && V.div_layer.k == P.div_layer.k && V.div_row.m == P.div_row.m &&
                     V.div_row.k == P.div_row.k && V.own_tz0 == P.own_tz0 && V.own_tz1 == P.own_tz1 && V.tz0 == P.tz0 && V.tz1 == P.tz1 && V.int_tz0 == P.int_tz0 &&
                     V.int_tz1 == P.int_tz1 && V.zlo == P.zlo && V.zhi == P.zhi && V.n_stored_tiles == P.n_stored_tiles && V.pool_tiles == P.pool_tiles &&
                     V.halo_layers == P.halo_layers && V.tiles_n == P.tiles_n && (uint64_t)V.nvox == P.nvox;
              if (!ok) {
                std::fprintf(stderr, "slab: res %d %d %d range %u %u limit %g recompute %d pool %u: old class %d, plan %d\n", res[0], res[1], res[2], z.first, z.second,
                             limit, recompute, pool, oe, (int)P.error);
                std::exit(1);
              }
              ++refused[oe]; ++rows;
            }
  }
  for (int k = 0; k < 7; ++k) CHECK(refused[k] > 0);       // every class was met, the accepted one included
  CHECK(old_halo_layers_for(0.04f, 64) == halo_layers_for(0.04f, 64) && halo_layers_for(0.04f, 64) == 1 && halo_layers_for(0.3f, 136) == 6);
  return rows;
}

static const uint32_t kAtlasExtra[5][2] = {{1280, 720}, {1920, 1080}, {2, 16384}, {16384, 16384}, {16384, 2}};
static unsigned long walk_atlas() {
  unsigned long rows = 0;
  auto row = [&](uint32_t w, uint32_t h, bool accepted) {
    OldAtlas O; memset(&O, 0, sizeof(O));
    const bool ok = old_setup_view(w, h, O);
    const AtlasPlan P = AtlasPlan::of(w, h);
    CHECK(ok == accepted && P.ok == accepted);
    if (ok) {
      CHECK(O.num_lods == P.num_lods && O.aw == P.aw && O.h == P.h);
      CHECK(memcmp(O.off, P.off, sizeof(O.off)) == 0 && memcmp(O.res, P.res, sizeof(O.res)) == 0);
      CHECK(same_bits(old_draw_textures_rf_x((int)w), (float)P.aw));
    }
    ++rows;
  };
  for (uint32_t w = 2; w <= 130; ++w) for (uint32_t h = 2; h <= 130; ++h) row(w, h, true);
  for (const auto& s : kAtlasExtra) row(s[0], s[1], true);
  row(1, 100, false); row(100, 1, false); row(16385, 100, false); row(100, 16385, false);
  return rows;
}

static unsigned long walk_lut() {
  std::vector<int> vals;
  for (int v = 1; v <= 64; ++v) vals.push_back(v);
  for (int v : {200, 221, 256, 286, 315, 512}) vals.push_back(v);
  const int n = (int)vals.size();
  // {box_cap, row_cap}: the library's own -- k_integrate.hip:541,546-547: RR_K1_BOXCAP 384, kRowCap 512 --, a smaller and a larger budget
  const int caps[3][2] = {{384, 512}, {216, 256}, {512, 768}};
  unsigned long rows = 0, cls[3] = {0, 0, 0};
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j)
      for (const auto& cap : caps) {
        // the pair under test on x; y and z from elsewhere in the list, so that all three classes occur
        const int res[3] = {vals[i], vals[(i + 1) % n], vals[(i + 7) % n]}, inv[3] = {vals[j], vals[(j + 3) % n], vals[(j + 11) % n]};
        const OldFit O = old_fit_lut_to_volume(res, inv, cap[0], cap[1]);
        const LutFit F = LutFit::of(res, inv, cap[0], cap[1]);
        if (O.lut_dz != F.dz || O.lds_ok != F.cls) {
          std::fprintf(stderr, "lut fit: res %d %d %d inv %d %d %d caps %d %d: old dz %d class %d, plan dz %d class %d\n", res[0], res[1], res[2], inv[0], inv[1], inv[2], cap[0],
                       cap[1], O.lut_dz, O.lds_ok, F.dz, F.cls);
          std::exit(1);
        }
        ++cls[F.cls]; ++rows;
      }
  CHECK(cls[0] > 0 && cls[1] > 0 && cls[2] > 0);
  return rows;
}

static unsigned long walk_fast_div() {
  unsigned long rows = 0;
  for (uint32_t d = 1; d <= (1u << 18); d = d < 4200 ? d + 1 : d * 2 - 1) {                    // every divisor a volume of at most 512 tiles per axis has, then sparser
    const OldFastDiv o = old_make_fast_div(d); const DivPlan p = make_fast_div(d);
    CHECK(o.m == p.m && o.k == p.k);
    for (uint64_t n : {(uint64_t)0, (uint64_t)d - 1, (uint64_t)d, (uint64_t)d * 7 + 3, (uint64_t)(1u << 27) - 1}) if (n < (1u << 27)) CHECK(((n * p.m) >> p.k) == n / d);
    ++rows;
  }
  return rows;
}

// ================================================================ (b), (c): what the Python side compares
static void print_ints(const char* name, const int* v, int n) { std::printf("\"%s\": [", name); for (int i = 0; i < n; ++i) std::printf("%s%d", i ? ", " : "", v[i]); std::printf("]"); }
template <class T> static void print_table(const char* name, const std::vector<T>* t) {
  std::printf("\"%s\": [", name);
  for (int a = 0; a < 3; ++a) { std::printf("%s[", a ? ", " : ""); for (size_t i = 0; i < t[a].size(); ++i) std::printf("%s%u", i ? ", " : "", (unsigned)t[a][i]); std::printf("]"); }
  std::printf("]");
}
static void print_atlas(const AtlasPlan& A) {
  std::printf("{\"num_lods\": %d, \"aw\": %d, \"h\": %d, \"res\": [", A.num_lods, A.aw, A.h);
  for (int i = 0; i < A.num_lods; ++i) std::printf("%s[%d, %d]", i ? ", " : "", A.res[i][0], A.res[i][1]);
  std::printf("], \"off\": [");
  for (int i = 0; i < A.num_lods; ++i) std::printf("%s[%d, %d]", i ? ", " : "", A.off[i][0], A.off[i][1]);
  std::printf("]}");
}
// grid: bbox_min[3] bbox_max[3] voxel_size res[3] brick[3] view_w view_h, floats as C99 hex -> one JSON object
static int emit_grid(char** v) {
  float bmin[3], bmax[3], req[3]; uint32_t res_in[3];
  for (int a = 0; a < 3; ++a) { bmin[a] = strtof(v[a], nullptr); bmax[a] = strtof(v[3 + a], nullptr); res_in[a] = (uint32_t)strtoul(v[7 + a], nullptr, 10); req[a] = strtof(v[10 + a], nullptr); }
  const VoxelGrid G = VoxelGrid::of(bmin, bmax, strtof(v[6], nullptr), res_in);
  CHECK(G.error == VoxelGrid::kOk);
  const BrickPlan P = BrickPlan::of(bmin, bmax, G.res, G.vox, req);
  CHECK(P.error == BrickPlan::kOk);
  std::printf("{"); print_ints("res", G.res, 3); std::printf(", "); print_ints("res_bricks", P.res, 3);
  std::printf(", \"brick_size\": [\"%a\", \"%a\", \"%a\"], \"n\": %d, \"uniform\": %d, ", P.size[0], P.size[1], P.size[2], P.n, P.uniform ? 1 : 0);
  print_table("vox_first", P.vox_first); std::printf(", "); print_table("vox_count", P.vox_count); std::printf(", ");
  print_table("tile_b0", P.tile_b0); std::printf(", "); print_table("tile_b1", P.tile_b1); std::printf(", "); print_table("tile_full", P.tile_full); std::printf(", ");
  print_table("brick_t0", P.brick_t0); std::printf(", "); print_table("brick_t1", P.brick_t1);
  std::printf(", \"atlas\": "); print_atlas(AtlasPlan::of((uint32_t)strtoul(v[13], nullptr, 10), (uint32_t)strtoul(v[14], nullptr, 10)));
  std::printf("}\n");
  return 0;
}
static int emit_atlases() {
  std::printf("[");
  for (uint32_t w = 2; w <= 130; ++w) for (uint32_t h = 2; h <= 130; ++h) { if (w != 2 || h != 2) std::printf(",\n"); print_atlas(AtlasPlan::of(w, h)); }
  for (const auto& s : kAtlasExtra) { std::printf(",\n"); print_atlas(AtlasPlan::of(s[0], s[1])); }
  std::printf("]\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 17 && !strcmp(argv[1], "grid")) return emit_grid(argv + 2);
  if (argc == 2 && !strcmp(argv[1], "atlases")) return emit_atlases();
  CHECK(argc == 1);
  unsigned long grid_rows = 0;
  const unsigned long bricks = walk_bricks(&grid_rows);
  std::printf("against the old statements: %lu brick rows, %lu voxel grid rows, %lu slab rows, %lu atlas rows, %lu lut rows, %lu divisor rows\n", bricks, grid_rows, walk_slab(),
              walk_atlas(), walk_lut(), walk_fast_div());
  std::puts("grid plan ok");
  return 0;
}
'''


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("grid_plan")
    src = d / "grid_plan_main.cpp"
    src.write_text(MAIN)
    out = str(d / "grid_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, str(src), "-o", out])
    return out


def run(exe, *args):
    p = subprocess.run([exe, *args], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr
    return p.stdout


def test_grid_plan_includes_only_the_standard_library():
    with open(os.path.join(CSRC, "grid_plan.hpp")) as f:
        includes = [l.split()[1] for l in f if l.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i and "." not in i for i in includes), includes


def test_against_the_statements_it_replaces(exe):
    out = run(exe)
    print(out)
    assert "grid plan ok" in out
    rows = {name: int(n) for n, name in re.findall(r"(\d+) ([a-z ]+?) rows", out)}
    assert set(rows) == {"brick", "voxel grid", "slab", "atlas", "lut", "divisor"} and all(n > 0 for n in rows.values()), rows
    # explicit res: 4 boxes x (res + 1 lengths for res 1..96) x 2 requests; from a voxel size: 4 boxes x (the longest axis' planes + 1) x 2; 5 refusals
    ext = ((0, 1), (-1, 1), (0, 2.2), (-0.35, 0.85))
    planes = lambda lo, hi, size: int(np.ceil((f32(hi) - f32(lo)) / f32(size)))
    by_size = sum(2 * (max(planes(*ext[(e + a) % 4], size) for a in range(3)) + 1) for size in (0.01, 0.04) for e in range(4))
    assert rows["brick"] == 4 * 2 * sum(r + 1 for r in range(1, 97)) + by_size + 5 and rows["voxel grid"] == 4 * 96 + 8
    assert rows["atlas"] == 129 * 129 + 5 + 4 and rows["lut"] == 70 * 70 * 3


# ---- (b) the grids pinned for the oracle: (bbox, voxel size, res or None, brick size, view)
UNIT, ROOM = ((0, 0, 0), (1, 1, 1)), ((-1, 0, -1), (1, 2.2, 1))
GRIDS = {
    "reference default": (ROOM, 0.01, None, 0.1, (1280, 720)),                                   # 200 x 221 x 200 voxels, 20 x 22 x 20 bricks, overlapping lists
    "empty sixth brick": (UNIT, 0.04, None, 0.21, (8, 8)),                                       # 25^3 voxels, six bricks per axis
    "bricks of 8 voxels": (UNIT, 0.01, (20, 22, 20), [8 / 20, 8 / 22, 8 / 20], (160, 90)),
    "72 planes in bricks of 4": (ROOM, 0.01, (64, 72, 64), [2.0 / 16, 2.2 / 18, 2.0 / 16], (96, 64)),   # tests/test_gpu_round2.py:255: 19 bricks along y
}
EXPECT = {"reference default": ((200, 221, 200), (20, 22, 20)), "empty sixth brick": ((25, 25, 25), (6, 6, 6)), "bricks of 8 voxels": ((20, 22, 20), (3, 3, 3)),
          "72 planes in bricks of 4": ((64, 72, 64), (16, 19, 16))}


@pytest.mark.parametrize("name", list(GRIDS))
def test_brick_tables_against_the_oracle(exe, name):
    bbox, voxel, res, brick, view = GRIDS[name]
    sc = tiny_scene([(0.5, 0.5, 0.5)], [0.5], [1.0], [1.0])
    sc["bbox_min"], sc["bbox_max"] = f32(bbox[0]), f32(bbox[1])
    orc = OracleRecon(sc, res=res, voxel_size=voxel, brick_size=brick, limit=0.01, view=view)
    bs = [brick] * 3 if np.isscalar(brick) else brick
    hexf = lambda x: float(f32(x)).hex()
    plan = json.loads(run(exe, "grid", *[hexf(x) for x in bbox[0]], *[hexf(x) for x in bbox[1]], hexf(voxel), *[str(r) for r in (res or (0, 0, 0))], *[hexf(b) for b in bs],
                          str(view[0]), str(view[1])))
    assert (tuple(plan["res"]), tuple(plan["res_bricks"])) == (orc.res, orc.res_bricks) == EXPECT[name]
    assert [f32(float.fromhex(s)).tobytes() for s in plan["brick_size"]] == [f32(b).tobytes() for b in orc.brick_size]
    assert plan["n"] == orc.numBricks()
    rx, ry, rz = orc.res_bricks
    ranges = orc.brick_ranges().reshape(rz, ry, rx, 6).astype(np.int64)                            # brick id = z ry rx + y rx + x: {lo x y z, hi x y z}
    uniform = True
    for a in range(3):
        first, count = np.array(plan["vox_first"][a]), np.array(plan["vox_count"][a])
        nb, nv, nt = orc.res_bricks[a], orc.res[a], (orc.res[a] + 7) // 8
        assert first.size == count.size == nv
        lo, hi = np.moveaxis(ranges[..., a], 2 - a, 0).reshape(nb, -1), np.moveaxis(ranges[..., 3 + a], 2 - a, 0).reshape(nb, -1)
        assert (lo == lo[:, :1]).all() and (hi == hi[:, :1]).all()                                 # (an axis' range depends on the brick's index along it alone)
        sets = []
        for b in range(nb):                                                                        # the voxels whose [first, first + count) holds b == the oracle's [lo, hi)
            mine = set(np.flatnonzero((first <= b) & (b < first + count)).tolist())
            assert mine == set(range(int(lo[b, 0]), int(hi[b, 0]))), (name, a, b)
            sets.append(mine)
        # ... and the five tables derived from them, from the oracle's ranges
        for t in range(nt):
            tile = set(range(t * 8, min(t * 8 + 8, nv)))
            reach = [b for b in range(nb) if sets[b] & tile]
            assert (plan["tile_b0"][a][t], plan["tile_b1"][a][t]) == ((reach[0], reach[-1]) if reach else (1, 0))
            assert plan["tile_full"][a][t] == int(all(any(v in s for s in sets) for v in tile))
            uniform = uniform and len(reach) == 1                                                  # a tile never straddles two bricks ...
        for b in range(nb):
            assert (plan["brick_t0"][a][b], plan["brick_t1"][a][b]) == ((min(sets[b]) >> 3, max(sets[b]) >> 3) if sets[b] else (1, 0))
        uniform = uniform and all(sum(v in s for s in sets) == 1 for v in range(nv))               # ... and every voxel lies in exactly one
    assert plan["uniform"] == int(uniform)
    if name == "empty sixth brick":
        assert plan["vox_count"][0].count(0) == 0 and (plan["brick_t0"][0][5], plan["brick_t1"][0][5]) == (1, 0)   # the sliver holds no voxel
    if name == "reference default":
        assert max(plan["vox_count"][0]) == 2 and plan["uniform"] == 0                             # neighbouring lists overlap by one plane
    # the atlas of the oracle's view
    off, lres = orc.lod_tables()
    A = plan["atlas"]
    assert A["num_lods"] == orc.num_lods and (np.array(A["off"]) == off).all() and (np.array(A["res"]) == lres).all()
    assert (A["aw"], A["h"]) == (int(f32(view[0]) * f32(1.5)), view[1])


# ---- (c) the hole filling's reference tables, over the levels both hold
def test_atlas_plan_against_the_fill_reference(exe):
    sizes = [(w, h) for w in range(2, 131) for h in range(2, 131)] + [(1280, 720), (1920, 1080), (2, 16384), (16384, 16384), (16384, 2)]
    plans = json.loads(run(exe, "atlases"))
    assert len(plans) == len(sizes)
    for (w, h), A in zip(sizes, plans):
        t = lod_tables(w, h)
        n = min(A["num_lods"], t["num_lods"])
        assert n == t["num_lods"] == A["num_lods"] >= 1, (w, h)                                    # (20 levels would take a side of 2^19)
        assert (A["aw"], A["h"]) == t["full"], (w, h)
        assert (np.array(A["res"][:n]) == t["res"][:n]).all() and (np.array(A["off"][:n]) == t["off"][:n]).all(), (w, h)
