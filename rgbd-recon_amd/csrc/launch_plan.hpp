// Which kernels one integrate() / one march launches and with what grids: decided once per call, from plain scalars, by pure functions.
// Host only and free of HIP (a plain C++ compiler takes this header alone: tests/test_launch_plan.py); the launchers of k_integrate.hip
// and k_raymarch.hip make exactly the launch the plan names and decide nothing themselves.
#pragma once
#include <cstdint>

namespace rr {

// The forms are the TSDF_K1_* values of rgbd_recon_hip.h; kFormCached = k_integrate_cached + the separable LDS kernel for the tiles the
// cache does not hold (grid: the latter's)
enum { kFormGeneric = 0, kFormLdsDirect = 1, kFormLdsSeparable = 2, kFormRecord = 3, kFormCached = 4 };
struct IntegratePlan {
  int form = -1;                // kForm*: which kernel integrates (-1: no integrate() since the volume was set up)
  bool culled = false;          // the work items are the active-tile list of the brick culling / every tile
  bool per_voxel_check = false; // a work item's voxels are tested against their bricks (culled, bricks not aligned to the tiles)
  bool ranges = false;          // the kernel takes the frame's (tile, stream) pair classes ...
  bool pair_pass = false;       // ... which k_pair_masks writes first
  bool rec = false;             // the pair pass leaves 16-byte work records, k_integrate_tiles_rec reads them
  bool cached = false;          // the pair pass classifies the work items for the projection cache, k_integrate_cached takes the cached ones
  uint32_t grid = 0;            // workgroups of the integrate kernel (of the LDS kernel when cached)
};
// lds_ok: 0 .. 2 as in tsdf_ctx::lds_ok, already capped by RR_K1_FORM; have_bounds: the tile-bounds table and the pair-mask buffer exist;
// forced_grid (RR_K1_GRID, 0 = none) / dense_cap (RR_K1_DENSE_GRID, 0 = none): the A/B hooks, read by the caller
inline IntegratePlan plan_integrate(bool culled, int lds_ok, bool have_range_cells, bool have_bounds, bool have_recs, bool cache_usable, bool sparse, bool uniform_bricks,
                                    int n_tiles, int forced_grid, int dense_cap) {
  IntegratePlan P;
  P.culled = culled;
  P.per_voxel_check = culled && !uniform_bricks;
  P.ranges = P.pair_pass = have_range_cells && have_bounds && lds_ok >= 2;
  P.cached = P.ranges && cache_usable;
  P.rec = P.ranges && !P.cached && !sparse && have_recs;
  P.form = P.cached ? kFormCached : P.rec ? kFormRecord : lds_ok >= 2 ? kFormLdsSeparable : lds_ok ? kFormLdsDirect : kFormGeneric;
  // Culled: the workgroups stride over the work list.  2048 = the 8 x 256 a MI355X holds at once: beside the other lanes' kernels (stage overlap) a c2 frame takes
  // 112 - 113 us with it against 119 with 4096 (the launch alone 43.9 against 42.9 us: queued workgroups of this kernel no longer take the slots a co-runner's
  // workgroups wait for), c3 the same either way; the 25 000-tile launch of a 1024^3 volume wants the larger grid (c4: 2 834 against 2 551 frames/s).
  // Dense with pair classes: at most 16 384 workgroups striding over the tiles instead of one per tile: the launch alone is as fast (119 us at c1), the frame beside
  // the other lanes 2.5 % faster (4 349 against 4 242 frames/s; 8 192: 4 380 but the launch alone 125 us, 2 048: 3 796).  Otherwise one workgroup per tile.
  int cap = n_tiles;
  if (culled) cap = forced_grid > 0 ? forced_grid : (n_tiles <= 262144 ? 2048 : 4096);
  else if (P.ranges && !P.cached && dense_cap > 0) cap = dense_cap;
  P.grid = (uint32_t)(n_tiles < cap ? n_tiles : cap);
  return P;
}

enum { kMarchPartial = 0, kMarchTwoPass, kMarchBoxPair, kMarchBox, kMarchGather };
struct MarchPlan {
  int kernel;       // kMarch*: a Z-slab's partial march, the first of two passes (long rays handed on), k_march_box with two boxes per wave / one, the plain gather march
  bool two_pass;    // rays still running after `cap` samples go to the long list, and k_shade_and_long finishes them beside the shading
  bool sparse;      // the volume is a tile pool
  uint32_t cap;     // what k_march gets: the sample cap of a two-pass march, 0xffffffff otherwise
};
// cap: 0xffffffff = no second pass; box_mode: tsdf_ctx::march_box
inline MarchPlan plan_march(bool partial, bool skip, bool sparse, bool have_long_list, uint32_t cap, int box_mode) {
  MarchPlan M;
  M.two_pass = !partial && skip && have_long_list && cap != 0xffffffffu;
  M.sparse = sparse;
  M.cap = M.two_pass ? cap : 0xffffffffu;
  const bool box = !sparse && !skip && box_mode != 0;
  M.kernel = partial ? kMarchPartial : M.two_pass ? kMarchTwoPass : box ? (box_mode == 2 ? kMarchBoxPair : kMarchBox) : kMarchGather;
  return M;
}

}  // namespace rr
