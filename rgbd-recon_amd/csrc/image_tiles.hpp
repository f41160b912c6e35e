// The view's dirty-tile bookkeeping: which 8x8-pixel tiles of the picture the recent draws touched, and what the frame loop may skip because
// of it.  Host only, free of HIP: the state and one named transition per event, handing back plain values (indices into tsdf_ctx::d_touched,
// booleans, RayTarget's two rewrite_* ints).  Device pointers, launches and the swap of the two peel images stay in abi.cpp, driven by what a
// transition returns.  tests/test_image_tiles.py walks every state, event and input on a CPU.
//
// Three masks in rotation (k_raymarch.hip): d_touched[touched_idx] is the coming draw's, (idx + 2) % 3 the previous draw's (peels, sample
// counts), (idx + 1) % 3 the one before (the other pyramid when two alternate; recycled by the march).  A draw with space skipping that takes
// part ("tiled": no shifted viewport, no masked-direct target, RR_IMAGE_TILES on) resets only the peel tiles its predecessor touched and
// marches only where this draw or the one that last wrote its target touched.  The history is dropped whenever something else changes what
// the march target holds; tiled_draws = consecutive tiled draws since then (saturates at 2).
//
// Two peel images (tsdf_ctx::d_peels / d_peels_alt) alternate per tiled draw while the lanes are on: the one the coming draw uses was last
// written two draws ago, so its touched tiles -- in the OLDEST mask -- can be reset on the lane ahead (a block range of the brick marking
// launch, k_mark_bricks) instead of by a launch of its own on the context's stream: 12 + 6 us of the lane that bounds the frame.  With the
// lanes off the one image is reset by the classify launch of integrate() (part C of k_classify_lists), from the previous draw's mask.  Either
// way peels_cleared tells the coming draw that its reset has been done.  A change of that mode starts a new history.
//
// Two pyramids (tsdf_ctx::atlas_color / atlas_depth) alternate per draw while stage overlap is on: the march of frame f + 1 writes level 0
// of the OTHER one while the hole filling of frame f still reads this one (the reference's m_view_inpaint / m_view_inpaint2, for another
// reason: it swaps them between its transfer passes, recon_integration.cpp:279-338).  The draw that last wrote this draw's target is then
// the one before the previous, and a target is trusted one tiled draw later.
//
// Hole filling by dirty tiles (k_inpaint.hip): the hole filling of a draw may keep to the tiles of this draw and the two before once three
// tiled draws in a row have left nothing else in the pyramid it fills (draw_masks_valid), and only while nothing but the hole filling has
// written the framebuffer since it last held the plain, cleared picture (fb_consistent): background wherever no tile was dirty.
//
// The texture view (tsdf_draw_textures) shows the atlas the latest hole filling completed (GL's unit 15, tex_atlas_ok) and the depth-limit
// image of the latest draw with space skipping (unit 16, tex_limits_ok) -- each until something rewrites it.
#pragma once
#include <algorithm>

namespace rr {

struct ImageTiles {
  // configuration, read when the view is set up
  bool use_history = true;        // RR_IMAGE_TILES=0 turns the history off (A/B)
  bool fill_tiles = true;         // RR_FILL_TILES=0: the hole filling goes through every tile (A/B and test hook)
  // state (abi.cpp goes through the transitions below)
  int touched_idx = 0; bool tile_history = false; int tiled_draws = 0;
  bool last_alt_peels = false;    // the latest draw with space skipping alternated the peel images
  bool peels_cleared = false;     // the peel tiles the coming draw would reset have been reset already
  bool draw_masks_valid = false, fb_consistent = false;
  bool tex_atlas_ok = false, tex_limits_ok = false;

  // a new view size (or none): every image the state speaks of is gone
  void reset() {
    last_alt_peels = false;
    draw_masks_valid = false; fb_consistent = false; tex_atlas_ok = false; tex_limits_ok = false;
    tile_history = false; touched_idx = 0;
  }

  // The peel reset of the coming draw, riding on a launch in front of it; `can` = everything the caller knows (lane, flags, the image exists).
  // Returns the mask whose tiles to reset, or -1 for no reset.
  // ... on the lane ahead (tsdf_mark_bricks), in the ALT image: the tiles of the draw before the previous one
  int peel_reset_ahead(bool can) {
    if (!(can && use_history && tile_history && last_alt_peels)) return -1;
    peels_cleared = true;
    return (touched_idx + 1) % 3;
  }
  // ... on the classify launch (tsdf_integrate), in the one image: the previous draw's tiles.  Unit 16's image is no longer that draw's
  int peel_reset_classify(bool can) {
    if (!(can && use_history && tile_history && !last_alt_peels)) return -1;
    tex_limits_ok = false;
    peels_cleared = true;
    return (touched_idx + 2) % 3;
  }

  // One draw, first half: the depth limits.  lanes = the lanes are on and the second peel image exists
  struct Limits {
    bool use_tiles;               // this draw takes part in the tile history
    bool alt_peels;               // ... and alternates the peel images
    bool start_history;           // first: zero the three masks and, with alt_peels, clear the other peel image
    bool swap_peels;              // then: swap the peel images (the image of the draw before the previous one: its tiles are in the oldest mask)
    int touched_cur, touched_prev;   // the masks the depth limits write / reset by (-1: none)
    int already_cleared;          // the reset by touched_prev has been done (peel_reset_*)
  };
  Limits draw_limits(bool skip, bool shifted, bool masked_direct, bool lanes) {
    Limits L{};
    L.use_tiles = skip && use_history && !shifted && !masked_direct;
    L.touched_cur = L.touched_prev = -1;
    if (skip) {
      L.alt_peels = L.use_tiles && lanes;
      if (L.alt_peels != last_alt_peels) tile_history = false;   // a change of that mode starts a new tile history
      if (L.use_tiles && !tile_history) { L.start_history = true; peels_cleared = false; }
      L.swap_peels = L.alt_peels && tile_history;
      last_alt_peels = L.alt_peels;
      if (L.use_tiles) L.touched_cur = touched_idx;
      if (L.use_tiles && tile_history) { L.touched_prev = (touched_idx + (L.alt_peels ? 1 : 2)) % 3; L.already_cleared = peels_cleared ? 1 : 0; }
      tex_limits_ok = true;                                       // drawDepthLimits() rewrote m_view_depth (unit 16)
    }
    peels_cleared = false;                                        // consumed (or void: this draw did its own reset)
    return L;
  }

  // ... between the halves: the draw takes the other pyramid while stage overlap is on,
  static bool two_pyramids(bool fill_holes, bool stage_overlap, bool masked_direct) { return fill_holes && stage_overlap && !masked_direct; }
  // and one allocated just now holds nothing of any draw (the depth limits above still went by the history)
  void second_pyramid_allocated() { tile_history = false; }

  // ... second half: the march.  use_tiles = Limits::use_tiles, partial = a slab context
  struct March {
    int touched_cur, touched_prev, touched_prev_target, touched_recycle;   // RayTarget's four masks (-1 without use_tiles)
    int rewrite_all, rewrite_target;   // no valid history for the sample counts / for the target
    bool fill_mask;               // the march leaves the tile mask of this draw's hole filling
  };
  March draw_march(bool use_tiles, bool two_pyramids, bool fill_holes, bool masked_direct, bool partial) {
    March M{};
    M.touched_cur = M.touched_prev = M.touched_prev_target = M.touched_recycle = -1;
    if (!tile_history) tiled_draws = 0;
    if (use_tiles) {
      const int cur = touched_idx, prev = (cur + 2) % 3, oldest = (cur + 1) % 3;
      M.touched_cur = cur; M.touched_prev = prev;
      M.touched_prev_target = two_pyramids ? oldest : prev;
      M.touched_recycle = oldest;
      M.rewrite_all = tiled_draws >= 1 ? 0 : 1;
      M.rewrite_target = tiled_draws >= (two_pyramids ? 2 : 1) ? 0 : 1;
      // the hole filling of this draw may keep to the tiles of this draw and the two before, once three tiled draws in a row have left
      // nothing else in the pyramid it fills and in the framebuffer
      M.fill_mask = fill_holes;
      draw_masks_valid = fill_holes && tiled_draws >= 2 && !partial;
      touched_idx = (cur + 1) % 3;
      tile_history = true;
      tiled_draws = std::min(2, tiled_draws + 1);
    } else { tile_history = false; draw_masks_valid = false; }
    if (!fill_holes) fb_consistent = false;                       // the march (or the masked merge) writes the framebuffer itself
    if (fill_holes || masked_direct) tex_atlas_ok = false;        // level 0 of the atlas: this march's until its hole filling completes the pyramid
    return M;
  }

  // the hole filling: true = it may keep to the dirty tiles
  bool fill(bool colour_mask, bool colour_kept) {
    const bool plain = !colour_mask && !colour_kept;
    const bool by_tiles = fill_tiles && draw_masks_valid && fb_consistent && plain;
    fb_consistent = plain;                                        // the framebuffer is this pass's now: background wherever no tile was dirty
    draw_masks_valid = false;                                     // (consumed: a second fillColors() of the same draw, e.g. after a composite, goes through every tile)
    tex_atlas_ok = true;                                          // the texture bound on unit 15 at recon_integration.cpp:315
    return by_tiles;
  }

  // someone else writes the framebuffer (the point / triangle draws, the overlays, an upload): the hole filling may no longer keep to the dirty tiles
  void framebuffer_written() { fb_consistent = false; }
  // the march target overwritten from outside (tsdf_upload_image): it no longer holds what the last march left
  void target_uploaded(bool target_is_atlas) {
    tile_history = false; draw_masks_valid = false;
    if (target_is_atlas) tex_atlas_ok = false;
  }
  // the march target composited (slab contexts): the composite writes every pixel of it, so this draw's hole filling goes through every
  // tile.  The history stays: a tile without a brick under it holds clear values after the march AND after a composite into this target --
  // the brick tables are replicated, so no rank can hit there
  void target_composited(bool target_is_atlas) {
    draw_masks_valid = false;
    if (target_is_atlas) tex_atlas_ok = false;
  }
  // a setter changed what the march targets hold or where the march puts it
  void drop_history() { tile_history = false; }

  // what the texture view may show
  bool atlas_complete() const { return tex_atlas_ok; }
  bool limits_complete() const { return tex_limits_ok; }
};

}  // namespace rr
