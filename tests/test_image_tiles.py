"""csrc/image_tiles.hpp: the view's dirty-tile bookkeeping as one state machine, for every combination of its state fields
(3 x 2 x 3 x 2 x 2 x 2 x 2 x 2 x 2) and its two configuration booleans, every event, and every combination of the event's boolean inputs,
against a restatement of the statements abi.cpp held at each of those places before the header existed.  Then a breadth-first walk from
the reset state: what the protocol promises on every state the events can reach.  The header is host-only and free of HIP, so a plain g++
builds the table; the 2.5 million rows come as bytes and are compared column-wise with numpy (the full product, not the reachable part)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbd-recon_amd", "csrc")

STATE = ("touched_idx", "tile_history", "tiled_draws", "last_alt_peels", "peels_cleared", "draw_masks_valid", "fb_consistent", "tex_atlas_ok", "tex_limits_ok")
RADIX = (3, 2, 3, 2, 2, 2, 2, 2, 2)
N_STATES = int(np.prod(RADIX))
# events, the number of boolean inputs of each, and the names of what each hands back
RESET, PEEL_AHEAD, PEEL_CLASSIFY, DRAW, FILL, FB_WRITTEN, UPLOADED, COMPOSITED, DROP, QUERY = range(10)
N_INPUTS = {RESET: 0, PEEL_AHEAD: 1, PEEL_CLASSIFY: 1, DRAW: 8, FILL: 2, FB_WRITTEN: 0, UPLOADED: 1, COMPOSITED: 1, DROP: 0, QUERY: 0}
DRAW_OUT = ("use_tiles", "alt_peels", "start_history", "swap_peels", "limits_cur", "limits_prev", "already_cleared", "two_pyramids",
            "cur", "prev", "prev_target", "recycle", "rewrite_all", "rewrite_target", "fill_mask")
ROWS_PER_STATE = sum(1 << n for n in N_INPUTS.values())
# one row: event, the two configuration booleans, the state, 8 inputs, the next state, up to 15 returned values; -1 travels as 255
COLS = 3 + 9 + 8 + 9 + 15
NONE = 255

PROGRAM = r"""
#include <cstdio>
#include "image_tiles.hpp"
using rr::ImageTiles;
static unsigned char row[3 + 9 + 8 + 9 + 15];
static void put_state(const ImageTiles& T, unsigned char* p) {
  p[0] = (unsigned char)T.touched_idx; p[1] = T.tile_history; p[2] = (unsigned char)T.tiled_draws; p[3] = T.last_alt_peels; p[4] = T.peels_cleared;
  p[5] = T.draw_masks_valid; p[6] = T.fb_consistent; p[7] = T.tex_atlas_ok; p[8] = T.tex_limits_ok;
}
int main() {
  for (int uh = 0; uh < 2; ++uh) for (int ft = 0; ft < 2; ++ft)
  for (int idx = 0; idx < 3; ++idx) for (int hist = 0; hist < 2; ++hist) for (int td = 0; td < 3; ++td) for (int alt = 0; alt < 2; ++alt) for (int pc = 0; pc < 2; ++pc)
  for (int mv = 0; mv < 2; ++mv) for (int fb = 0; fb < 2; ++fb) for (int ta = 0; ta < 2; ++ta) for (int tl = 0; tl < 2; ++tl) {
    ImageTiles S;
    S.use_history = uh; S.fill_tiles = ft;
    S.touched_idx = idx; S.tile_history = hist; S.tiled_draws = td; S.last_alt_peels = alt; S.peels_cleared = pc;
    S.draw_masks_valid = mv; S.fb_consistent = fb; S.tex_atlas_ok = ta; S.tex_limits_ok = tl;
    const int n_inputs[10] = {0, 1, 1, 8, 2, 0, 1, 1, 0, 0};
    for (int ev = 0; ev < 10; ++ev) for (int in = 0; in < (1 << n_inputs[ev]); ++in) {
      ImageTiles T = S;
      for (unsigned char& b : row) b = 0;
      row[0] = (unsigned char)ev; row[1] = (unsigned char)uh; row[2] = (unsigned char)ft;
      put_state(S, row + 3);
      bool i[8];
      for (int k = 0; k < 8; ++k) { i[k] = (in >> k) & 1; row[12 + k] = i[k]; }
      unsigned char* out = row + 29;
      switch (ev) {
        case 0: T.reset(); break;
        case 1: out[0] = (unsigned char)T.peel_reset_ahead(i[0]); break;
        case 2: out[0] = (unsigned char)T.peel_reset_classify(i[0]); break;
        case 3: {   // inputs: space skipping, shifted viewport, masked-direct, lanes on, colour filling, stage overlap, second pyramid newly allocated, slab context
          const ImageTiles::Limits L = T.draw_limits(i[0], i[1], i[2], i[3]);
          const bool two = ImageTiles::two_pyramids(i[4], i[5], i[2]);
          if (two && i[6]) T.second_pyramid_allocated();
          const ImageTiles::March M = T.draw_march(L.use_tiles, two, i[4], i[2], i[7]);
          const int v[15] = {L.use_tiles, L.alt_peels, L.start_history, L.swap_peels, L.touched_cur, L.touched_prev, L.already_cleared, two,
                             M.touched_cur, M.touched_prev, M.touched_prev_target, M.touched_recycle, M.rewrite_all, M.rewrite_target, M.fill_mask};
          for (int k = 0; k < 15; ++k) out[k] = (unsigned char)v[k];
          break;
        }
        case 4: out[0] = T.fill(i[0], i[1]); break;
        case 5: T.framebuffer_written(); break;
        case 6: T.target_uploaded(i[0]); break;
        case 7: T.target_composited(i[0]); break;
        case 8: T.drop_history(); break;
        default: out[0] = T.atlas_complete(); out[1] = T.limits_complete(); break;
      }
      if (T.use_history != S.use_history || T.fill_tiles != S.fill_tiles) return 1;   // no event touches the configuration
      put_state(T, row + 20);
      std::fwrite(row, 1, sizeof(row), stdout);
    }
  }
  return 0;
}
"""


class Rows:
    """the table's columns by name; integer columns stay uint8 (255 = -1), boolean ones become bool"""

    def __init__(self, raw):
        self.raw = raw
        self.event, self.use_history, self.fill_tiles = raw[:, 0], raw[:, 1].astype(bool), raw[:, 2].astype(bool)
        self.inputs = [raw[:, 12 + k].astype(bool) for k in range(8)]
        self.out = raw[:, 29:]

    def state(self, next_state=False):
        cols = self.raw[:, 20:29] if next_state else self.raw[:, 3:12]
        return {n: (cols[:, k].astype(np.int64) if n in ("touched_idx", "tiled_draws") else cols[:, k].astype(bool)) for k, n in enumerate(STATE)}

    def of(self, event):
        return Rows(self.raw[self.event == event])


def index_of(state):
    ix = np.zeros(len(state["touched_idx"]), np.int64)
    for n, r in zip(STATE, RADIX):
        ix = ix * r + state[n].astype(np.int64)
    return ix


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    d = tmp_path_factory.mktemp("image_tiles")
    src, exe, dump = str(d / "tiles_table.cpp"), str(d / "tiles_table"), str(d / "table.bin")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src, "-o", exe])
    with open(dump, "wb") as f:
        subprocess.check_call([exe], stdout=f)
    raw = np.fromfile(dump, np.uint8).reshape(-1, COLS)
    os.remove(dump)
    assert len(raw) == 4 * N_STATES * ROWS_PER_STATE
    return Rows(raw)


def put(cond, old, new):
    """`if (cond) field = new;` for every row at once"""
    return np.where(cond, new, old)


# ---- abi.cpp as it stood, one function per site; c = the nine fields (and the two knobs) of tsdf_ctx, every row at once
def old_reset(c, i, R):
    """release_view / setup_view"""
    c["last_alt_peels"] = put(True, c["last_alt_peels"], False)
    for n in ("draw_masks_valid", "fb_consistent", "tex_atlas_ok", "tex_limits_ok", "tile_history"):
        c[n] = put(True, c[n], False)
    c["touched_idx"] = put(True, c["touched_idx"], 0)
    return []


def old_mark_bricks(c, i, R):
    """tsdf_mark_bricks; i[0] = lane != c->stream && c->use_bricks && c->skip_space && c->d_peels_alt"""
    take = i[0] & R.use_history & c["tile_history"] & c["last_alt_peels"]
    mask = put(take, -1, (c["touched_idx"] + 1) % 3)          # pc.touched_prev = c->d_touched[(c->touched_idx + 1) % 3]
    c["peels_cleared"] = put(take, c["peels_cleared"], True)
    return [mask]


def old_integrate(c, i, R):
    """tsdf_integrate; i[0] = !deep && !pipelined(c) && c->use_bricks && !c->full_classify && c->skip_space && whole && c->d_peels"""
    take = i[0] & R.use_history & c["tile_history"] & ~c["last_alt_peels"]
    mask = put(take, -1, (c["touched_idx"] + 2) % 3)
    c["tex_limits_ok"] = put(take, c["tex_limits_ok"], False)
    c["peels_cleared"] = put(take, c["peels_cleared"], True)
    return [mask]


def old_raymarch(c, i, R):
    """raymarch_impl, top to bottom"""
    skip, shifted, masked_direct, lanes, fill_holes, overlap_fill, new_pyramid, partial = i
    use_tiles = skip & R.use_history & ~shifted & ~masked_direct
    # if (P.skip) {
    alt_peels = use_tiles & lanes                                                        # use_tiles && pipelined(c) && c->d_peels_alt
    c["tile_history"] = put(skip & (alt_peels != c["last_alt_peels"]), c["tile_history"], False)
    start = skip & use_tiles & ~c["tile_history"]                                        # the memsets, the clear of the other peel image
    c["peels_cleared"] = put(start, c["peels_cleared"], False)
    swap = skip & alt_peels & c["tile_history"]                                          # std::swap(c->d_peels, c->d_peels_alt)
    c["last_alt_peels"] = put(skip, c["last_alt_peels"], alt_peels)
    limits_cur = put(skip & use_tiles, -1, c["touched_idx"])
    limits_prev = put(skip & use_tiles & c["tile_history"], -1, (c["touched_idx"] + np.where(alt_peels, 1, 2)) % 3)
    already = skip & use_tiles & c["tile_history"] & c["peels_cleared"]
    c["tex_limits_ok"] = put(skip, c["tex_limits_ok"], True)
    # }
    c["peels_cleared"] = put(True, c["peels_cleared"], False)
    two_pyramids = fill_holes & overlap_fill & ~masked_direct
    c["tile_history"] = put(two_pyramids & new_pyramid, c["tile_history"], False)       # if (!c->atlas_color[p]) { ... c->tile_history = false; }
    c["tiled_draws"] = put(~c["tile_history"], c["tiled_draws"], 0)
    # if (use_tiles) {
    cur = c["touched_idx"]; prev = (cur + 2) % 3; oldest = (cur + 1) % 3
    rt = [put(use_tiles, -1, cur), put(use_tiles, -1, prev), put(use_tiles, -1, np.where(two_pyramids, oldest, prev)), put(use_tiles, -1, oldest)]
    rewrite_all = put(use_tiles, 0, np.where(c["tiled_draws"] >= 1, 0, 1))              # (RayTarget R{}: 0 without tiles)
    rewrite_target = put(use_tiles, 0, np.where(c["tiled_draws"] >= np.where(two_pyramids, 2, 1), 0, 1))
    fill_mask = use_tiles & fill_holes
    c["draw_masks_valid"] = put(use_tiles, c["draw_masks_valid"], fill_holes & (c["tiled_draws"] >= 2) & ~partial)
    c["touched_idx"] = put(use_tiles, c["touched_idx"], (cur + 1) % 3)
    c["tile_history"] = put(use_tiles, c["tile_history"], True)
    c["tiled_draws"] = put(use_tiles, c["tiled_draws"], np.minimum(2, c["tiled_draws"] + 1))
    # } else {
    c["tile_history"] = put(~use_tiles, c["tile_history"], False)
    c["draw_masks_valid"] = put(~use_tiles, c["draw_masks_valid"], False)
    # }
    c["fb_consistent"] = put(~fill_holes, c["fb_consistent"], False)
    c["tex_atlas_ok"] = put(fill_holes | masked_direct, c["tex_atlas_ok"], False)
    return [use_tiles, alt_peels & skip, start, swap, limits_cur, limits_prev, already, two_pyramids] + rt + [rewrite_all, rewrite_target, fill_mask]


def old_fill_colors(c, i, R):
    """fill_colors_impl; i = (c->color_mask_mode != 0, c->keep_color)"""
    plain = ~i[0] & ~i[1]
    by_tiles = R.fill_tiles & c["draw_masks_valid"] & c["fb_consistent"] & plain
    c["fb_consistent"] = put(True, c["fb_consistent"], plain)
    c["draw_masks_valid"] = put(True, c["draw_masks_valid"], False)
    c["tex_atlas_ok"] = put(True, c["tex_atlas_ok"], True)
    return [by_tiles]


def old_foreign_draw(c, i, R):
    """the nine draw calls and tsdf_upload_framebuffer"""
    c["fb_consistent"] = put(True, c["fb_consistent"], False)
    return []


def old_upload_image(c, i, R):
    """tsdf_upload_image; i[0] = c->fill_holes || masked_direct(c)"""
    c["tile_history"] = put(True, c["tile_history"], False)
    c["draw_masks_valid"] = put(True, c["draw_masks_valid"], False)
    c["tex_atlas_ok"] = put(i[0], c["tex_atlas_ok"], False)
    return []


def old_composite(c, i, R):
    """tsdf_composite_dev, tsdf_composite_hits_dev; i[0] = c->fill_holes || masked_direct(c)"""
    c["draw_masks_valid"] = put(True, c["draw_masks_valid"], False)
    c["tex_atlas_ok"] = put(i[0], c["tex_atlas_ok"], False)
    return []


def old_setter(c, i, R):
    """colour filling, viewport offset / origin, colour mask mode, framebuffer clear, march cap, tsdf_set_stage_overlap"""
    c["tile_history"] = put(True, c["tile_history"], False)
    return []


def old_draw_textures(c, i, R):
    """tsdf_draw_textures: unit 15, unit 16"""
    return [c["tex_atlas_ok"], c["tex_limits_ok"]]


OLD = {RESET: old_reset, PEEL_AHEAD: old_mark_bricks, PEEL_CLASSIFY: old_integrate, DRAW: old_raymarch, FILL: old_fill_colors, FB_WRITTEN: old_foreign_draw,
       UPLOADED: old_upload_image, COMPOSITED: old_composite, DROP: old_setter, QUERY: old_draw_textures}


@pytest.mark.parametrize("event", sorted(OLD))
def test_every_transition_is_abi_cpp_as_it_stood(table, event):
    R = table.of(event)
    assert len(R.raw) == 4 * N_STATES * (1 << N_INPUTS[event])
    c = R.state()
    key = (index_of(c) * 4 + R.raw[:, 1] * 2 + R.raw[:, 2]) * 256 + sum(R.inputs[k].astype(np.int64) << k for k in range(8))
    assert len(np.unique(key)) == len(key)                               # every combination once
    want = OLD[event](c, R.inputs, R)
    got = R.state(next_state=True)
    for n in STATE:
        bad = np.flatnonzero(np.asarray(c[n]).astype(np.int64) != got[n].astype(np.int64))
        assert bad.size == 0, (n, R.raw[bad[0]].tolist())
    for k in range(COLS - 29):
        w = np.asarray(want[k]).astype(np.int64) if k < len(want) else np.zeros(len(R.raw), np.int64)
        bad = np.flatnonzero((w & 255) != R.out[:, k])
        assert bad.size == 0, (event, "returned value", k, R.raw[bad[0]].tolist())


def test_what_only_one_event_may_raise(table):
    """over every state: the framebuffer becomes consistent and the atlas complete by a hole filling alone; the masks become valid, the
    depth-limit image complete and a history begins by a draw alone; only the two peel resets announce a reset"""
    before, after = table.state(), table.state(next_state=True)
    for field, events in (("fb_consistent", (FILL,)), ("tex_atlas_ok", (FILL,)), ("draw_masks_valid", (DRAW,)), ("tex_limits_ok", (DRAW,)),
                          ("tile_history", (DRAW,)), ("peels_cleared", (PEEL_AHEAD, PEEL_CLASSIFY))):
        raised = after[field] & ~before[field]
        assert not (raised & ~np.isin(table.event, events)).any(), field
    assert not (after["tiled_draws"] > before["tiled_draws"])[table.event != DRAW].any()
    assert (table.raw[table.event == QUERY][:, 3:12] == table.raw[table.event == QUERY][:, 20:29]).all()   # the queries change nothing


def test_invariants_on_the_reachable_states(table):
    """breadth-first from the reset state, every event with every input (more than any caller can do: the inputs are not independent of
    each other in abi.cpp, so what holds here holds there)"""
    raw = table.raw.reshape(4, N_STATES, ROWS_PER_STATE, COLS)
    first = {}
    k = 0
    for ev in range(10):
        first[ev] = k
        k += 1 << N_INPUTS[ev]
    seen_by_tiles = 0
    for cfg in range(4):
        use_history, fill_tiles = cfg >> 1, cfg & 1
        T = raw[cfg]
        assert (T[:, :, 1] == use_history).all() and (T[:, :, 2] == fill_tiles).all()
        flat = Rows(T.reshape(-1, COLS))
        assert (index_of(flat.state()).reshape(N_STATES, ROWS_PER_STATE) == np.arange(N_STATES)[:, None]).all()
        nxt = index_of(flat.state(next_state=True)).reshape(N_STATES, ROWS_PER_STATE)
        reach = np.zeros(N_STATES, bool)
        reach[nxt[0, first[RESET]]] = True                                # reset of a context just created: every field at its default
        assert nxt[0, first[RESET]] == 0
        frontier = np.array([0])
        while frontier.size:
            new = np.unique(nxt[frontier])
            new = new[~reach[new]]
            reach[new] = True
            frontier = new
        assert 1 < reach.sum() < N_STATES
        S = Rows(T[reach].reshape(-1, COLS))
        st = S.state()
        # the masks are valid only with a history of at least two tiled draws behind the draw that left them
        assert (st["tiled_draws"][st["draw_masks_valid"]] == 2).all()
        assert (st["tiled_draws"] <= 2).all()
        # by tiles: never with an inconsistent framebuffer, a colour mask, an uncleared colour buffer, invalid masks or RR_FILL_TILES=0
        F = S.of(FILL)
        fs = F.state()
        by_tiles = F.out[:, 0].astype(bool)
        assert not (by_tiles & ~(fs["fb_consistent"] & ~F.inputs[0] & ~F.inputs[1] & fs["draw_masks_valid"] & F.fill_tiles)).any()
        assert not (by_tiles & ~fill_tiles).any() and not (by_tiles & ~use_history).any()
        seen_by_tiles += by_tiles.sum()
        # ... and a hole filling right behind a foreign write of the framebuffer goes through every tile
        W = S.of(FB_WRITTEN)
        after_write = index_of(W.state(next_state=True))
        fill_rows = T[after_write][:, first[FILL]:first[FILL] + 4]
        assert (fill_rows[:, :, 0] == FILL).all() and not fill_rows[:, :, 29].any()
        # without RR_IMAGE_TILES no history, no masks, no reset announced
        if not use_history:
            assert not st["tile_history"].any() and not st["draw_masks_valid"].any() and not st["peels_cleared"].any()
        # a draw: the three masks in their three roles, the rotation, the depth limits and the march agree
        D = S.of(DRAW)
        o = {n: D.out[:, k].astype(np.int64) for k, n in enumerate(DRAW_OUT)}
        ds, ds2 = D.state(), D.state(next_state=True)
        t = o["use_tiles"].astype(bool)
        assert (np.sort(np.stack([o["cur"], o["prev"], o["recycle"]], 1)[t], axis=1) == [0, 1, 2]).all()
        assert (o["prev_target"][t] == np.where(o["two_pyramids"], o["recycle"], o["prev"])[t]).all()
        assert (o["cur"][t] == o["limits_cur"][t]).all() and (ds2["touched_idx"][t] == (o["cur"][t] + 1) % 3).all()
        assert (ds2["touched_idx"][~t] == ds["touched_idx"][~t]).all()
        for n in ("cur", "prev", "prev_target", "recycle", "limits_cur", "limits_prev"):
            assert (o[n][~t] == NONE).all()
        assert (ds2["tile_history"] == t).all()                          # a history exists exactly behind a tiled draw
        assert not (o["rewrite_target"] == 0)[o["rewrite_all"] == 1].any()   # a target is trusted no sooner than the sample counts
        assert (o["rewrite_all"][o["start_history"] == 1] == 1).all()    # a new history rewrites everything
        assert (o["limits_prev"][(o["rewrite_all"] == 0) & t] != NONE).all()
        assert (o["limits_prev"][o["already_cleared"] == 1] != NONE).all()
        assert not (o["swap_peels"] & o["start_history"]).any()
        assert (ds2["draw_masks_valid"] <= ((o["rewrite_all"] == 0) & (o["rewrite_target"] == 0) & (o["fill_mask"] == 1))).all()
        # a reset announced by one of the two riders is the reset the coming draw's depth limits would have done: same mask
        for ev in (PEEL_AHEAD, PEEL_CLASSIFY):
            P = S.of(ev)
            did = P.out[:, 0] != NONE
            assert P.state()["tile_history"][did].all()                   # ... and announced under a live history only
            draws = T[index_of(P.state(next_state=True))[did]][:, first[DRAW]:first[DRAW] + 256]
            mask = np.broadcast_to(P.out[did, 0][:, None], draws.shape[:2])
            announced = draws[:, :, 29 + DRAW_OUT.index("already_cleared")] == 1
            assert announced.any() or not did.any()
            assert (draws[:, :, 29 + DRAW_OUT.index("limits_prev")][announced] == mask[announced]).all()
            assert (draws[:, :, 29 + DRAW_OUT.index("alt_peels")][announced] == (ev == PEEL_AHEAD)).all()
    assert seen_by_tiles > 0
