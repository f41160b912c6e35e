"""Inputs, the cut chain and the acceptance rule of the hole-filling tests, shared by tests/test_fill_reference.py (the oracle against
tests/fill_reference.py, no GPU) and tests/test_gpu_fill_reference.py (kernels and oracle against it).  HIP-free.

The chain is cut, as in the pre-processing judge: level l + 1 of a candidate's atlas is judged against inpaint_level(transfer(T_l), l),
where T_l is a cleared atlas holding the candidate's OWN levels 0 .. l, and the framebuffer against colorfill() of the candidate's own
finished atlas.  Every level and the pull are judged alone, so an excluded pixel taints nothing downstream, and a level the dirty-tile
path did not touch at all is judged like any other.  Level 0 must equal the uploaded image bit for bit, and whatever lies outside the
level rectangles the clear value.

Acceptance rule (compare() of tests/main_path_cases.py): an element is excluded only where the reference's own margin says so -- a
truncation on which fp32 and exact arithmetic disagree, a valid sample within `bound` of the mean depth of its window, a read past the
level tables; every other element must agree within the tolerance; at most 5 % of a level's pixels and of a case's framebuffer pixels may
be excluded; minimum counts stop a case from passing empty.

What was measured on the CPU, oracle against reference, over all_cpu_cases() (print_measurements() repeats it); the kernel is held to the
same numbers, they are never measured on it:
#   dev       largest deviation on non-excluded elements               -> tol = 4 x dev, rounded up
#   need      largest mean-depth margin of a pixel on which the oracle is off by more than the tolerance ("decides otherwise")
#   excluded  largest share of excluded elements of any level / framebuffer of any case
# quantity      dev        need       excluded
# pyr_colour    1.53e-7    --         4.14 %     a level's rgba; the excluded share is level 1 of 1280 x 720: pixels of the 14 inpaint coordinates
# pyr_depth     1.70e-7    --         4.14 %       on which fp32 and exact arithmetic truncate differently, and mean-depth margins under the bound
# fb_colour     4.70e-5    --         1.09 %     the bilinear pull at atlas coordinates up to 1920: ulp(1920) = 1.2e-4 of a texel in fp32
# depth_mean    --         9.31e-8    3.89 %     -> bound = 4 x need; fp32 error of a mean of 16 depths around 0.5: about 2e-7
No size had to change its content to stay under the cap but for what image() says about the columns and rows on which fp32 truncates
w * (x / w) to x - 1: 6 of 61 columns, 9 of 173 columns and 8 of 99 rows, 34 of 720 rows -- with independent content in them the
framebuffer of 61 x 45 alone would have had 8.2 % of its pixels excluded, that of 173 x 99 12.3 %.  In those columns and rows the cases
cannot tell x from x - 1: that the oracle reads x - 1 is pinned at 61 x 45 in x (tests/test_oracle_inpaint.py); for the kernel, for y and
for the other sizes it rests on the bit-equality tests of kernel and oracle (tests/test_gpu_round3.py, test_gpu_configs.py).
"""
import functools
import hashlib

import numpy as np

import fill_reference as R
import main_path_cases as M
from main_path_cases import close_abs, compare, deviation   # noqa: F401  (one rule, one implementation)
from helpers import tiny_scene
import rgbd_recon_amd as rr
from oracle.oracle import OracleRecon

S = rr.scene
f32 = np.float32

TABLE = {
    "pyr_colour": dict(tol=7e-7, cap=0.05),
    "pyr_depth":  dict(tol=7e-7, cap=0.05),
    "fb_colour":  dict(tol=1.9e-4, cap=0.05),
    "depth_mean": dict(bound=4e-7),
}
CAP = 0.05


def close(tol):
    """close_abs, and equal infinities agree too"""
    inner = close_abs(tol)

    def f(a, b):
        return inner(a, b) | (np.asarray(a, np.float64) == b)
    f.tolerance = True
    return f


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.view(np.uint32) == b.view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- inputs
HOLE_WIDTHS = (1, 2, 5, 12, 40, 100)            # 100: the width at which the level search of 1280 x 720 ends at level 5


@functools.lru_cache(maxsize=None)
def image(w, h, seed=1, widest=40):
    """(rgba [h][w][4], depth [h][w]) fp32: a tilted depth ramp with a second, nearer surface in stripes and a blob and per-pixel noise of
    +-2e-3 (three orders above the mean-depth bound: means do not tie); background (0, 1, 0, 0) at depth 1 in two corners and along part of
    every border; holes (alpha -1, surface depth) of the widths of HOLE_WIDTHS up to `widest`, touching all four borders; texels of alpha
    exactly 0 under depth < 1 and of tiny positive alpha; NaN in the colour of valid texels and of hole texels, +inf in that of hole
    texels alone (the filling never reads a hole's colour: an infinity there must not leak)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    depth = 0.35 + 0.3 * x / w + 0.2 * y / h
    near = (((x + 2 * y) // max(3, w // 8)) % 3 == 0) | ((x - 0.6 * w) ** 2 + (y - 0.4 * h) ** 2 < (0.18 * min(w, h)) ** 2)
    depth = np.where(near, depth - 0.25, depth) + rng.uniform(-2e-3, 2e-3, (h, w))
    rgba = np.concatenate([rng.random((h, w, 3)), np.ones((h, w, 1))], -1)
    rgba[near, :3] = 0.25 + 0.5 * rgba[near, :3]
    hole = np.zeros((h, w), bool)
    if widest >= 1 and w >= 8:
        hole[:, w // 3] = True                                     # width 1, top border to bottom border
        hole |= rng.random((h, w)) < 0.01
    if widest >= 2 and h >= 12:
        hole[h // 2:h // 2 + 2, :] = True                          # width 2, left border to right border
    if widest >= 5 and min(w, h) >= 24:
        hole[h // 5:h // 5 + 5, w - 5:] = True                     # 5 x 5 at the right border
        hole[:5, w // 2:w // 2 + 5] = True                         # ... and at the top
    if widest >= 12 and min(w, h) >= 45:
        hole[h - 12:, w // 2:w // 2 + 12] = True                   # 12 x 12 at the bottom border
    if widest >= 40 and min(w, h) >= 96:
        hole[h // 3:h // 3 + 40, :40] = True                       # 40 x 40 at the left border
    if widest >= 100 and min(w, h) >= 400:
        hole[h // 2 + 40:h // 2 + 140, w // 2:w // 2 + 100] = True # 100 x 100 inside
    rgba[hole] = (9.0, 9.0, 9.0, -1.0)
    zero_alpha = (rng.random((h, w)) < 0.004) & ~hole
    rgba[zero_alpha, 3] = 0.0                                      # alpha exactly 0, depth < 1: a hole like any other
    tiny_alpha = (rng.random((h, w)) < 0.004) & ~hole & ~zero_alpha
    rgba[tiny_alpha, 3] = 1e-30                                    # > 0: valid
    bg = np.zeros((h, w), bool)
    if w >= 8:
        bg[: h // 4, : w // 5] = True
        bg[h - h // 6:, w - w // 4:] = True
        bg[h // 2 + 3: h // 2 + 3 + max(1, h // 8), w - max(1, w // 16):] = True
        bg[: max(1, h // 16), w // 2 + 6: w // 2 + 6 + w // 8] = True
    rgba[bg] = R.CLEAR_COLOR
    depth[bg] = 1.0
    odd = np.flatnonzero(~bg.ravel())
    pick = rng.choice(odd, size=min(6, max(0, len(odd) // 40)), replace=False) if len(odd) else []
    for k, i in enumerate(pick):
        yy, xx = divmod(int(i), w)
        rgba[yy, xx, k % 3] = np.inf if (k % 2 and rgba[yy, xx, 3] < 0) else np.nan
    t = R.lod_tables(w, h)
    _, _, mx, my = R.colorfill_positions(t, 0)[:4]                 # where w * (x / w) truncates to x - 1 in fp32 (GL leaves the division's rounding
    for c in np.flatnonzero(mx == 0):                              # open) the colour fill of column x may read column x - 1: such a column repeats
        rgba[:, c], depth[:, c] = rgba[:, c - 1], depth[:, c - 1]  # its neighbour here, so that the pixel has one answer and stays judged
    for r in np.flatnonzero(my == 0):
        rgba[r], depth[r] = rgba[r - 1], depth[r - 1]
    out = rgba.astype(f32), depth.astype(f32)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def past_tables_image(w=5, h=3):
    """no level has alpha > 0 anywhere, the surface (depth < 1) is everywhere but at one pixel: the level search runs to num_lods"""
    rgba = np.zeros((h, w, 4), f32)
    rgba[..., 3] = -1.0
    depth = np.full((h, w), 0.5, f32)
    rgba[0, 0] = R.CLEAR_COLOR
    depth[0, 0] = 1.0
    return rgba, depth


def recon_kw(w, h):
    return dict(res=(8, 8, 8), brick_size=[0.5] * 3, limit=0.05, view=(w, h))


def scene():
    return tiny_scene([(0.5, 0.5, 0.5)], [0.5], [1.0], [1.0])


def only_oracle(sc, **kw):
    return {"oracle": OracleRecon(sc, **kw)}


# ---------------------------------------------------------------------------------------------------------------- the judge
_judged = {}


def _key(*arrays):
    d = hashlib.sha1()
    for a in arrays:
        d.update(np.ascontiguousarray(a).tobytes())
    return d.digest()


def level_references(ac, ad, t):
    """the cut chain for one candidate atlas: [inpaint_level(transfer(T_l), l) for l], cached by the atlas' bytes (kernel and oracle
    usually hold the same)"""
    k = ("levels", ac.shape, _key(ac, ad))
    if k not in _judged:
        c64, d64 = ac.astype(np.float64), ad.astype(np.float64)
        T = R.cleared_atlas(t)
        out = []
        for l in range(t["num_lods"] - 1):
            R.place_level(T, t, l, *R.level_of((c64, d64), t, l))
            Sq, sm = R.transfer(T, t)
            out.append(R.inpaint_level(Sq, t, l, sm))
        _judged[k] = out
    return _judged[k]


def fb_reference(ac, ad, t, mask, base):
    k = ("fb", ac.shape, mask, _key(ac, ad, np.zeros(1) if base is None else base))
    if k not in _judged:
        _judged[k] = R.colorfill((ac.astype(np.float64), ad.astype(np.float64)), t, mask, None if base is None else base.astype(np.float64))
    return _judged[k]


def judge(what, side, atlas, fb, level0=None, mask=0, base=None, min_filled=0, fb_only_share=None):
    """one candidate (`side`: 'kernel' / 'oracle' / ...) against the reference of its own levels.  Returns dict(level_excluded, fb_excluded, filled)."""
    ac, ad = atlas
    fc, fd = fb
    h, w = fd.shape
    t = R.lod_tables(w, h)
    assert ac.shape == (h, t["full"][0], 4)
    if level0 is not None:                                         # level 0 is the uploaded image, bit for bit
        assert same_bits(ac[:, :w], level0[0]).all() and same_bits(ad[:, :w], level0[1]).all(), f"{what}: [{side}] level 0 is not the uploaded image"
    outside = np.ones(ad.shape, bool)
    for l in range(t["num_lods"]):
        (ox, oy), (rx, ry) = t["off"][l], t["res"][l]
        outside[oy:oy + ry, ox:ox + rx] = False
    assert (ac[outside] == f32(R.CLEAR_COLOR)).all() and (ad[outside] == 1).all(), f"{what}: [{side}] the atlas outside the levels is not the clear value"
    bound = TABLE["depth_mean"]["bound"]
    shares = []
    for l, ref in enumerate(level_references(ac, ad, t)):
        gc, gd = R.level_of((ac, ad), t, l + 1)
        n = gd.size
        ex = ref["margin"] < bound
        name = f"{what} level {l + 1}"
        kw = dict(minimum=n - int(CAP * n), excluded=ex)
        s, _ = compare("pyr_colour: " + name, ref["rgba"], ref["margin"], bound, CAP, {side: gc}, close(TABLE["pyr_colour"]["tol"]), **kw)
        compare("pyr_depth: " + name, ref["depth"], ref["margin"], bound, CAP, {side: gd}, close(TABLE["pyr_depth"]["tol"]), **kw)
        if M.MEASURE is not None:                                  # the margin of the worst pixel that is off by more than the tolerance
            both = lambda a, b: close(TABLE["pyr_colour"]["tol"])(a[..., :4], b[..., :4]).all(-1) & close(TABLE["pyr_depth"]["tol"])(a[..., 4], b[..., 4])
            compare("depth_mean: " + name, np.concatenate([ref["rgba"], ref["depth"][..., None]], -1), np.where(ref["trunc_ok"], ref["mean_margin"], 0.0), bound, CAP,
                    {side: np.concatenate([gc, gd[..., None]], -1)}, both, excluded=~ref["trunc_ok"])
        shares.append(s)
    ref = fb_reference(ac, ad, t, mask, base)
    ex = ref["margin"] <= 0
    filled = ref["written"] & (ref["level"] >= 1)
    if fb_only_share is not None:                                  # past the tables: only what the reference predicts to be undefined
        assert float(ex.mean()) == fb_only_share, f"{what}: the reference excludes {ex.mean():.2%} of the framebuffer, {fb_only_share:.2%} expected"
        return dict(level_excluded=shares, fb_excluded=float(ex.mean()), filled=int(filled.sum()))
    s, _ = compare("fb_colour: " + what, ref["rgba"], ref["margin"], 0.5, CAP, {side: fc}, close(TABLE["fb_colour"]["tol"]), excluded=ex)
    compare("fb depth: " + what, ref["depth"], ref["margin"], 0.5, CAP, {side: fd}, lambda a, b: a == b, excluded=ex)
    n = int((filled & ~ex).sum())
    levels = np.bincount(ref["level"][filled & ~ex], minlength=t["num_lods"] + 1)
    want = (min_filled,) if np.isscalar(min_filled) else tuple(min_filled)        # per level 1, 2, ...; a single number: level 1
    for l, m in enumerate(want, 1):
        assert levels[l] >= m or M.MEASURE is not None, f"{what}: only {levels[l]} compared pixels whose level search ends at level {l}, {m} wanted"
    return dict(level_excluded=shares, fb_excluded=s, filled=n, levels=levels)


# ---------------------------------------------------------------------------------------------------------------- the cases
# size -> (widest hole, minimums of compared pixels whose level search ends at level 1, 2, ...: about half of what the reference finds).  The pull of a pixel whose search ends at level L reads the tables at L + 1 and
# L + 2: with num_lods = 1 + floor(log2(min(w, h))) levels only holes up to about 2^(num_lods - 4) pixels stay inside them, which is what
# `widest` is chosen by; 5 x 3 has two levels and cannot hold a defined pull at all (its framebuffer carries no hole).
SIZES = {(5, 3): (0, ()), (16, 16): (2, (30,)), (48, 32): (5, (120, 2)), (61, 45): (12, (200, 50)), (173, 99): (40, (400, 500, 400, 120)), (96, 72): (12, (300, 50)),
         (1280, 720): (100, (10000, 1200, 2500, 2000, 1200))}
MASK_SIZE = (61, 45)


def upload_case(make, size, mask=0):
    """set_view_images + fillColors() of image(size); mask 1 / 2: first a fill of another image, then the masked fill over its framebuffer"""
    w, h = size
    widest, min_filled = SIZES[size]
    objs = make(scene(), **recon_kw(w, h))
    img = image(w, h, 1, widest)
    out = {}
    for side, o in objs.items():
        base = None
        if mask:
            o.set_view_images(*image(w, h, 2, widest))
            o.fillColors()
            base = o.framebuffer()[0].copy()
            o.setColorMaskMode(mask)
            o.setFramebufferClear(False)
        o.set_view_images(*img)
        o.fillColors()
        out[side] = judge(f"upload {w}x{h} mask {mask}", side, o.atlas(), o.framebuffer(), img, mask, base, min_filled)
    return out, objs


def past_tables_case(make):
    img = past_tables_image()
    h, w = img[1].shape
    objs = make(scene(), **recon_kw(w, h))
    res = {}
    for side, o in objs.items():
        o.set_view_images(*img)
        o.fillColors()
        res[side] = (o.atlas(), o.framebuffer())
        judge("past the tables", side, *res[side], img, fb_only_share=float((img[1] < 1).mean()))
    return res


SEQ_VIEW = (203, 117)
SEQ_MK = dict(n_streams=3, width=160, height=120, lut_res=24, inv_res=32)
SEQ_EYES = [(0.0, 1.1, 3.0), (1.6, 1.4, 2.4), (-2.2, 0.6, 1.2), (0.2, 3.4, 0.4), (0.0, 1.1, 6.5)]
SEQ_FRAMES = 5                                                     # two full fills, then three by tiles


@functools.lru_cache(maxsize=None)
def sequence_scenes():
    """scene, eyes and frame loop of test_hole_filling_by_dirty_tiles_equals_the_full_pass (tests/test_gpu_round3.py)"""
    return [S.make_scene(**SEQ_MK), S.make_scene(**SEQ_MK, sphere_c=(0.4, 0.7, -0.3), box_c=(-0.5, 1.5, 0.2)), S.make_scene(**SEQ_MK, sphere_c=(-0.3, 1.3, 0.2))]


def sequence_case(make, prepare=None):
    """SEQ_FRAMES frames under a moving camera; the final atlas and framebuffer are judged.  make(scene, **kw) -> {side: object}"""
    scs = sequence_scenes()
    kw = dict(res=(96, 96, 96), brick_size=[2.0 / 12, 2.2 / 12, 2.0 / 12], limit=0.03, view=SEQ_VIEW)
    pr = S.gl_flat(S.perspective(50.0, SEQ_VIEW[0] / SEQ_VIEW[1], 0.1, 200.0))
    mvs = [S.gl_flat(S.look_at(e, (0.0, 1.1, 0.0))) for e in SEQ_EYES]
    objs = make(scs[0], **kw)
    out = {}
    for side, o in objs.items():
        if prepare is not None:
            prepare(side, o)
        for k in range(SEQ_FRAMES):
            o.upload_frame(scs[k % 3])
            o.clearOccupiedBricks(); o.markBricks(); o.updateOccupiedBricks(); o.integrate(); o.drawF(mvs[(k * 2) % 5], pr)
        out[side] = judge("draw sequence", side, o.atlas(), o.framebuffer(), min_filled=20)
    return out, objs


TILE_VIEW = (512, 256)                       # powers of two: no truncation is unsafe; level 3 has 64 x 32 pixels, more than the tail takes: it goes by tiles
TILE_DRAWS = 6
TILE_EYES = [((0.022 * k, 1.1, 2.3), (0.022 * k, 1.1, 0.0)) for k in range(TILE_DRAWS)]   # along -z, square onto the brick faces; 2.8 pixels sideways per draw:
#                                              the dirty tiles of three draws stay tight around the content, yet no tile's content repeats an earlier draw's.
#                                              (Of the steps 0.015 .. 0.03 tried on the CPU, 0.022 is the one at which no pixel of the 32- and 8-pixel levels 6 and 7 has a
#                                              mean-depth margin under the bound: one such pixel is 3 % resp. 12 % of its level, past the 5 % cap.)
TAIL_PIXELS = 1024                           # k_inpaint.hip: levels with at most this many pixels go to the tail, in full


@functools.lru_cache(maxsize=None)
def wall_volume(res, z_surface):
    """fp32 [z][y][x]: solid behind a plane near z = z_surface (normalised) that stays inside one layer of bricks, seen from +z: inside a brick the plane's patch is the brick's whole
    cross-section, so with space skipping the content ends within a pixel of the brick's outline"""
    p = M.R.voxel_positions(res)
    d = 0.5 * (z_surface + 0.05 * (p[..., 0] - 0.5) + 0.03 * (p[..., 1] - 0.5) - p[..., 2])       # tilted a little: depths must not tie (the equal-depth quirk)
    v = np.clip(d, -M.LIMIT, M.LIMIT).astype(f32)
    return np.ascontiguousarray(np.where(d <= -M.LIMIT, -f32(M.LIMIT), v))


def wall_counters(res_bricks, layer):
    """occupied: in brick layer `layer` of z, every second brick of the lowest row (cut by the picture's first rows) and of the row after the next;
    nothing above the middle, so the picture's last rows stay empty"""
    rx, ry, rz = res_bricks
    c = np.zeros((rz, ry, rx), np.uint32)
    c[layer, 0, 0::2] = 25
    c[layer, 2, 1::2] = 25
    return c.reshape(-1)


def level_tile_masks(mask0, t, narrow=False, force_last_row=True):
    """k_inpaint.hip's claim restated: the dirty tiles of levels 1 .. from those of level 0 -- child tile T is dirty if one of the parent tiles
    2T - 1 .. 2T + 2 is (narrow: 2T .. 2T + 1), and from level 3 on the last tile row always.  -> {level: mask} for the levels that go by tiles"""
    out, parent = {}, np.asarray(mask0, bool)
    for lod in range(min(3, t["num_lods"] - 1)):
        rx, ry = t["res"][lod + 1]
        if rx * ry <= TAIL_PIXELS:
            break
        cnx, cny = (rx + 7) // 8, (ry + 7) // 8
        child = np.zeros((cny, cnx), bool)
        lo, hi = (0, 2) if narrow else (-1, 3)
        for ty in range(cny):
            for tx in range(cnx):
                ys = [y for y in range(2 * ty + lo, 2 * ty + hi) if 0 <= y < parent.shape[0]]
                xs = [x for x in range(2 * tx + lo, 2 * tx + hi) if 0 <= x < parent.shape[1]]
                child[ty, tx] = parent[np.ix_(ys, xs)].any()
        if force_last_row and lod + 1 >= 3:
            child[-1, :] = True
        out[lod + 1] = child
        parent = child
    return out


def content_outside(atlases, t, masks):
    """pixels of the levels of `masks` outside the mask whose value in atlases[-1] is neither the clear value nor what any earlier atlas held
    there: what a fill that keeps to these masks gets wrong, whatever its skipped tiles still hold from earlier fills"""
    n = 0
    for l, m in masks.items():
        c, d = R.level_of(atlases[-1], t, l)
        fresh = ~((c == f32(R.CLEAR_COLOR)).all(-1) & (d == 1))
        for old in atlases[:-1]:
            oc, od = R.level_of(old, t, l)
            fresh &= ~(same_bits(c, oc).all(-1) & same_bits(d, od))
        big = np.kron(m, np.ones((8, 8), bool))[:c.shape[0], :c.shape[1]]
        n += int((fresh & ~big).sum())
    return n


def tile_border_case(make, prepare=None):
    """Hole filling by dirty tiles with content tight against the border of the dirty tiles: single bricks of a wall seen square on by a
    camera that moves 2.8 pixels per draw.  The case asserts its own purpose on the oracle's side: with the level-0 tile masks recomputed
    from the brick outlines (a tile is dirty where a peel pixel is covered, k_depth_limits; a fill keeps to the tiles of its draw and the
    two before) and k_inpaint.hip's reach restated by level_tile_masks(), the full reach leaves no new content outside the dirty tiles,
    the reach 2T .. 2T + 1 would, and so would an unforced last tile row of level 3 (its window reads the first rows of level 1 past
    level 2's last row).  New content: neither the clear value nor what any earlier draw's pyramid held at that pixel."""
    res = M.MARCH_RES[0]
    sc = M.small_scene()
    objs = make(sc, res=res, brick_size=M.MARCH_BRICK, limit=M.LIMIT, view=TILE_VIEW)
    orc = objs["oracle"]
    rx, ry, rz = orc.res_bricks
    layer = rz // 2
    z_surface = (layer + 0.5) * float(orc.brick_size[2]) / float(sc["bbox_max"][2] - sc["bbox_min"][2])
    cnt, vol = wall_counters(orc.res_bricks, layer), wall_volume(res, z_surface)
    pr = S.gl_flat(S.perspective(50.0, TILE_VIEW[0] / TILE_VIEW[1], 0.1, 200.0))
    h, w = TILE_VIEW[1], TILE_VIEW[0]
    out, masks0, atlases = {}, [], []
    for side, o in objs.items():
        if prepare is not None:
            prepare(side, o)
        o.setUseBricks(True); o.setSpaceSkip(True); o.setColorFilling(True)
        o.set_counters(cnt); o.updateOccupiedBricks(); o.set_tsdf(vol)
        for eye, at in TILE_EYES:
            o.drawF(S.gl_flat(S.look_at(eye, at)), pr)
            if o is orc:
                covered = np.asarray(o.view_images()[3])[..., 0] < 1
                masks0.append(np.pad(covered, ((0, -h % 8), (0, -w % 8))).reshape((h + 7) // 8, 8, (w + 7) // 8, 8).any((1, 3)))
                atlases.append(o.atlas())
        out[side] = judge("tile border", side, o.atlas(), o.framebuffer(), min_filled=(300, 600, 900, 800, 1000, 800))
    t = R.lod_tables(*TILE_VIEW)
    mask0 = masks0[-1] | masks0[-2] | masks0[-3]
    purpose = dict(full=content_outside(atlases, t, level_tile_masks(mask0, t)), narrow=content_outside(atlases, t, level_tile_masks(mask0, t, narrow=True)),
                   unforced=content_outside(atlases, t, level_tile_masks(mask0, t, force_last_row=False)))
    assert 3 in level_tile_masks(mask0, t) and purpose["full"] == 0 and purpose["narrow"] > 0 and purpose["unforced"] > 0, purpose
    return out, objs


def all_cpu_cases():
    for size in SIZES:
        yield upload_case, (size,)
    for mask in (1, 2):
        yield upload_case, (MASK_SIZE, mask)
    yield sequence_case, ()
    yield tile_border_case, ()


def print_measurements():
    """python -c 'import fill_cases as C; C.print_measurements()' from tests/: what the table at the head was filled from"""
    M.MEASURE = {}
    try:
        for f, a in all_cpu_cases():
            f(only_oracle, *a)
    finally:
        m, M.MEASURE = M.MEASURE, None
    for k, v in m.items():
        print(f"{k:14s} cases {v['cases']:3d}  dev {v['dev']:.3g}  margin of the worst mismatch {v['need']:.3g}  excluded {v['excluded']:.2%}")
    return m
