"""Hole filling against the float64 reference of tests/fill_reference.py, the half that runs without a GPU: the oracle on every case of
tests/fill_cases.py under its one acceptance rule, closed-form known answers for the reference itself, and the reference's equal-depth
quirk.  tests/test_gpu_fill_reference.py holds the kernels to the same cases and numbers."""
import numpy as np
import pytest

import fill_cases as C
import fill_reference as R

f32 = np.float32
CASES = list(C.all_cpu_cases())


@pytest.mark.parametrize("case,args", CASES, ids=[f.__name__ + "-" + "-".join("x".join(map(str, a)) if isinstance(a, tuple) else str(a) for a in args) for f, args in CASES])
def test_oracle_hole_filling_against_the_float64_reference(case, args):
    out, _ = case(C.only_oracle, *args)
    r = out["oracle"]
    assert max(r["level_excluded"]) <= C.CAP and r["fb_excluded"] <= C.CAP


def test_oracle_past_the_level_tables():
    C.past_tables_case(C.only_oracle)


def test_measured_table_is_what_the_tolerances_come_from():
    """TABLE is 4 x what print_measurements() finds, rounded up, and nothing is measured anywhere else.  The upper side is meant: an oracle
    that comes closer to the reference (a reordering of its fp32 operations, say) fails here until the table is measured again, so the
    tolerances never stay wider than 5 x what they were derived from."""
    m = C.print_measurements()
    for k in ("pyr_colour", "pyr_depth", "fb_colour"):
        assert 4 * m[k]["dev"] <= C.TABLE[k]["tol"] <= 5 * m[k]["dev"], (k, m[k])
        assert m[k]["excluded"] <= C.CAP
    assert 4 * m["depth_mean"]["need"] <= C.TABLE["depth_mean"]["bound"] <= 5 * m["depth_mean"]["need"], m["depth_mean"]
    assert m["fb depth"]["dev"] == 0 and m["fb depth"]["need"] == 0


# ---------------------------------------------------------------------------------------------------------------- known answers
def test_lod_tables_1280x720():
    """view_lod.cpp:24-50 by hand"""
    t = R.lod_tables(1280, 720)
    assert t["num_lods"] == 10 and t["full"] == (1920, 720)
    assert t["res"].tolist() == [[1280, 720], [640, 360], [320, 180], [160, 90], [80, 45], [40, 22], [20, 11], [10, 5], [5, 2], [2, 1]]
    assert t["off"].tolist() == [[0, 0], [1280, 360], [1280, 180], [1280, 90], [1280, 45], [1280, 23], [1280, 12], [1280, 7], [1280, 5], [1280, 4]]
    assert R.lod_tables(173, 99)["full"] == (259, 99) and R.lod_tables(5, 3)["num_lods"] == 2


def valid_image(w, h, seed=3):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.random((h, w, 3)), np.ones((h, w, 1))], -1), np.full((h, w), 0.5)


def test_level_1_of_a_valid_image_is_the_mean_over_the_squeezed_window():
    """every sample valid, every depth 0.5 (16 x 0.5 is exact, every sample passes `>= depth_av`): level-1 pixel (i, j) is the mean over rows
    2j - 1 .. 2j + 2 and over the atlas columns floor(1.5 (floor(2 X / 3) + dx + .5)), X = 2 i, dx = -1 .. 2"""
    w, h = 48, 32
    rgba, depth = valid_image(w, h)
    f = R.fill_colors(rgba, depth)
    l1c, l1d = R.level_of(f["atlas"], f["tables"], 1)
    for i, j in ((7, 5), (1, 1), (20, 9), (3, 14)):
        cols = [int(np.floor(1.5 * ((2 * (2 * i)) // 3 + dx + 0.5))) for dx in (-1, 0, 1, 2)]
        want = rgba[2 * j - 1:2 * j + 3][:, cols, :3].reshape(16, 3).mean(0)
        np.testing.assert_allclose(l1c[j, i, :3], want, rtol=0, atol=1e-15)
        assert l1c[j, i, 3] == 1 and l1d[j, i] == 0.5 and f["levels"][0]["n"][j, i] == 16


def test_every_third_column_is_never_read():
    """the squeezed copy holds atlas columns floor(1.5 (s + .5)) = 0, 2, 3, 5, 6, ...: columns 1, 4, 7, ... of level 0 reach no level"""
    w, h = 48, 32
    rgba, depth = valid_image(w, h)
    t = R.lod_tables(w, h)
    read = set(R.transfer_columns(t)[0][: 2 * w // 3].tolist())
    assert read == {c for c in range(w) if c % 3 != 1}
    other = rgba.copy()
    other[:, 1::3, :3] = 7.0
    a, b = R.fill_colors(rgba, depth), R.fill_colors(other, depth)
    for la, lb in zip(a["levels"], b["levels"]):
        assert (la["rgba"] == lb["rgba"]).all() and (la["depth"] == lb["depth"]).all()
    changed = rgba.copy()
    changed[:, 2::3, :3] = 7.0
    assert (R.fill_colors(changed, depth)["levels"][0]["rgba"] != a["levels"][0]["rgba"]).any()


def test_a_pixel_valid_at_level_0_passes_through_the_colour_fill():
    w, h = 16, 16                                                # every coordinate product an exact integer: no truncation is unsafe
    rgba, depth = (a.astype(np.float64) for a in C.image(w, h, 1, 2))
    fb = R.fill_colors(rgba, depth)["framebuffer"]
    valid = (rgba[..., 3] > 0) & (depth < 1)
    assert valid.sum() > 100 and fb["trunc_ok"].all()
    assert ((fb["rgba"][valid] == rgba[valid]) | np.isnan(rgba[valid])).all() and (fb["depth"][valid] == depth[valid]).all()
    assert (fb["level"][valid] == 0).all()
    bg = depth >= 1
    assert (fb["rgba"][bg] == 0).all() and (fb["depth"][bg] == 1).all() and not fb["written"][bg].any()


def test_mirrored_fetch_at_a_corner():
    """GL_MIRRORED_REPEAT: one texel past the right and the top edge the filter sees texels W - 1, W - 2 and h - 1, h - 2 again; half a texel
    before the left edge it sees texel 0 twice"""
    h, W = 4, 6
    tex = np.arange(h * W * 4, dtype=np.float64).reshape(h, W, 4)
    v, fragile = R.texture_linear_mirrored(tex, np.array([(W + 1.0) / W]), np.array([(h + 1.0) / h]))
    assert (v[0] == (tex[h - 1, W - 1] + tex[h - 1, W - 2] + tex[h - 2, W - 1] + tex[h - 2, W - 2]) / 4).all() and not fragile.any()
    v, _ = R.texture_linear_mirrored(tex, np.array([0.25 / W]), np.array([0.25 / h]))
    assert (v[0] == tex[0, 0]).all()
    v, _ = R.texture_linear_mirrored(tex, np.array([1.0 / W]), np.array([1.0 / h]))
    assert (v[0] == (tex[0, 0] + tex[0, 1] + tex[1, 0] + tex[1, 1]) / 4).all()
    tex[0, 1, 2] = np.nan
    assert R.texture_linear_mirrored(tex, np.array([0.5 / W]), np.array([0.5 / h]))[1].all()     # a NaN tap of weight 0


def test_mask_modes_write_their_channels_over_a_kept_buffer():
    w, h = 16, 16
    rgba, depth = (a.astype(np.float64) for a in C.image(w, h, 1, 2))
    base = np.full((h, w, 4), 5.0)
    plain = R.fill_colors(rgba, depth)["framebuffer"]
    wr = plain["written"]
    for mask, chan in ((1, [0]), (2, [1, 2])):
        fb = R.fill_colors(rgba, depth, mask, base)["framebuffer"]
        rest = [k for k in range(4) if k not in chan]
        same = (fb["rgba"][wr][:, chan] == plain["rgba"][wr][:, chan]) | np.isnan(plain["rgba"][wr][:, chan])
        assert same.all() and (fb["rgba"][wr][:, rest] == 5.0).all() and (fb["rgba"][~wr] == 5.0).all()


def test_a_cut_step_equals_the_literal_step():
    """the judge's step -- a cleared atlas with levels 0 .. l, squeezed, inpainted -- is the step fill_colors() takes with its two real atlases"""
    w, h = 61, 45
    rgba, depth = (a.astype(np.float64) for a in C.image(w, h, 1, 12))
    f = R.fill_colors(rgba, depth)
    t = f["tables"]
    T = R.cleared_atlas(t)
    for l in range(t["num_lods"] - 1):
        R.place_level(T, t, l, *R.level_of(f["atlas"], t, l))
        Sq, sm = R.transfer(T, t)
        cut, lit = R.inpaint_level(Sq, t, l, sm), f["levels"][l]
        for k in ("rgba", "depth"):
            assert ((cut[k] == lit[k]) | (np.isnan(cut[k]) & np.isnan(lit[k]))).all(), (l, k)
    last, _ = R.transfer(f["atlas"], t)
    assert all(((a == b) | (np.isnan(a) & np.isnan(b))).all() for a, b in zip(last, f["squeezed"]))      # the other atlas ends as the squeezed copy


# ---------------------------------------------------------------------------------------------------------------- the equal-depth quirk
def sequential_mean(d, n):
    s = f32(0)
    for _ in range(n):
        s = f32(s + d)
    return f32(s / f32(n))


def test_equal_depths_can_all_fail_the_mean_test():
    """A quirk of the reference, not of the kernels: in fp32 the sequential sum of n equal depths, divided by n, exceeds the depth itself for
    some depths unless n is 1, 2 or 4 (here: about 8 % of random depths at n = 3, about 36 % at n = 16).  tsdf_inpaint.fs:75-88 then rejects
    every sample and writes 0 / 0 with alpha 1.  The float64 reference gives such pixels margin 0, and the oracle produces exactly that NaN."""
    rng = np.random.default_rng(11)
    ds = rng.uniform(0.1, 0.95, 4000).astype(f32)
    rate = {n: float(np.mean([sequential_mean(d, n) > d for d in ds])) for n in (1, 2, 3, 4, 16)}
    assert rate[1] == rate[2] == rate[4] == 0
    assert 0.04 < rate[3] < 0.12 and 0.25 < rate[16] < 0.45, rate
    d = next(d for d in ds if sequential_mean(d, 16) > d)
    w, h = 16, 16
    rgba = valid_image(w, h)[0].astype(f32)
    depth = np.full((h, w), d, f32)
    ref = R.fill_colors(rgba, depth)["levels"][0]
    inner = ref["n"] == 16
    assert inner.sum() >= 10 and (ref["margin"][inner] == 0).all()
    assert (ref["margin"][np.isin(ref["n"], (1, 2, 4))] == np.inf).all()
    o = C.OracleRecon(C.scene(), **C.recon_kw(w, h))
    o.set_view_images(rgba, depth)
    o.fillColors()
    c1, d1 = R.level_of(o.atlas(), R.lod_tables(w, h), 1)
    assert np.isnan(c1[inner][:, :3]).all() and (c1[inner][:, 3] == 1).all() and np.isnan(d1[inner]).all()
