"""The float64 reference of the pre-processing passes (tests/preprocess_reference.py) against closed form, and the oracle against that
reference on every case of tests/preprocess_reference_cases.py -- CPU only.  tests/test_gpu_preprocess_reference.py holds the kernels to it.
`sensor` (512 x 424) appears here only: its reference takes some ten seconds in numpy."""
import itertools

import numpy as np
import pytest

import preprocess_reference as P
import preprocess_reference_cases as C

f32 = np.float32
N = 8                                           # texels per axis of linear_lut()
LIN = (2.0, 2.2, -3.0)                          # world = LIN * (u, v, d): a camera that looks along -z


def linear_lut(scale=LIN):
    """cv_xyz(u, v, d) = scale * (u, v, d): trilinear interpolation is exact between the outermost texel centres"""
    c = (np.arange(N) + 0.5) / N
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    return np.stack([x, y, z], -1) * np.asarray(scale)


def interior(h, w):
    """pixels whose own and whose neighbours' coordinates lie between the outermost texel centres of linear_lut()"""
    v, u, (tx, ty) = P.tex_coords(h, w)
    ok = lambda c, t: (c - t > 0.5 / N) & (c + t < 1 - 0.5 / N)
    return ok(v, ty)[:, None] & ok(u, tx)[None, :]


# ---------------------------------------------------------------------------------------------------------------- morph
def test_morph_fills_a_hole_with_the_mean_of_its_eight_neighbours():
    raw = np.full((9, 11), 2.5, f32)
    raw[4, 5] = 0.0
    raw[3, 4] = 2.6
    out, margin = P.morph(raw)
    assert abs(out[4, 5] - (7 * 2.5 + float(f32(2.6))) / 8) < 1e-15          # pre_morph.fs:78-111
    keep = np.ones(raw.shape, bool); keep[4, 5] = False
    assert (out[keep] == raw[keep]).all() and np.isinf(margin[keep]).all()
    assert abs(margin[4, 5] - (0.2 - (float(f32(2.6)) - out[4, 5]))) < 1e-7   # the tap furthest from the average: 2.6


def test_morph_second_loop_measures_from_the_average_not_from_a_depth():
    """neighbours 2.5 x 5, 2.9 x 3: average 2.65; 2.5 is 0.15 from it (kept), 2.9 is 0.25 from it (dropped) -- although 2.9 and 2.5 are 0.4 apart"""
    raw = np.full((5, 5), 2.5, f32)
    raw[2, 2] = 0.0
    raw[1, 1:4] = 2.9
    out, _ = P.morph(raw)
    assert out[2, 2] == 2.5
    raw[1, 1:4] = 2.75                            # average 2.59375: 2.75 is 0.156 from it -> all eight kept
    out, _ = P.morph(raw)
    assert abs(out[2, 2] - (5 * 2.5 + 3 * 2.75) / 8) < 1e-15


def test_morph_keeps_only_depths_strictly_inside_the_limits_and_clamps_its_taps():
    raw = np.zeros((4, 4), f32)
    raw[0, 0] = 4.5                               # the limit itself: no return (pre_morph.fs:38) ...
    raw[3, 3] = np.nextafter(f32(4.5), f32(0))    # ... one ulp inside: kept, and the only valid neighbour of (2, 2), (2, 3), (3, 2)
    out, _ = P.morph(raw)
    assert out[0, 0] == 0 and out[1, 1] == 0 and out[3, 3] == raw[3, 3]
    assert out[2, 2] == raw[3, 3] and out[2, 3] == raw[3, 3] and out[3, 2] == raw[3, 3]


# ---------------------------------------------------------------------------------------------------------------- filter
LIMITS = (0.5, 4.5)
BOX = ((-10.0, -10.0, -10.0), (10.0, 10.0, 10.0))


def run_filter(depth, filter_textures=True, box=BOX, compression=None):
    h, w = depth.shape
    uv = linear_lut((1.0, 1.0, 0.0))[..., :2]
    colour = np.full((3, 4, 3), (200, 60, 40), np.uint8)
    return P.filter_pass(depth.astype(f32), colour, linear_lut(), uv, box[0], box[1], LIMITS, filter_textures, compression)


def test_bilateral_of_a_constant_plane_is_the_plane():
    rg, lab, m = run_filter(np.full((20, 24), 2.5))
    assert np.abs(rg[..., 0] - 0.5).max() < 1e-15 and np.abs(rg[..., 1] - 1.0).max() < 1e-15      # every range weight 1, also where taps clamp
    want = P.rgb_to_lab(np.array([200, 60, 40]) / 255.0)
    assert np.abs(lab - want).max() < 1e-15
    assert abs(m["depth_rg"][10, 12] - 0.35 * 2.5 / 4.5) < 1e-7                                       # every tap sits on the centre: |0 - range limit|
    raw, _, _ = run_filter(np.full((20, 24), 2.5), filter_textures=False)
    assert (raw[..., 0] == 0.5).all() and (raw[..., 1] == 1.0).all()                                  # pre_depth.fs:148-150


def bilateral_by_hand(depth, y, x):
    """pre_depth.fs:85-127 for one interior pixel, as a plain loop"""
    d = depth[y, x]
    lim = float(f32(0.35)) * (d / 4.5)
    bf = w = wr = 0.0
    for dy in range(-6, 7):
        for dx in range(-6, 7):
            s = depth[y + dy, x + dx]
            if s < 0.5 or s > 4.5 or abs(s - d) > lim:
                continue
            gs, gr = 1.0 - np.hypot(dx, dy) / 6.0, 1.0 - min(abs(s - d), lim) / lim
            bf, w, wr = bf + gs * gr * s, w + gs * gr, wr + gr
    return (bf / w - 0.5) / 4.0, wr / 169.0


def test_bilateral_at_a_depth_step_wider_and_narrower_than_the_range_limit():
    """range limit at 2.5 m: 0.35 * 2.5 / 4.5 = 0.194 m"""
    for step in (0.3, 0.1):
        depth = np.full((30, 30), 2.5)
        depth[:, 16:] = 2.5 + step
        rg, _, m = run_filter(depth)
        for x in (12, 15, 16, 20):
            want = bilateral_by_hand(depth.astype(f32).astype(np.float64), 14, x)
            assert abs(rg[14, x, 0] - want[0]) < 1e-14 and abs(rg[14, x, 1] - want[1]) < 1e-14
        if step == 0.3:                                       # wider: the other side is rejected whole -- the depth stays, the share of taps drops
            assert abs(rg[14, 15, 0] - 0.5) < 1e-15 and abs(rg[14, 15, 1] - 7 * 13 / 169.0) < 1e-15
            assert abs(m["depth_rg"][14, 15] - (float(f32(2.8)) - 2.5 - float(f32(0.35)) * 2.5 / float(f32(4.5)))) < 1e-12
        else:                                                 # narrower: the other side pulls the depth over
            assert rg[14, 15, 0] > 0.5 + 1e-4 and 7 * 13 / 169.0 < rg[14, 15, 1] < 1.0


def test_filter_bounding_box_and_colour_slice():
    """world z = -3 * d_norm: a box that ends at z = -1.2 cuts at d_norm 0.4, i.e. 2.1 m (inc_bbox_test.glsl:11-21, pre_depth.fs:143-146)"""
    depth = np.full((12, 12), 2.5)
    depth[:, :6] = 2.0
    rg, _, m = run_filter(depth, filter_textures=False, box=((-10, -10, -1.2), (10, 10, 10)))
    assert (rg[:, 6:] == 0).all() and np.abs(rg[:, :6, 0] - 0.375).max() < 1e-15
    assert np.abs(m["depth_rg"][:, :6] - (1.2 - 3 * 0.375)).max() < 1e-6 and np.abs(m["depth_rg"][:, 6:] - (1.5 - 1.2)).max() < 1e-6
    _, _, m = run_filter(np.array([[0.5, 4.5, 2.5, 0.0]] * 4), filter_textures=False)
    assert (m["lab"][0, :2] == 0).all()                       # d_norm exactly 0 / 1, where :136 switches the cv_uv slice
    assert ((m["lab"][0, 2:] > 0.008) & (m["lab"][0, 2:] < 0.008856)).all()         # elsewhere: X / Xn, Y / Yn, Z / Zn against epsilon


def test_uncompress_follows_the_driver_s_uniforms():
    near, far = 0.3, 3.0
    scale = f32(f32(far) - f32(near))
    sn = f32(scale / f32(255))
    code = np.array([0.0, float(sn) * 0.999, float(sn), 0.5, 1.0], f32)
    got = P.uncompress(code, near, far)
    want = [0.0, 0.0] + [(float(c) ** 2 + float(f32(0.15)) * float(sn)) * float(scale) + float(f32(near)) for c in code[2:]]
    assert np.abs(got - want).max() < 1e-15                  # pre_depth.fs:51-61; `d_c < scaled_near` is strict: the threshold itself decodes


# ---------------------------------------------------------------------------------------------------------------- colour
def lab_by_hand(n):
    """grey of linear-light argument n (= rgb / 255 / 255 in the pipeline): closed form through the branch each pivot takes"""
    lin = (((n + 0.055) / 1.055) ** 2.4 if n > 0.04045 else n / 12.92) * 100.0
    piv = lambda t: t ** (1.0 / 3.0) if t > 0.008856 else (903.3 * t + 16.0) / 116.0
    x = piv(lin * (0.4124 + 0.3576 + 0.1805) / 95.047)
    y = piv(lin * (0.2126 + 0.7152 + 0.0722) / 100.0)
    z = piv(lin * (0.0193 + 0.1192 + 0.9505) / 108.883)
    return np.array([max(0.0, 116 * y - 16), 500 * (x - y), 200 * (y - z)])


@pytest.mark.parametrize("n,gamma,root", [(1.0 / 255, False, False), (0.04, False, False), (0.05, True, False), (0.09, True, False), (0.1, True, True), (0.5, True, True), (1.0, True, True)])
def test_rgb_to_lab_every_branch(n, gamma, root):
    """the argument is what texture() returned; values up to 255 stand for a colour image that was NOT normalised, which is what reaches the
    gamma and cube-root branches (linear + cube root cannot occur: n <= 0.04045 gives Y / Yn <= 0.0032 < epsilon)"""
    assert (n > 0.04045) == gamma
    lin = (((n + 0.055) / 1.055) ** 2.4 if gamma else n / 12.92)
    assert (lin > 0.008856) == root
    got = P.rgb_to_lab(np.full(3, n * 255.0))
    np.testing.assert_allclose(got, lab_by_hand(n), rtol=1e-6, atol=2e-5)      # the reference's literals are fp32 constants: 500 * (x - y) carries 500 * 3e-8
    if not gamma:
        assert abs(got[0] - 903.3 * n / 12.92) < 1e-6                          # L = kappa * Y / Yn outright
    if n == 1.0:
        assert abs(got[0] - 100.0) < 1e-4                                      # white


def test_rgb_to_lab_thresholds_take_the_lower_branch():
    t = P.F(0.04045)
    up = np.nextafter(t, 1.0)
    assert P.pivot_rgb(t) == t / P.F(12.92) * 100 and P.pivot_rgb(up) == ((up + P.F(0.055)) / P.F(1.055)) ** P.F(2.4) * 100 != up / P.F(12.92) * 100
    e = P.F(0.008856)
    assert abs(P.pivot_xyz(e) - (P.F(903.3) * e + 16) / 116) < 1e-15 and abs(P.pivot_xyz(np.nextafter(e, 1.0)) - e ** (1.0 / 3.0)) < 1e-9


def test_8_bit_colours_never_leave_the_linear_branches_yet_reach_the_distance_threshold():
    """With the second / 255 every 8-bit colour stays in the linear branches, where Lab is linear in rgb: the distance of two colours is convex
    in either, so its maximum over the colour cube lies at two of its corners.  L stays below 0.28, but a and b carry 500 * 7.787 and
    200 * 7.787: green and magenta are 0.99 apart, twice the 0.5 pre_boundary.fs:19,105 asks for.  make_scene's own palette stays below 0.29
    (preprocess_reference_cases.saturated is the input on which the comparison decides)."""
    corners = np.array(list(itertools.product((0.0, 1.0), repeat=3)))
    assert (corners / 255.0 < 0.04045).all() and P.lab_decisions(corners).min() > 0.008     # both pivots' arguments stay far below their thresholds
    lab = P.rgb_to_lab(corners)
    assert lab[..., 0].max() < 0.28                                             # L of white
    dist = np.linalg.norm(lab[:, None] - lab[None], axis=-1)
    i, j = np.unravel_index(dist.argmax(), dist.shape)
    assert 0.98 < dist[i, j] < 1.0 and {tuple(corners[i]), tuple(corners[j])} == {(0.0, 1.0, 0.0), (1.0, 0.0, 1.0)}
    palette = P.rgb_to_lab(np.array([[200, 60, 40], [40, 90, 200], [16, 16, 16]]) / 255.0)
    assert max(np.linalg.norm(a - b) for a in palette for b in palette) < 0.29


# ---------------------------------------------------------------------------------------------------------------- boundary
def candidates_around(k):
    """a 21 x 21 image of filter rejects (depth 0.5, share 0.5) with k accepted pixels among the 24 neighbours of (10, 10)"""
    rg = np.zeros((21, 21, 2), f32)
    rg[...] = (0.5, 0.5)
    near = [(y, x) for y in range(8, 13) for x in range(8, 13) if (y, x) != (10, 10)]
    for y, x in near[:k]:
        rg[y, x, 1] = 1.0
    return rg


def test_boundary_needs_eight_of_the_25_taps():
    """total_samples = 16 (pre_boundary.fs:23), so `num_samples < total_samples * 0.5` asks for 8 of the 25 taps of the loop"""
    lab = np.zeros((21, 21, 3))
    lab[10, 10, 0] = 0.2
    for k, kept in ((7, False), (8, True), (24, True)):
        db, sil, m, info = P.boundary(candidates_around(k), lab)
        assert info["counted"][10, 10] == k and info["candidates"][10, 10]
        assert tuple(db[10, 10]) == ((0.5, 1.0) if kept else (-1.0, float(f32(0.1)))) and sil[10, 10] == 0
        # kept: colour distance 0.2, 0.3 from its threshold; dropped by the count, which is exact: only the NEAREST fetches' half texel is left
        assert abs(m[10, 10] - (0.3 if kept else 0.5)) < 1e-6
    db, _, m, _ = P.boundary(candidates_around(8), lab, refine=False)
    assert tuple(db[10, 10]) == (-1.0, float(f32(0.1))) and abs(m[10, 10] - 0.5) < 1e-6   # :105


def test_boundary_colour_distance_and_the_three_kinds_of_pixel():
    rg = candidates_around(24)
    rg[0, 0] = (0.0, 1.0)                                                       # outside the box
    rg[0, 1] = (-1.0, 1.0)
    lab = np.zeros((21, 21, 3))
    lab[8:13, 8:13, 0] = 0.6
    lab[10, 10, 0] = 0.0                                                        # every neighbour 0.6 away: mean 0.6 > 0.5
    db, sil, m, info = P.boundary(rg, lab)
    assert abs(info["colour_dist"][10, 10] - 0.6) < 1e-6 and tuple(db[10, 10]) == (-1.0, float(f32(0.1))) and abs(m[10, 10] - 0.1) < 1e-6
    assert tuple(db[0, 0]) == (0.0, 0.0) and tuple(db[0, 1]) == (-1.0, 0.0) and sil[0, 0] == 0 and sil[0, 1] == 0      # :90-99
    assert tuple(db[9, 9]) == (0.5, 0.0) and sil[9, 9] == 1                     # accepted by the filter: :114-116
    lab[8:13, 8:13, 0] = 0.4
    lab[10, 10, 0] = 0.0
    assert tuple(P.boundary(rg, lab)[0][10, 10]) == (0.5, 1.0)


def test_boundary_share_threshold_is_the_fp32_constant():
    rg = candidates_around(24)
    rg[9, 9, 1] = f32(0.65)                                                     # 0.65f > 0.65f is false: a candidate (with 23 accepted taps)
    rg[9, 10, 1] = np.nextafter(f32(0.65), f32(1))
    _, sil, _, info = P.boundary(rg, np.zeros((21, 21, 3)))
    assert info["candidates"][9, 9] and sil[9, 9] == 0 and not info["candidates"][9, 10] and sil[9, 10] == 1


# ---------------------------------------------------------------------------------------------------------------- normal, bricks
def test_normal_of_a_tilted_plane_with_its_sign():
    """d = d0 + gx * u + gy * v under world = (a u, b v, c d): dW/du = (a, 0, c gx), dW/dv = (0, b, c gy), and pre_normal.fs:55 takes
    cross(bottom - top, left - right) = cross(dW/dv, dW/du) = (b c gx, a c gy, -a b)"""
    h, w = 40, 50
    gx, gy = 0.2, -0.1
    v, u, _ = P.tex_coords(h, w)
    d = (0.3 + gx * u[None, :] + gy * v[:, None]).astype(f32)
    db = np.stack([d, np.zeros_like(d)], -1)
    n, m, marks = P.normal_pass(db, linear_lut(), (-1, -1, -4), (0.5, 0.5, 0.5), (8, 8, 8))
    a, b, c = LIN
    want = np.array([b * c * gx, a * c * gy, -a * b])
    want /= np.linalg.norm(want)
    ins = interior(h, w)
    assert np.abs(n[ins] - want).max() < 1e-5 and want[2] < 0                   # 1e-5: d is an fp32 image
    assert (m[ins] > 1e-4).all() and marks["pixel"].size == h * w
    db[5, 5, 0] = 0.0                                                           # a hole: no normal, no mark; its neighbours fall back on their own depth
    n2, m2, marks2 = P.normal_pass(db, linear_lut(), (-1, -1, -4), (0.5, 0.5, 0.5), (8, 8, 8))
    assert (n2[5, 5] == 0).all() and np.isinf(m2[5, 5]) and marks2["pixel"].size == h * w - 1
    assert np.abs(n2[5, 6] - want).max() > 1e-3 and abs(np.linalg.norm(n2[5, 6]) - 1) < 1e-12


def test_normal_of_a_flat_patch_in_the_lut_s_clamped_rim_is_a_zero_cross_product():
    db = np.zeros((40, 50, 2), f32)
    db[..., 0] = 0.5
    n, m, _ = P.normal_pass(db, linear_lut(), (-1, -1, -4), (0.5, 0.5, 0.5), (8, 8, 8))
    assert (m[0] < 1e-12).all() and (m[:, 0] < 1e-12).all() and (m[interior(40, 50)] > 1e-4).all()


def test_brick_of_a_known_world_point():
    lo, bs, res = (-1.0, 0.0, -1.0), (0.25, 0.25, 0.25), (8, 9, 8)
    gid = lambda x, y, z: (z * 9 + y) * 8 + x
    pos = np.array([[0.3, 0.6, -0.15],          # brick (5, 2, 3), centre (0.375, 0.625, -0.125): x is furthest (-0.075) -> neighbour (4, 2, 3), counted
                    [0.37, 0.7, -0.125],        # same brick, y furthest (+0.075) -> neighbour (5, 3, 3); |dx| = 0.005 < 0.025: the neighbour gets + 0
                    [-0.99, 0.1, -0.9]])        # brick (0, 0, 0), x furthest towards -1: the neighbour is clamped onto the brick itself
    main, nb, add, margin = P.mark_brick(pos, lo, bs, res)
    assert list(main) == [gid(5, 2, 3), gid(5, 2, 3), gid(0, 0, 0)]
    assert list(nb) == [gid(4, 2, 3), gid(5, 3, 3), gid(0, 0, 0)] and list(add) == [1, 0, 1]
    assert abs(margin[0] - 0.05) < 1e-9 and abs(margin[1] - 0.02) < 1e-9       # 0.3 is 0.05 from the face x = 0.25; 0.005 is 0.02 from the 0.1 test
    counts = P.brick_counts(dict(main=main, neighbour=nb, add=add), 8 * 9 * 8)
    assert counts[gid(5, 2, 3)] == 2 and counts[gid(4, 2, 3)] == 1 and counts[gid(5, 3, 3)] == 0 and counts[gid(0, 0, 0)] == 2 and counts.sum() == 5
    out = P.mark_brick(np.array([[-1.01, 0.1, 0.0]]), lo, bs, res)
    assert out[3][0] == 0                                                       # uvec3() of a negative float: left open


# ---------------------------------------------------------------------------------------------------------------- quality
def test_quality_of_a_fronto_parallel_plane():
    """no tap rejected, every range weight 1, the normal towards a camera straight in front of the pixel: 1 / (6.5 * depth)"""
    h, w = 30, 30
    db = np.zeros((h, w, 2), f32)
    db[..., 0] = 0.4
    nrm = np.zeros((h, w, 3), f32)
    nrm[..., 2] = 1.0
    v, u, _ = P.tex_coords(h, w)
    cam = (LIN[0] * u[15], LIN[1] * v[15], 5.0)                                 # world z of the plane: -1.2
    q, m = P.quality_pass(db, nrm, linear_lut(), cam)
    assert abs(q[15, 15] - 1.0 / (float(f32(6.5)) * float(f32(0.4)))) < 1e-12
    assert abs(m[15, 15] - float(f32(0.35)) * float(f32(0.4))) < 1e-12           # all taps at the centre's depth
    cosine = 6.2 / np.hypot(6.2, LIN[0] * (u[25] - u[15]))
    assert abs(q[15, 25] / q[15, 15] - cosine ** 2) < 1e-7                      # off axis: cos^2 (1e-7: 0.4 is an fp32 depth)
    q2, m2 = P.quality_pass(db, -nrm, linear_lut(), cam)
    assert (m2 == 0).all() and abs(q2[15, 15] - q[15, 15]) < 1e-12              # pow(negative, 2.0): left open, margin 0


def test_quality_counts_rejected_taps():
    h, w = 30, 30
    db = np.zeros((h, w, 2), f32)
    db[..., 0] = 0.4
    db[:, 20:, 0] = 0.6                                                         # 0.2 > 0.35 * 0.4: the window of x = 15 loses its columns 20, 21
    db[0, 0, 0] = -1.0
    nrm = np.zeros((h, w, 3), f32)
    nrm[..., 2] = 1.0
    v, u, _ = P.tex_coords(h, w)
    q, m = P.quality_pass(db, nrm, linear_lut(), (LIN[0] * u[15], LIN[1] * v[15], 5.0))
    share = 1.0 - 26.0 / 169.0
    assert abs(q[15, 15] - share ** 6 * share ** 6 / (float(f32(6.5)) * float(f32(0.4)))) < 1e-12    # pre_quality.fs:107-111
    assert abs(m[15, 15] - (float(f32(0.6)) - float(f32(0.4)) - float(f32(0.35)) * float(f32(0.4)))) < 1e-9
    assert q[0, 0] == 0 and np.isinf(m[0, 0])


# ---------------------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("case", C.all_cases(), ids=C.case_id)
def test_oracle_matches_the_reference(case):
    res = C.run_case(C.only_oracle, *case)
    assert len(res) == 2                                                        # the input as built, and under the mirrored calibration


def test_the_cases_as_built_leave_the_quality_pass_undefined():
    """what mirrored() is for: under make_scene's calibration the angle of pre_quality.fs:46 is negative wherever there is a normal"""
    sc = C.scene("odd")
    o = C.only_oracle(sc, **C.kw_of("odd"))["oracle"]
    C.pc.process(o, sc)
    pp = o.preprocessed()
    _, m = C._quality(pp["depth_b"][0], pp["normals"][0], 0, "odd")
    assert np.isfinite(m).sum() > 1000 and (m[np.isfinite(m)] == 0).mean() > 0.99
