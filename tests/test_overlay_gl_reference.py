"""CPU: known answers that pin tests/overlay_gl_reference.py, the float64 GL reference of the overlay draws, and then every case of
tests/overlay_gl_cases.py with the fp32 twins alone against it (tests/test_gpu_overlay_gl_reference.py adds the kernels)."""
import numpy as np
import pytest

import overlay_gl_cases as C
import overlay_gl_reference as G
import brick_overlay_reference as TB
import client_overlay_reference as TC
import overlay_reference as TO
import sensor_view_reference as TS
from oracle.oracle import frustum

RED = (1.0, 0.0, 0.0, 1.0)


def line(a, b, view=(8, 8), width=1.0):
    """the fragments {(px, py): z} of one window segment, and the margins it leaves"""
    fr = G.Frags(view)
    G.window_line(fr, a, b, RED, width)
    out = {}
    if fr.pix:
        for p, z in zip(np.concatenate(fr.pix), np.concatenate(fr.z)):
            out[(int(p % view[0]), int(p // view[0]))] = float(z)
    return out, fr.margin


def twin_line(a, b, view=(8, 8), width=1):
    return {(px, py) for px, py, _ in TC.wide_window_line_fragments(a, b, view, width)}


# ---------------------------------------------------------------------- the diamond-exit rule by hand
def test_start_inside_a_diamond_right_of_its_centre_is_drawn_and_an_end_inside_one_is_not():
    """(2.7, 3.5) -> (5.6, 3.5): the start lies in pixel 2's diamond (0.2 from its centre) and the line leaves it: a fragment.  The end lies in
    pixel 5's diamond: none.  The column walk asks for centres in [2.7, 5.6) and draws 3, 4, 5: the two differ at the pixels that hold an end
    point, which GL leaves open."""
    got, margin = line((2.7, 3.5, 0.5), (5.6, 3.5, 0.5))
    assert set(got) == {(2, 3), (3, 3), (4, 3)}
    assert twin_line((2.7, 3.5, 0.5), (5.6, 3.5, 0.5)) == {(3, 3), (4, 3), (5, 3)}
    assert margin[3, 2, G.OPEN] == 0 and margin[3, 5, G.OPEN] == 0 and np.isinf(margin[3, 3, G.OPEN]) and np.isinf(margin[3, 4, G.OPEN])
    assert margin[3, 3, G.EDGE] == 0.5 and abs(margin[3, 2, G.EDGE] - 0.3) < 1e-12      # through the centre; the start 0.2 off its centre


def test_a_segment_wholly_inside_one_diamond_makes_no_fragment():
    got, margin = line((3.3, 3.4, 0.5), (3.6, 3.6, 0.5))
    assert got == {} and margin[3, 3, G.OPEN] == 0


def test_a_45_degree_segment_along_diamond_edges():
    """(1, 1.5) -> (4, 4.5) runs along the upper left edges of the diamonds (k, k) and the lower right edges of (k, k + 1).  The spec's shift by
    (-e, -e^2) moves it up and left, into the diamonds (k, k + 1): it starts inside (0, 1)'s and ends inside (3, 4)'s.  Edge margin 0 all along."""
    got, margin = line((1.0, 1.5, 0.5), (4.0, 4.5, 0.5))
    assert set(got) == {(0, 1), (1, 2), (2, 3)}
    for px, py in ((0, 1), (1, 2), (2, 3), (3, 4), (1, 1), (2, 2), (3, 3)):
        assert margin[py, px, G.EDGE] < 1e-12


def test_a_vertical_segment_on_an_integer_x():
    """x = 3 touches the right corners of column 2's diamonds and the left corners of column 3's; shifted by -e it enters column 2's.  The walk's
    floor(3.0) picks column 3: a tie, margin 0 on both columns (14.5.1's conditions allow a fragment one pixel off)."""
    got, margin = line((3.0, 1.2, 0.5), (3.0, 4.8, 0.5))
    assert set(got) == {(2, 1), (2, 2), (2, 3), (2, 4)}
    assert twin_line((3.0, 1.2, 0.5), (3.0, 4.8, 0.5)) == {(3, 1), (3, 2), (3, 3), (3, 4)}
    assert (margin[1:5, 2:4, G.EDGE] < 1e-12).all()


def test_depth_is_that_of_the_fragments_centre_projected_onto_the_segment():
    """eq. 14.5: (1.2, 1.2) -> (6.2, 4.2), z 0.1 -> 0.9; pixel (3, 2) has its centre (3.5, 2.5) at t = (2.3 * 5 + 1.3 * 3) / 34"""
    got, _ = line((1.2, 1.2, 0.1), (6.2, 4.2, 0.9))
    assert (3, 2) in got and abs(got[(3, 2)] - (0.1 + 0.8 * (2.3 * 5 + 1.3 * 3) / 34.0)) < 1e-12
    tw = {(px, py): z for px, py, z in TC.wide_window_line_fragments((1.2, 1.2, 0.1), (6.2, 4.2, 0.9), (8, 8), 1)}
    assert set(tw) - {(1, 1), (6, 4)} == set(got) - {(1, 1), (6, 4)}
    assert max(abs(tw[k] - got[k]) for k in set(tw) & set(got)) < 2e-7


def test_a_width_2_line_by_hand():
    """(1.2, 3.7) -> (5.2, 3.7), width 2: moved to y = 3.2 it crosses the diamonds of row 3 in columns 1 .. 4 (column 5's centre is 0.6 from its
    end); each fragment is the lower one of two, rows 3 and 4, at the lower one's depth 0.2 + 0.4 * (c - 1.2) / 4"""
    got, margin = line((1.2, 3.7, 0.2), (5.2, 3.7, 0.6), width=2.0)
    assert set(got) == {(c, r) for c in (1, 2, 3, 4) for r in (3, 4)}
    for c in (1, 2, 3, 4):
        assert abs(got[(c, 3)] - (0.2 + 0.4 * (c + 0.5 - 1.2) / 4.0)) < 1e-12 and got[(c, 4)] == got[(c, 3)]
    assert twin_line((1.2, 3.7, 0.2), (5.2, 3.7, 0.6), width=2) == set(got)
    assert abs(margin[3, 2, G.EDGE] - 0.2) < 1e-12 and margin[4, 2, G.EDGE] == margin[3, 2, G.EDGE]      # the moved line runs 0.3 from row 3's centres
    # through pixel centres (y = 3.5) the moved line runs along the row boundary y = 3: the literal rule, shifted by -e^2, takes rows 2 and 3
    got, margin = line((1.2, 3.5, 0.2), (5.2, 3.5, 0.6), width=2.0)
    assert set(got) == {(c, r) for c in (1, 2, 3, 4) for r in (2, 3)} and (margin[2:4, 1:5, G.EDGE] < 1e-12).all()


def test_a_size_3_point_by_hand():
    """window centre (4.2, 4.7): the centres p with c - 1.5 <= p < c + 1.5 are 3.5, 4.5, 5.5 in x and in y"""
    fr = G.Frags((8, 8))
    G.clip_points(fr, np.array([[4.2 / 8 * 2 - 1, 4.7 / 8 * 2 - 1, 0.0, 1.0]]), 3.0, RED)
    rgba, depth, margin, touched = fr.resolve(np.zeros((8, 8, 4)), np.ones((8, 8)))
    want = np.ones((8, 8))
    want[3:6, 3:6] = 0.5
    assert (depth == want).all() and (rgba[3:6, 3:6] == RED).all() and (touched == (want < 1)).all()
    assert abs(margin[3, 3, G.EDGE] - 0.3) < 1e-12 and abs(margin[3, 2, G.EDGE] - 0.2) < 1e-12          # the square's edges x 2.7, y 3.2 against the centres (3.5, 3.5) and (2.5, 3.5)


def test_a_point_is_clipped_by_its_centre():
    fr = G.Frags((8, 8))
    G.clip_points(fr, np.array([[1.0 + 1e-9, 0.0, 0.0, 1.0]]), 3.0, RED)                                  # a hair outside: nothing, though its square reaches in
    _, depth, margin, touched = fr.resolve(np.zeros((8, 8, 4)), np.ones((8, 8)))
    assert (depth == 1).all() and touched[4, 7] and margin[4, 7, G.TEST] < 1e-8


def test_gl_less_keeps_the_first_of_equal_depths_and_reports_the_gap_to_another_colour():
    fr = G.Frags((4, 1))
    fr.add([1], [0], [0.5], (0.0, 1.0, 0.0, 1.0))
    fr.add([1, 2], [0, 0], [0.5, 0.25], RED)
    fr.add([2], [0], [0.75], (0.0, 1.0, 0.0, 1.0))
    rgba, depth, margin, _ = fr.resolve(np.zeros((1, 4, 4)), np.array([[1.0, 1.0, 0.25, 1.0]]))
    assert (rgba[0, 1] == (0, 1, 0, 1)).all() and depth[0, 1] == 0.5 and margin[0, 1, G.ZGAP] == 0.0
    assert (rgba[0, 2] == 0).all() and depth[0, 2] == 0.25 and margin[0, 2, G.TEST] == 0.0                # 0.25 < 0.25 fails: a tie with the framebuffer


def test_one_brick_orthographic_outline_by_hand():
    """the outline of tests/test_brick_overlay_reference.py: corners exactly on the pixel centres 2.5 and 6.5.  A segment that starts on a centre
    leaves that diamond (drawn), one that ends on a centre ends inside it (not drawn); the four segments along z are points inside a diamond."""
    ortho = np.zeros(16, np.float32)
    ortho[0], ortho[5], ortho[10], ortho[12], ortho[13], ortho[15] = 0.5, 0.5, -0.25, -0.6875, -0.6875, 1.0
    rgba, depth, margin, touched = G.draw_bricks([0], (2, 2, 2), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), np.eye(4).reshape(16), ortho, (16, 16),
                                                 np.zeros((16, 16, 4)), np.ones((16, 16)))
    want = np.ones((16, 16))
    for k in range(2, 7):
        want[2, k] = want[6, k] = want[k, 2] = want[k, 6] = 0.375
    want[6, 2] = want[2, 6] = 0.5
    assert (depth == want).all() and (rgba[want < 1] == G.WIRE_RED).all() and (rgba[want == 1] == 0).all()
    assert (margin[[2, 2, 6, 6], [2, 6, 2, 6], G.OPEN] == 0).all()
    # GL binds nobody at these end pixels; the header's walk (centres in [start, end)) sides with the literal rule there, and must go on doing so
    tc, td = TB.draw_bricks(np.array([0]), (2, 2, 2), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), np.eye(4, dtype=np.float32).reshape(16), ortho, (16, 16),
                            np.zeros((16, 16, 4), np.float32), np.ones((16, 16), np.float32))
    assert (td == depth).all() and (tc == rgba).all()


def test_points_of_equal_depth_the_first_drawn_stays_and_a_tie_with_the_framebuffer_fails():
    """a 4^3 grid over a 4^3 volume (every sample is a texel: data) under P = diag(1e-6, 1e-6, 1e-20, 1): all 64 points fall on the four pixels
    about the view's centre at window z 0.5 exactly, in fp32 and in float64 alike, each with its own shade of red.  GL_LESS keeps the first of
    them per pixel, and draws nothing where the framebuffer already holds 0.5 -- exact ties, which no margin excuses."""
    vol = np.random.default_rng(8).uniform(0.001, 0.009, (4, 4, 4)).astype(np.float32)
    flat = np.diag([1e-6, 1e-6, 1e-20, 1.0]).astype(np.float32).T.reshape(16)
    mv = np.eye(4, dtype=np.float32).reshape(16)
    fc, fd = np.zeros((8, 8, 4), np.float32), np.ones((8, 8), np.float32)
    fd[3, 4] = 0.5
    args = (vol, (4, 4, 4), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), mv, flat, (8, 8), fc, fd)
    rgba, depth, margin, touched = G.draw_calibvis(*args)
    tc, td = TO.draw_calibvis(*args)
    assert (depth[3:5, 3:5] == 0.5).all() and (depth != fd).sum() == 3 and (td == depth).all()
    first = {(3, 3): 0, (3, 4): 2, (4, 3): 8, (4, 4): 10}                # (row, column) -> the lowest grid index x + 4 y (+ 16 z) with that sign of x and y
    for (row, col), i in first.items():
        want = (0, 0, 0, 0) if (row, col) == (3, 4) else (1.0 - float(vol.reshape(-1)[i]) / G.CALIB_LIMIT, 0, 0, 1)
        assert np.allclose(rgba[row, col], want, atol=1e-12) and np.allclose(tc[row, col], want, atol=1e-6)
        assert margin[row, col, G.ZGAP] == 0 or (row, col) == (3, 4)


def test_one_blit_texel_by_hand():
    """view 8 x 4: resolution_full.x = 12, viewport 6 x 2.  Pixel (1, 0) has (u, v) = (0.25, 0.25); on the 12 x 4 atlas u * 12 - 0.5 = 2.5 and
    v * 4 - 0.5 = 0.5: the mean of texels (2, 0), (3, 0), (2, 1), (3, 1).  Pixel (5, 1), (u, v) = (11 / 12, 0.75): 10.5 and 2.5"""
    assert G.blit_viewport(8, 4) == (6, 2) and G.blit_viewport(173, 99) == (129, 49)
    src = np.random.default_rng(1).uniform(0, 1, (4, 12, 4))
    fb = np.full((4, 8, 4), 7.0)
    rgba, depth, margin, touched = G.blit(src, (8, 4), fb, np.full((4, 8), 0.5))
    assert np.allclose(rgba[0, 1, :3], src[0:2, 2:4, :3].mean((0, 1)), atol=1e-15) and rgba[0, 1, 3] == 1.0
    assert np.allclose(rgba[1, 5, :3], src[2:4, 10:12, :3].mean((0, 1)), atol=1e-15)
    assert touched.sum() == 12 and (rgba[~touched] == 7).all() and (depth == 0.5).all()
    flipped = src[::-1]
    assert not np.allclose(G.blit(flipped, (8, 4), fb, depth)[0][0, 1, :3], rgba[0, 1, :3])       # row 0 of the source is the bottom row of the view


def test_one_turned_sensor_texel_by_hand():
    """view 8 x 8, quad (2, 1) - (6, 5), a 4 x 4 NEAREST layer (type 5).  Pixel column 3, GL row 5: ImGui position (3.5, 2.5), Frag_UV
    (0.375, 0.375); turned: (-0.125 + 0.5, 0.125 + 0.5) = (0.375, 0.625) -> texel (1, 2).  The reversed turn would fetch texel (2, 1)."""
    layer = np.arange(16, dtype=np.float32).reshape(4, 4)
    rgba, depth, margin, touched = G.sensor_window(5, layer, (2.0, 1.0, 6.0, 5.0), None, np.zeros((8, 8, 4)), np.ones((8, 8)))
    assert (rgba[5, 3] == (9, 9, 9, 1)).all() and layer[2, 1] == 9
    assert touched.sum() == 16 and touched[3:7, 2:6].all() and (depth == 1).all()
    assert G.ROT_COS == float(np.float32(-4.371138828673793e-08)) and G.ROT_SIN == 1.0
    twin = TS.draw(5, layer, (2.0, 1.0, 6.0, 5.0), None, np.zeros((8, 8, 4), np.float32))
    assert (twin == rgba).all()


def test_the_blend_of_a_partly_transparent_colour_layer():
    """RGBA8 texels with every alpha (the decoded DXT1 of a wire frame): SRC_ALPHA, ONE_MINUS_SRC_ALPHA on all four channels"""
    rng = np.random.default_rng(4)
    layer = rng.integers(0, 256, (30, 40, 4)).astype(np.uint8)
    layer[:10, :, 3], layer[10:20, :, 3] = 255, 0
    fb = rng.uniform(0, 1, (C.VIEW[1], C.VIEW[0], 4)).astype(np.float32)
    before = (fb, np.ones((C.VIEW[1], C.VIEW[0]), np.float32))
    n, share = C.sensor_check(C.only_twins(), {"twin": layer}, 0, 0, C.RECT, None, before, "alpha")
    assert n >= 2000
    ref = G.sensor_window(0, layer, C.RECT, None, *before)
    v, u = np.meshgrid(np.linspace(0.02, 0.98, 40), np.linspace(0.02, 0.98, 40), indexing="ij")
    a = G.tex2d_linear(G.texel_rgba(0, layer), u, v)[..., 3]
    assert ((a > 0) & (a < 1)).any() and (a == 0).any() and (a == 1).any() and (ref[0][ref[3]] != fb[ref[3]]).any()


def test_camera_position_is_the_hosts():
    sc = C.scene()
    r = sc["lut_res"]
    for i in range(sc["n"]):
        cam = frustum(np.asarray(sc["cv_xyz"][i], np.float32).reshape(int(r[2]), int(r[1]), int(r[0]), 3))[1]
        assert np.abs(G.camera_position(G.frustum_corners(sc["cv_xyz"][i], r)) - cam).max() < 1e-5


def test_the_grid_buffer_is_float_data():
    assert (G.grid_axis(32) == (np.arange(32) + 0.5) / 32).all()           # dyadic: exact
    a = G.grid_axis(24)
    assert (a == a.astype(np.float32)).all() and np.abs(a - (np.arange(24) + 0.5) / 24).max() < 1e-7


# ---------------------------------------------------------------------- every case, the twins against the reference
@pytest.mark.parametrize("case", list(C.all_cpu_cases()), ids=lambda c: c[0].__name__ + " " + " ".join(str(a) for a in c[1]))
def test_case(case):
    f, args = case
    n, share = f(C.only_twins(), *args)
    print(f"{n} touched pixels compared, {share:.2%} excluded")


@pytest.mark.parametrize("kind, name", [("small", n) for n in C.SENSOR_CASES] + [("colour", "all types")])
def test_sensor_case(kind, name):
    C.sensor_case(C.only_twins(), lambda side, stream: C.oracle_layers(kind)[stream], name, kind)


def test_two_sensor_windows_over_a_drawn_frame():
    C.sensor_two_windows_case(C.only_twins(), lambda side, stream: C.oracle_layers("small")[stream])


def test_the_acceptance_rule_names_the_side_and_guards_untouched_pixels():
    eye, fb = C.LINE_CASES[0]
    mv, pr = C.matrices(eye)
    before = C.framebuffer(fb, eye)
    good = C.Twins().bbox(C.scene(), mv, pr, before)
    ref = C.bbox_reference(eye, fb)
    away = np.argwhere(~ref[3])[0]
    c = good[0].copy()
    c[tuple(away)] += np.float32(1e-3)                                     # a pixel the overlay must leave alone
    with pytest.raises(C.Mismatch, match="the kernel changes"):
        C.check("bbox", "x", ref, before, {"kernel": (c, good[1]), "twin": good})
    inner = np.argwhere(ref[3] & (ref[2] >= 1e-3).all(-1) & (ref[1] != before[1]))[0]
    d = good[1].copy()
    d[tuple(inner)] = before[1][tuple(inner)]                              # a drawn pixel not drawn
    with pytest.raises(C.Mismatch, match="the kernel disagrees"):
        C.check("bbox", "x", ref, before, {"kernel": (good[0], d), "twin": good})
