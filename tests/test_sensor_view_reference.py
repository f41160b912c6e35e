"""CPU: tests/sensor_view_reference.py (the definition of tsdf_draw_sensor_texture in include/rgbd_recon_hip.h) against answers worked out
by hand: the direction of the quarter turn and the row flip, the fp32 cosine that is not zero, the blend, the scissor box, coverage."""
import numpy as np

import sensor_view_reference as S

F = np.float32


def test_the_rotation_constants_are_the_fp32_cosine_and_sine_of_fp32_radians_90():
    r = np.radians(F(90.0)).astype(np.float32)
    assert r == F(1.5707964) and r.dtype == np.float32
    assert S.ROT_C.view(np.uint32) == 0xb33bbd2e and S.ROT_C == F(-4.37113883e-08) and S.ROT_C != 0
    assert F(np.cos(np.float64(r))) == S.ROT_C and F(np.sin(np.float64(r))) == S.ROT_S == F(1)


def test_quarter_turn_and_row_flip_pixel_by_pixel():
    """a 4 x 2 source under a quad of exactly its (turned) size, 2 wide and 4 high, filling a 2 x 4 view.  Pixel (i, j) -- GL row j, so ImGui
    y = 4 - (j + .5) -- has Frag_UV ((i + .5) / 2, (3.5 - j) / 4); turned, u' = v and v' = 1 - u: texel x = 3 - j, texel y = 1 - i."""
    src = np.array([[10, 11, 12, 13], [20, 21, 22, 23]], np.float32)      # src[y][x]
    fb = np.full((4, 2, 4), 7, np.float32)
    want = np.array([[23, 13], [22, 12], [21, 11], [20, 10]], np.float32)  # want[j][i]
    for i in range(2):
        for j in range(4):
            assert want[j, i] == src[1 - i, 3 - j]
    out = S.draw(5, src, (0, 0, 2, 4), None, fb)                           # NEAREST, (L, L, L, 1)
    assert (out[..., 0] == want).all() and (out[..., 1] == want).all() and (out[..., 2] == want).all() and (out[..., 3] == 1).all()
    lin = S.draw(4, src, (0, 0, 2, 4), None, fb)                           # LINEAR at texel centres, (r, 0, 0, 1)
    assert np.abs(lin[..., 0] - want).max() <= 1e-5 and (lin[..., 1:3] == 0).all() and (lin[..., 3] == 1).all()
    # in words: the source's first row (y = 0) is the window's RIGHT column, and the source's left end (x = 0) the window's TOP (GL row 3)
    assert (out[3, 1, 0], out[0, 1, 0], out[3, 0, 0]) == (10, 13, 20)


def test_the_seven_texel_rules():
    rgb = np.array([[[255, 0, 51]]], np.uint8)
    assert (S.texel_vec4(0, rgb)[0, 0] == np.array([1, 0, F(51) / F(255), 1], np.float32)).all()
    rgba = np.array([[[255, 0, 51, 128]]], np.uint8)
    assert (S.texel_vec4(0, rgba)[0, 0] == np.array([1, 0, F(51) / F(255), F(128) / F(255)], np.float32)).all()
    assert (S.texel_vec4(1, np.array([[[2.5, -1.0]]], np.float32))[0, 0] == [2.5, -1, 0, 1]).all()
    assert (S.texel_vec4(1, np.array([[2.5]], np.float32))[0, 0] == [2.5, 0, 0, 1]).all()
    assert (S.texel_vec4(2, np.array([[0.25]], np.float32))[0, 0] == [0.25, 0.25, 0.25, 1]).all()
    assert (S.texel_vec4(3, np.array([[[0.1, -0.2, 0.3]]], np.float32))[0, 0] == np.array([0.1, -0.2, 0.3, 1], np.float32)).all()
    assert (S.texel_vec4(4, np.array([[0.75]], np.float32))[0, 0] == [0.75, 0, 0, 1]).all()
    assert (S.texel_vec4(5, np.array([[3.5]], np.float32))[0, 0] == [3.5, 3.5, 3.5, 1]).all()
    assert (S.texel_vec4(6, np.array([[[50, -20, 30]]], np.float32))[0, 0] == [50, -20, 30, 1]).all()
    assert S.NEAREST == {1, 5}


def test_the_cosine_moves_one_nearest_pick_at_a_texel_border():
    """4 wide x 5 high quad over a 4-texel-wide source: the pixel row with ImGui y = 2.5 has v = 0.5 exactly, the border between texel
    columns 1 and 2.  u' = c * (u - .5) + (v - .5) + .5: at cx = 3.5, u - .5 = .375 and c * .375 = -1.64e-8 is more than half an ulp below
    0.5 (1.49e-8), so u' = 0.49999997 and the pick is column 1; c = 0 gives 0.5 and column 2.  At cx = 2.5 (c * .125 = -5.5e-9) nothing moves."""
    src = np.arange(8, dtype=np.float32).reshape(2, 4)                      # src[y][x] = 4 y + x
    fb = np.zeros((5, 4, 4), np.float32)
    rect = (0, 0, 4, 5)
    with_c = S.draw(5, src, rect, None, fb)[..., 0]
    with_0 = S.draw(5, src, rect, None, fb, c=F(0))[..., 0]
    diff = np.argwhere(with_c != with_0)
    assert [tuple(x) for x in diff] == [(2, 3)]                             # GL row 2 is ImGui y = 5 - 2.5 = 2.5; column 3 is cx = 3.5
    u, v = S.rotate(np.array([F(3.5) / F(4)]), np.array([F(0.5)]))
    assert u[0] == np.nextafter(F(0.5), F(0)) and S.axis_nearest(u, 4)[0] == 1
    # cx = 3.5: v' = 1 - 0.875 = 0.125 -> source row 0
    assert with_c[2, 3] == 1 and with_0[2, 3] == 2
    assert with_c[2, 2] == with_0[2, 2] == 2


def test_blend_of_a_dxt_style_source_over_a_random_framebuffer():
    """alpha 0, 0.5 (128 / 255 is not 0.5: use a float source through the blend itself) and 1"""
    rng = np.random.default_rng(3)
    d = rng.uniform(-2, 2, (3, 1, 4)).astype(np.float32)
    s = np.array([[[0.2, 0.4, 0.6, 0.0]], [[0.2, 0.4, 0.6, 0.5]], [[0.2, 0.4, 0.6, 1.0]]], np.float32)
    out = S.blend(s, d)
    assert (out[0] == d[0]).all()                                          # s * 0 + d * 1
    for ch in range(4):
        assert out[1, 0, ch] == F(F(s[1, 0, ch] * F(0.5)) + F(d[1, 0, ch] * F(0.5)))
    assert out[1, 0, 3] == F(F(0.25) + F(d[1, 0, 3] * F(0.5)))             # alpha blends like a colour: a * a + d.a * (1 - a)
    assert (out[2] == s[2]).all()
    # through draw(): an RGBA8 layer whose alpha byte is 0 / 128 / 255, NEAREST-like (a 1 x 1 source: every tap is the one texel)
    for byte in (0, 128, 255):
        layer = np.array([[[51, 102, 153, byte]]], np.uint8)
        fb = rng.uniform(0, 1, (2, 2, 4)).astype(np.float32)
        got = S.draw(0, layer, (0, 0, 2, 2), None, fb)
        a = F(byte) / F(255)
        sv = np.array([F(51) / F(255), F(102) / F(255), F(153) / F(255), a], np.float32)
        want = sv if byte == 255 else (sv * a + fb * (F(1) - a)).astype(np.float32)
        assert (got == want).all()


def test_nan_and_inf_underneath_do_not_leak_through_an_opaque_sample():
    src = np.array([[0.5]], np.float32)
    fb = np.full((2, 2, 4), np.nan, np.float32)
    fb[0, 0] = np.inf
    out = S.draw(2, src, (0, 0, 2, 2), None, fb)
    assert (out == np.array([0.5, 0.5, 0.5, 1], np.float32)).all()
    # ... and do where alpha < 1, as GL's blend would
    half = np.array([[[255, 255, 255, 0]]], np.uint8)
    under = S.draw(0, half, (0, 0, 2, 2), None, fb)                        # alpha 0: s * 0 + d * 1
    assert np.isinf(under[0, 0]).all() and np.isnan(under[0, 1]).all() and np.isnan(under[1]).all()


def test_clip_rect_cuts_the_quad():
    """view 8 x 6, quad columns 1..6 and ImGui rows 1..5; ClipRect (2, 2, 5, 4): scissor x = 2, y = (int)(6 - 4) = 2, 3 wide, 2 high"""
    assert S.scissor_box((2, 2, 5, 4), (8, 6)) == (2, 2, 3, 2)
    assert S.scissor_box((2.9, 1.5, 5.2, 4.75), (8, 6)) == (2, 1, 2, 3)    # (int)2.9, (int)(6 - 4.75), (int)2.3, (int)3.25
    fb = np.zeros((6, 8, 4), np.float32)
    out = S.draw(2, np.ones((2, 2), np.float32), (1, 1, 7, 5), (2, 2, 5, 4), fb)
    want = np.zeros((6, 8), bool)
    want[2:4, 2:5] = True
    assert ((out[..., 3] == 1) == want).all() and (out[~want] == 0).all()
    # an empty or negative box draws nothing
    assert (S.draw(2, np.ones((2, 2), np.float32), (1, 1, 7, 5), (5, 2, 2, 4), fb) == fb).all()
    # without a clip rect: GL rows j with 1 <= 6 - (j + .5) < 5, that is j = 1 .. 4; columns 1 .. 6
    full = S.draw(2, np.ones((2, 2), np.float32), (1, 1, 7, 5), None, fb)
    want = np.zeros((6, 8), bool)
    want[1:5, 1:7] = True
    assert ((full[..., 3] == 1) == want).all()


def test_quad_partly_outside_the_view():
    """the part inside is what the whole quad would show there: Frag_UV does not depend on the view's edge"""
    src = np.arange(12, dtype=np.float32).reshape(3, 4)
    big = S.draw(5, src, (6, 5, 14, 15), None, np.zeros((20, 20, 4), np.float32))
    small = S.draw(5, src, (6 - 4, 5 - 10, 14 - 4, 15 - 10), None, np.zeros((8, 8, 4), np.float32))   # the view is the window [4, 12) x [10, 18) of the big one
    # ImGui y of the big view's row j is 20 - (j + .5); the small view shows ImGui rows 10 .. 18 of it = GL rows 2 .. 9
    assert (small == big[2:10, 4:12]).all()
    assert (small[..., 3] == 1).sum() == 6 * 5                              # columns 2 .. 7, ImGui rows 0 .. 4
    wholly_out = S.draw(5, src, (-9, -9, -1, -1), None, np.zeros((8, 8, 4), np.float32))
    assert (wholly_out == 0).all()


def test_fractional_corners():
    """p_min = (1.5, 0.75), p_max = (4.25, 3.5) in a 6 x 4 view: centres cx = 1.5 (on p_min: inside), 2.5, 3.5 (4.5 >= 4.25: outside); cy = 0.5
    (outside), 1.5, 2.5 (3.5 is p_max: outside) = GL rows 2 and 1"""
    rect = (1.5, 0.75, 4.25, 3.5)
    mask, cx, cy = S.coverage(rect, None, (6, 4))
    want = np.zeros((4, 6), bool)
    want[1:3, 1:4] = True
    assert (mask == want).all()
    u, v = S.frag_uv(rect, cx, cy)
    assert u[0, 1] == 0 and u[0, 2] == F(1) / F(2.75) and v[2, 0] == F(0.75) / F(2.75) and v[1, 0] == F(1.75) / F(2.75)
    src = np.arange(6, dtype=np.float32).reshape(2, 3)                      # 3 wide, 2 high
    out = S.draw(5, src, rect, None, np.zeros((4, 6, 4), np.float32))[..., 0]
    # u' = v, v' = 1 - u: GL row 2 (v = .2727) -> texel x 0, row 1 (v = .636) -> x 1; column 1 (u = 0) -> v' = 1 -> y 1, columns 2, 3 (u = .36, .73) -> y 1, 0
    assert (out[2, 1:4] == [3, 3, 0]).all() and (out[1, 1:4] == [4, 4, 1]).all()


def test_view_size_is_the_clients():
    assert S.view_size(480, (640, 480)) == (480, 640)
    w, h = S.view_size(100, (512, 424))
    assert w == 100 and h == F(100) / (F(424) / F(512))
