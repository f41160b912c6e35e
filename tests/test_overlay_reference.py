"""CPU: known answers of the overlay reference (tests/overlay_reference.py), each with hand-computed window coordinates, and its own
trilinear sampler against the oracle's."""
import numpy as np
import pytest

import overlay_reference as O
from oracle.oracle import tex3d

F = np.float32
ID = np.eye(4, dtype=np.float32).reshape(16)
BOX = (np.array([-1, -1, -1], np.float32), np.array([1, 1, 1], np.float32))


def clear_fb(view, depth=1.0):
    w, h = view
    return np.zeros((h, w, 4), np.float32), np.full((h, w), depth, np.float32)


def one_point(d, fb_d=1.0):
    """grid 1^3 -> p = (0.5, 0.5, 0.5) -> world (0, 0, 0) -> clip (0, 0, 0, 1) -> window (2.5, 2.5, 0.5) in a 5 x 5 view: pixel (2, 2)"""
    vol = np.full((2, 2, 2), d, np.float32)
    fc, fd = clear_fb((5, 5), fb_d)
    return O.draw_calibvis(vol, (1, 1, 1), *BOX, ID, ID, (5, 5), fc, fd)


@pytest.mark.parametrize("d, want", [
    (-0.01, None),                   # d <= -limit: discarded
    (-0.005, (0.0, 0.5, 0.0)),       # green, 1 - |d| / limit
    (0.0, (0.0, 1.0, 0.0)),          # d > 0 is false: green, inv = 0
    (0.005, (0.5, 0.0, 0.0)),        # red
    (0.01, (0.0, 0.0, 1.0)),         # d >= limit: blue
    (0.02, (0.0, 0.0, 1.0)),
])
def test_calibvis_colour_branches(d, want):
    ids, dd, ok, xw, yw, zw = O.calibvis_points(np.full((2, 2, 2), d, np.float32), (1, 1, 1), *BOX, ID, ID, (5, 5))
    assert dd[0] == F(d) and (xw[0], yw[0], zw[0]) == (F(2.5), F(2.5), F(0.5))
    fc, fd = one_point(d)
    others = np.ones((5, 5), bool)
    others[2, 2] = False
    assert (fd[others] == 1).all() and (fc[others] == 0).all()
    if want is None:
        assert fd[2, 2] == 1 and (fc[2, 2] == 0).all()
        return
    assert fd[2, 2] == F(0.5)
    np.testing.assert_allclose(fc[2, 2, :3], want, atol=1e-6)
    assert fc[2, 2, 3] == 1
    assert (fc[2, 2, :3] == 0).sum() == 2                                  # exactly one channel lit


def test_calibvis_depth_tie_with_the_framebuffer_is_not_drawn():
    fc, fd = one_point(0.005, fb_d=0.5)                                    # z == 0.5 == fb depth: GL_LESS fails
    assert fd[2, 2] == F(0.5) and (fc[2, 2] == 0).all()
    fc, fd = one_point(0.005, fb_d=np.nextafter(F(0.5), F(1)))              # one ulp deeper: drawn
    assert fd[2, 2] == F(0.5) and fc[2, 2, 0] > 0


@pytest.mark.parametrize("first, second, channel", [(0.005, -0.005, 0), (-0.005, 0.005, 1)])
def test_calibvis_depth_tie_between_points_lower_index_wins(first, second, channel):
    """grid 2 x 1 x 1: world x = -0.5 and 0.5; P = diag(1e-6, 1e-6, 1e-20, 1) puts both at window x = 2.5 -/+ 1.25e-6 (pixel 2) and z = 0.5"""
    pr = np.diag([1e-6, 1e-6, 1e-20, 1.0]).astype(np.float32).T.reshape(16)
    vol = np.zeros((2, 2, 2), np.float32)
    vol[:, :, 0], vol[:, :, 1] = first, second                            # the taps of u = 0.25 / 0.75 land exactly on texel 0 / 1
    ids, d, ok, xw, yw, zw = O.calibvis_points(vol, (2, 1, 1), *BOX, ID, pr, (5, 5))
    assert list(d) == [F(first), F(second)] and ok.all() and (zw == F(0.5)).all()
    assert xw[0] < F(2.5) < xw[1] and abs(xw - 2.5).max() < 1e-5
    fc, fd = O.draw_calibvis(vol, (2, 1, 1), *BOX, ID, pr, (5, 5), *clear_fb((5, 5)))
    assert fd[2, 2] == F(0.5) and fc[2, 2, channel] == pytest.approx(0.5, abs=1e-6) and fc[2, 2, 1 - channel] == 0
    assert (fd < 1).sum() == 1


def test_gl_less_keeps_the_first_of_equal_depths():
    fc, fd = clear_fb((2, 1))
    a, b = np.array([1, 0, 0, 1], np.float32), np.array([0, 1, 0, 1], np.float32)
    c, d = O.gl_less([(0, 0, F(0.5), a), (0, 0, F(0.5), b), (1, 0, F(0.7), a), (1, 0, F(0.6), b)], fc, fd)
    assert (c[0, 0] == a).all() and d[0, 0] == F(0.5)
    assert (c[0, 1] == b).all() and d[0, 1] == F(0.6)


def px(frags):
    return [(x, y) for x, y, _ in frags]


def test_line_horizontal_half_open_both_directions():
    # centres 1.5 2.5 3.5 4.5 lie in [1.5, 5.5): the start column is drawn, the end column is not
    assert px(O.window_line_fragments((1.5, 2.5, 0.5), (5.5, 2.5, 0.5), (8, 8))) == [(1, 2), (2, 2), (3, 2), (4, 2)]
    # the other way: centres in (1.5, 5.5]
    assert sorted(px(O.window_line_fragments((5.5, 2.5, 0.5), (1.5, 2.5, 0.5), (8, 8)))) == [(2, 2), (3, 2), (4, 2), (5, 2)]


def test_line_vertical_and_depth_interpolation():
    f = O.window_line_fragments((3.2, 0.5, 0.0), (3.2, 4.5, 1.0), (8, 8))
    assert px(f) == [(3, 0), (3, 1), (3, 2), (3, 3)]                       # y-major: rows 0..3, column floor(3.2)
    assert [z for _, _, z in f] == [F(0.0), F(0.25), F(0.5), F(0.75)]     # t = (row centre - 0.5) / 4


def test_line_45_degrees_is_x_major():
    assert px(O.window_line_fragments((0.5, 0.5, 0.5), (4.5, 4.5, 0.5), (8, 8))) == [(0, 0), (1, 1), (2, 2), (3, 3)]


def test_line_sub_pixel():
    assert O.window_line_fragments((2.1, 3.3, 0.5), (2.4, 3.4, 0.5), (8, 8)) == []         # no column centre in [2.1, 2.4)
    assert px(O.window_line_fragments((2.3, 3.3, 0.5), (2.7, 3.4, 0.5), (8, 8))) == [(2, 3)]   # centre 2.5 at y = 3.35
    assert O.window_line_fragments((2.3, 3.3, 0.5), (2.3, 3.3, 0.5), (8, 8)) == []         # zero length


def test_line_crossing_the_near_plane_is_clipped():
    # a = (-0.5, 0, -3, 1) is behind the near plane (z + w = -2), b = (0.5, 0, 1, 1) on the far plane: t = 0.5, a' = (0, 0, -1, 1)
    # window a' = (4, 4, 0), b = (6, 4, 1) in an 8 x 8 view: centres 4.5 and 5.5 at t = 0.25, 0.75
    f = O.line_fragments((-0.5, 0, -3, 1), (0.5, 0, 1, 1), (8, 8))
    assert f == [(4, 4, F(0.25)), (5, 4, F(0.75))]
    # unclipped it would start at window x = 2
    assert px(O.window_line_fragments((2.0, 4.0, 0.0), (6.0, 4.0, 1.0), (8, 8))) == [(2, 4), (3, 4), (4, 4), (5, 4)]


def test_line_wholly_outside():
    assert O.line_fragments((0, 0, -3, 1), (0.5, 0, -2, 1), (8, 8)) == []   # behind the near plane
    assert O.line_fragments((0, 0, 2, 1), (0.5, 0, 3, 1), (8, 8)) == []     # beyond the far plane
    assert O.line_fragments((2, 0, 0, 1), (3, 0, 0, 1), (8, 8)) == []       # window x 12 .. 16, right of the view


def test_camera_point_covers_3x3():
    assert O.point_pixels(F(2.5), F(2.5), 3, (5, 5)) == [(x, y) for y in (1, 2, 3) for x in (1, 2, 3)]
    assert O.point_pixels(F(0.2), F(4.9), 3, (5, 5)) == [(0, 3), (1, 3), (0, 4), (1, 4)]   # x in [ceil(-1.8), ceil(1.2) - 1], y in [3, 5], clipped by the view


def test_frustum_draw_order_and_colours():
    """one stream seen head-on: the camera point (drawn last, red) wins over nothing; lines are green"""
    corners = np.array([[-.5, -.5, -1], [-.5, .5, -1], [.5, .5, -1], [.5, -.5, -1], [-.5, -.5, 0], [-.5, .5, 0], [.5, .5, 0], [.5, -.5, 0]], np.float32)
    cam = np.array([0, 0, 0.5], np.float32)
    mv = ID
    pr = np.diag([1.0, 1.0, 0.5, 1.0]).astype(np.float32).T.reshape(16)
    fc, fd = O.draw_frustums([corners], [cam], mv, pr, (16, 16), *clear_fb((16, 16)))
    assert (fc[fd < 1][:, 3] == 1).all()
    red = (fc[..., 0] == 1) & (fc[..., 1] == 0)
    assert red.sum() == 9 and red[6:9, 6:9].all()                          # window (8, 8): pixels ceil(6) .. ceil(9) - 1
    green = (fc[..., 1] == 1) & (fc[..., 0] == 0)
    assert green.sum() > 20 and (fd[green] < 1).all()


def test_sampler_matches_the_oracle():
    rng = np.random.default_rng(7)
    vol = rng.standard_normal((5, 7, 6)).astype(np.float32)
    u = rng.uniform(-0.2, 1.2, (300, 3)).astype(np.float32)
    got = O.sample_tsdf(vol, u[:, 0], u[:, 1], u[:, 2])
    want = np.array([tex3d(vol[..., None], *p)[0] for p in u], np.float32)
    np.testing.assert_array_equal(got, want)
