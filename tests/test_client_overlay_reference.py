"""CPU: known answers of the bounding-box wireframe and texture-view reference (tests/client_overlay_reference.py)."""
import numpy as np

import client_overlay_reference as R
import overlay_reference as O

F = np.float32


def pix(frags):
    return sorted((px, py) for px, py, _ in frags)


def test_horizontal_width2_line_is_two_rows_half_open():
    got = pix(R.wide_window_line_fragments((10.5, 20.7, 0.5), (20.5, 20.7, 0.5), (64, 64)))
    assert got == sorted([(i, 20) for i in range(10, 20)] + [(i, 21) for i in range(10, 20)])   # column 20 (centre 20.5 = end) excluded
    back = pix(R.wide_window_line_fragments((20.5, 20.7, 0.5), (10.5, 20.7, 0.5), (64, 64)))
    assert back == sorted([(i, 20) for i in range(11, 21)] + [(i, 21) for i in range(11, 21)])  # reversed: start 20.5 in, end 10.5 out


def test_vertical_width2_line_is_two_columns():
    got = pix(R.wide_window_line_fragments((30.2, 5.5, 0.5), (30.2, 15.5, 0.5), (64, 64)))
    assert got == sorted([(29, y) for y in range(5, 15)] + [(30, y) for y in range(5, 15)])    # x - 0.5 = 29.7: columns 29 and 30


def test_diagonal_width2_line_is_x_major_columns_of_two():
    got = pix(R.wide_window_line_fragments((4.0, 4.0, 0.25), (20.0, 20.0, 0.75), (64, 64)))
    assert got == sorted([(i, i) for i in range(4, 20)] + [(i, i + 1) for i in range(4, 20)])   # |dx| == |dy|: x-major, y - 0.5 = i exactly


def test_replicas_are_clipped_one_by_one():
    got = pix(R.wide_window_line_fragments((2.5, 0.2, 0.5), (6.5, 0.2, 0.5), (64, 64)))
    assert got == [(i, 0) for i in range(2, 6)]                              # row -1 dropped, row 0 kept
    got = pix(R.wide_window_line_fragments((2.5, 63.9, 0.5), (6.5, 63.9, 0.5), (64, 64)))
    assert got == [(i, 63) for i in range(2, 6)]                             # row 63 kept, row 64 dropped


def test_width1_walk_is_overlay_reference_walk():
    rng = np.random.default_rng(5)
    for _ in range(200):
        a = (rng.uniform(-5, 70), rng.uniform(-5, 50), rng.uniform(0, 1))
        b = (rng.uniform(-5, 70), rng.uniform(-5, 50), rng.uniform(0, 1))
        assert R.wide_window_line_fragments(a, b, (64, 48), width=1) == O.window_line_fragments(a, b, (64, 48))


HEAD_ON = dict(bmin=(-0.5, -0.5, -0.5), bmax=(0.5, 0.5, 0.5), mv=np.eye(4, dtype=np.float32).reshape(16),
               pr=np.diag([1.0, 1.0, -0.5, 1.0]).astype(np.float32).reshape(16), view=(64, 48))


def test_head_on_box_is_a_two_pixel_outline():
    """front and back squares land on x 16..48, y 12..36; the depth edges are single points (no fragment).  Horizontal edges: rows 11-12 and
    35-36 over columns 16..47 (64 + 64), vertical ones: columns 15-16 and 47-48 over rows 12..35 (48 + 48), 4 pixels shared: 220"""
    H = HEAD_ON
    fc = np.zeros((48, 64, 4), np.float32)
    fd = np.ones((48, 64), np.float32)
    c, d = R.draw_bbox(H["bmin"], H["bmax"], H["mv"], H["pr"], H["view"], fc, fd)
    drawn = d < 1
    assert drawn.sum() == 220
    assert (d[drawn] == F(0.375)).all()                                     # the front square (z = 0.5 -> 0.375) beats the back one (0.625)
    assert (c[drawn] == R.BBOX_COLOR).all() and (c[~drawn] == 0).all()
    assert drawn[11, 16:48].all() and drawn[12, 16:48].all() and drawn[35, 16:48].all() and drawn[36, 16:48].all()
    assert drawn[12:36, 15].all() and drawn[12:36, 16].all() and drawn[12:36, 47].all() and drawn[12:36, 48].all()


def test_box_edge_drawn_twice_keeps_the_first_segment():
    H = HEAD_ON
    segs = R.bbox_segments(H["bmin"], H["bmax"])
    assert len(segs) == 24 and segs[0] == ([F(-0.5), F(-0.5), F(0.5)], [F(0.5), F(-0.5), F(0.5)])
    assert segs[22] == (segs[0][1], segs[0][0])                             # the bottom loop walks the front bottom edge backwards
    frags = R.bbox_fragments(H["bmin"], H["bmax"], H["mv"], H["pr"], H["view"])
    at = [(s, z) for s, px, py, z in frags if (px, py) == (20, 11)]
    assert (0, F(0.375)) in at and (22, F(0.375)) in at
    win = R.bbox_winners(H["bmin"], H["bmax"], H["mv"], H["pr"], H["view"], np.ones((48, 64), np.float32))
    assert win[11, 20] == 0 and win[12, 30] == 0


def test_viewport_of_the_blit():
    assert R.blit_viewport(1280, 720) == (960, 360)
    assert R.blit_viewport(160, 90) == (120, 45)
    assert R.blit_viewport(161, 91) == (120, 45)                            # 1.5f * 161 = 241.5 -> 241, / 2 = 120.5 -> 120


def test_blit_of_a_block_constant_atlas_is_exact():
    rng = np.random.default_rng(7)
    blocks = rng.uniform(-1, 2, (360, 960, 4)).astype(np.float32)
    atlas = np.repeat(np.repeat(blocks, 2, axis=0), 2, axis=1)              # 720 x 1920: 2 x 2 blocks
    fc = np.full((720, 1280, 4), 0.25, np.float32)
    out = R.blit(atlas, (1280, 720), fc)
    np.testing.assert_array_equal(out[:360, :960, :3], blocks[..., :3])
    assert (out[:360, :960, 3] == 1).all()
    assert (out[360:] == 0.25).all() and (out[:, 960:] == 0.25).all()


def test_blit_of_a_full_size_image_matches_a_hand_tap():
    rng = np.random.default_rng(9)
    src = rng.uniform(0, 1, (720, 1280, 4)).astype(np.float32)
    out = R.blit(src, (1280, 720), np.zeros((720, 1280, 4), np.float32))
    for x, y in [(0, 0), (959, 359), (123, 45), (500, 200)]:
        u = (F(x) + F(0.5)) / F(960)
        v = (F(y) + F(0.5)) / F(360)
        fx, fy = u * F(1280) - F(0.5), v * F(720) - F(0.5)
        ix, iy = int(np.floor(fx)), int(np.floor(fy))
        ax, ay = F(fx - F(ix)), F(fy - F(iy))
        i0, i1 = min(max(ix, 0), 1279), min(max(ix + 1, 0), 1279)
        j0, j1 = min(max(iy, 0), 719), min(max(iy + 1, 0), 719)
        lerp = lambda a, b, t: F(a + F(F(b - a) * t))
        for k in range(3):
            want = lerp(lerp(src[j0, i0, k], src[j0, i1, k], ax), lerp(src[j1, i0, k], src[j1, i1, k], ax), ay)
            assert out[y, x, k] == want, (x, y, k)
        assert out[y, x, 3] == 1
    assert (out[360:] == 0).all() and (out[:, 960:] == 0).all()
