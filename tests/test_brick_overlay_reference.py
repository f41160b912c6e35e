"""CPU: known answers that pin tests/brick_overlay_reference.py, the numpy definition the GPU overlay (tsdf_draw_bricks) is compared with
bit for bit, and the vectorised form against the literal one (overlay_reference.line_fragments + the in-order GL_LESS loop)."""
import numpy as np

import brick_overlay_reference as B
import rgbd_recon_amd as rr

F = np.float32
VIEW = (16, 16)
RES = (2, 2, 2)
SIZE = (1.0, 1.0, 1.0)
BMIN = (0.0, 0.0, 0.0)
MV = np.eye(4, dtype=np.float32).reshape(16)
# orthographic, looking down -z: window x = 2.5 + 4 * world x (y alike) in a 16 x 16 view, window z = 0.5 - 0.125 * world z.  Every
# coefficient is a dyadic fraction, so the brick corners land exactly on pixel centres.
ORTHO = np.zeros(16, np.float32)
ORTHO[0], ORTHO[5], ORTHO[10], ORTHO[12], ORTHO[13], ORTHO[15] = 0.5, 0.5, -0.25, -0.6875, -0.6875, 1.0
Z_FRONT, Z_BACK = F(0.375), F(0.5)


def clean():
    return np.zeros((VIEW[1], VIEW[0], 4), np.float32), np.ones((VIEW[1], VIEW[0]), np.float32)


def both(ids, mv=MV, pr=ORTHO, res=RES, size=SIZE, bmin=BMIN, view=VIEW, fb=None):
    """the vectorised result, after checking it against the literal one"""
    fc, fd = clean() if fb is None else fb
    c, d = B.draw_bricks(np.asarray(ids, np.int64), res, size, bmin, mv, pr, view, fc, fd)
    lc, ld = B.draw_bricks_literal(np.asarray(ids, np.int64), res, size, bmin, mv, pr, view, fc, fd)
    assert (c == lc).all() and (d == ld).all()
    return c, d


def test_one_brick_orthographic_outline_by_hand():
    """corners at window 2.5 and 6.5: a segment's start pixel is drawn, its end pixel is not (diamond exit).  Front face (z = 1): v0 -> v1
    leftwards in row 6 covers columns 3..6, v0 -> v4 downwards in column 6 rows 3..6, v5 -> v1 upwards in column 2 rows 2..5, v5 -> v4
    rightwards in row 2 columns 2..5: the ring without (2, 6) and (6, 2).  The back face's segments run the other way and add exactly those
    two pixels, at the back depth.  The four segments along z project to points and make no fragment."""
    c, d = both([0])
    want = np.ones((16, 16), np.float32)
    for k in range(2, 7):
        want[2, k] = want[6, k] = want[k, 2] = want[k, 6] = Z_FRONT
    want[6, 2] = want[2, 6] = Z_BACK                                   # [row][column]: pixels (2, 6) and (6, 2)
    assert (d == want).all()
    assert (c[want < 1] == B.WIRE_COLOR).all() and (c[want == 1] == 0).all()


def test_shuffling_the_id_list_changes_nothing():
    ids = np.arange(8)
    a = both(ids)
    rng = np.random.default_rng(3)
    for _ in range(3):
        b = B.draw_bricks(rng.permutation(ids), RES, SIZE, BMIN, MV, ORTHO, VIEW, *clean())
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    flags = np.ones(8, np.uint8)
    b = B.draw_bricks(flags, RES, SIZE, BMIN, MV, ORTHO, VIEW, *clean())
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


def test_shared_face_edges_go_to_the_lower_id():
    """bricks 0 and 1 share the face x = 1: brick 0 draws its front edge there as segment 2 (v0 -> v4, rows 3..6 of column 6), brick 1 as
    segment 3 (v5 -> v1, rows 2..5), both at the front depth"""
    win, d, st = B.brick_winners(np.array([0, 1]), RES, SIZE, BMIN, MV, ORTHO, VIEW, clean()[1])
    assert [int(win[r, 6]) for r in (3, 4, 5)] == [2, 2, 2]
    assert int(win[6, 6]) == 0                                            # the corner pixel: brick 0's own segment 0 (v0 -> v1) starts there too
    assert int(win[2, 6]) == 12 + 3                                       # only brick 1 reaches row 2 at the front depth
    assert (d[2:7, 6] == Z_FRONT).all()
    assert st["tie_pixels"] >= 3
    both([0, 1])


def test_strict_depth_test_and_untouched_pixels():
    fc, fd = clean()
    fc[...] = 0.25
    fd[2, 3] = Z_FRONT                                                    # equal: GL_LESS fails
    fd[2, 4] = np.nextafter(Z_FRONT, F(1))                                # one ulp behind: passes
    c, d = both([0], fb=(fc, fd))
    assert d[2, 3] == Z_FRONT and (c[2, 3] == 0.25).all()
    assert d[2, 4] == Z_FRONT and (c[2, 4] == B.WIRE_COLOR).all()
    assert (c[0, 0] == 0.25).all() and d[0, 0] == 1


def persp(eye, target, near=0.5, fov=60.0, view=(64, 48)):
    return (rr.scene.gl_flat(rr.scene.look_at(eye, target)), rr.scene.gl_flat(rr.scene.perspective(fov, view[0] / float(view[1]), near, 50.0)), view)


def test_near_plane_clips_a_straddling_brick_and_drops_one_behind_the_eye():
    res, size, bmin = (1, 1, 4), (0.3, 0.3, 1.0), (-0.15, -0.15, 0.0)
    mv, pr, view = persp((0.0, 0.0, 2.7), (0.0, 0.0, 0.0), near=0.5)     # the eye inside brick 2 (z in [2, 3]), looking down -z: near plane at z = 2.2
    clip = B.vertex_clip(np.array([0, 1, 2, 3]), res, size, bmin, mv, pr)
    inside = clip[2] + clip[3] >= 0                                       # [brick][vertex]: in front of the near plane
    assert inside[0].all() and inside[1].all()
    assert inside[2].any() and not inside[2].all()                        # straddles it
    assert not inside[3].any()                                            # wholly behind the eye
    fc, fd = np.zeros((view[1], view[0], 4), np.float32), np.ones((view[1], view[0]), np.float32)
    for i, drawn in ((1, True), (2, True), (3, False)):
        prim, px, py, z = B.brick_fragments(np.array([i]), res, size, bmin, mv, pr, view)
        assert (prim.size > 0) == drawn
        assert ((px >= 0) & (px < view[0]) & (py >= 0) & (py < view[1]) & (z >= 0) & (z <= 1)).all()
        c, d = B.draw_bricks(np.array([i]), res, size, bmin, mv, pr, view, fc, fd)
        lc, ld = B.draw_bricks_literal(np.array([i]), res, size, bmin, mv, pr, view, fc, fd)
        assert (c == lc).all() and (d == ld).all()
    _, _, _, z2 = B.brick_fragments(np.array([2]), res, size, bmin, mv, pr, view)
    assert z2.min() < 0.1 and z2.max() > 0.25                             # the segments along z run from the face at z = 2 towards the cut at the near plane (depth 0)


def test_last_brick_of_an_axis_is_drawn_at_full_size():
    """a box of 1.5 bricks along x: brick 1 spans x in [1, 2] although the box ends at 1.5 (window 8.5): its right edge is column 10"""
    c, d = both([1])
    assert d[4, 10] == Z_FRONT and d[2, 9] == Z_FRONT
    assert (d[:, 11:] == 1).all()


def test_empty_list_leaves_the_framebuffer_untouched():
    rng = np.random.default_rng(5)
    fc = rng.uniform(0, 1, (16, 16, 4)).astype(np.float32)
    fd = rng.uniform(0, 1, (16, 16)).astype(np.float32)
    for ids in (np.zeros(0, np.int64), np.zeros(8, np.uint8)):
        c, d = B.draw_bricks(ids, RES, SIZE, BMIN, MV, ORTHO, VIEW, fc, fd)
        assert (c == fc).all() and (d == fd).all()
    lc, ld = B.draw_bricks_literal(np.zeros(8, np.uint8), RES, SIZE, BMIN, MV, ORTHO, VIEW, fc, fd)
    assert (lc == fc).all() and (ld == fd).all()


def test_vectorised_equals_literal_on_a_perspective_grid_over_random_depth():
    res, size, bmin = (3, 4, 3), (0.4, 0.3, 0.5), (-0.6, 0.0, -0.7)
    rng = np.random.default_rng(9)
    ids = np.flatnonzero(rng.uniform(size=36) < 0.6)
    for eye in ((1.5, 1.4, 2.0), (0.05, 0.5, 0.1), (-2.0, 0.2, 0.3)):
        mv, pr, view = persp(eye, (0.0, 0.6, 0.0), near=0.2)
        fd = rng.uniform(0.8, 1.0, (view[1], view[0])).astype(np.float32)
        fc = np.zeros((view[1], view[0], 4), np.float32)
        st = {}
        c, d = B.draw_bricks(ids, res, size, bmin, mv, pr, view, fc, fd, stats=st)
        lc, ld = B.draw_bricks_literal(ids, res, size, bmin, mv, pr, view, fc, fd)
        assert (c == lc).all() and (d == ld).all()
        assert st["changed"] >= st["bricks"] and st["failed"] > 0
