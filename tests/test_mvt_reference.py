"""CPU: known answers of the MVT reference (tests/mvt_reference.py) on hand-built depth images, and the proof that the kernel's tap
index clamp(g + k, 0, n - 1) (k_mvt.hip) is the literal fp32 NEAREST lookup of mvt_accum.vs:70 for every size used."""
import numpy as np
import pytest

import mvt_reference as M

F = np.float32
D = F(2.0)                                  # a depth whose multiples stay exact: constant windows filter to D exactly


def lq_of(border):
    return np.power(F(1.0) - F(border) / F(169.0), F(30.0))


def one(img):
    return M.vertex_stage(np.asarray(img, np.float32)[None])[0]


def test_constant_depth():
    v = one(np.full((24, 32), D))
    assert v.shape == (33, 25, 2)
    assert (v[..., 0] == D).all() and (v[..., 1] == F(1.0)).all()


def test_one_hole_in_the_window():
    img = np.full((24, 32), D)
    img[10, 10] = 0.0
    v = one(img)
    assert v[10, 13, 0] == D and v[10, 13, 1] == lq_of(1)                     # vertex (gx 13, gy 10): the hole is tap (-3, 0)
    assert v[10, 13, 1] == np.power(F(1.0) - F(1.0) / F(169.0), F(30.0))
    assert v[10, 10, 0] == 0.0 and v[10, 10, 1] == 0.0                        # the hole itself: is_outside -> (0, 0)
    assert v[10, 17, 0] == D and v[10, 17, 1] == F(1.0)                       # 7 columns away: outside the window


@pytest.mark.parametrize("step, rejected", [(0.10, False), (0.30, True)])
def test_depth_step_against_the_range_threshold(step, rejected):
    img = np.full((24, 32), D)
    img[:, 16:] = D + F(step)                                                 # threshold 0.35 * (2 / 4.5) = 0.156 m
    v = one(img)
    d, q = v[12, 12]                                                          # vertex (gx 12, gy 12): columns 16..18 of its window are across
    assert F(0.35) * (D / F(4.5)) == pytest.approx(0.1556, abs=1e-4)
    if rejected:
        assert d == D and q == lq_of(3 * 13)
    else:
        assert q == F(1.0) and abs(d - D) < F(step)
        assert d < D      # the across taps sit mostly past radius 6, where the spatial weight is negative: the result leaves [D, D + step]


@pytest.mark.parametrize("holes, cut", [(60, True), (59, False)])
def test_range_weight_cutoff(holes, cut):
    img = np.full((30, 40), D)
    taps = [(x, y) for y in range(-6, -1) for x in range(-6, 7)][:holes]      # rows -6 .. -2 of the window of vertex (gx 16, gy 12)
    for x, y in taps:
        img[12 + y, 16 + x] = 0.0
    d, q = one(img)[12, 16]
    assert F(169) * F(0.65) == F(109.85)
    assert q == lq_of(holes)
    assert (d == 0.0) if cut else (d == D)                                    # 109 vs 110 accepted taps, every range weight 1


def test_negative_corner_weights_cancel():
    """reject the 59 taps nearest the centre: 110 taps remain (the range weights pass the cut-off) but the spatial weights, negative
    for the 56 taps past radius 6, sum to <= 0 -> depth 0"""
    taps = sorted([(x, y) for y in range(-6, 7) for x in range(-6, 7) if (x, y) != (0, 0)], key=lambda t: (t[0] ** 2 + t[1] ** 2, t))
    gs = {t: F(1.0) - np.sqrt(F(t[0] ** 2 + t[1] ** 2)) * (F(1.0) / F(6.0)) for t in taps}
    assert sum(1 for t in taps if gs[t] < 0) == 56
    kept = [t for t in taps[59:]]
    w = F(1.0)
    for t in kept:
        w = F(w + gs[t])
    assert w <= 0.0
    img = np.full((30, 40), D)
    for x, y in taps[:59]:
        img[12 + y, 16 + x] = 0.0
    d, q = one(img)[12, 16]
    assert d == 0.0 and q == lq_of(59)


def test_vertex_past_the_image_edge_has_a_shifted_window():
    """W = 40 > H = 30: vertex rows gy 30 .. 40 lie below the image (v > 1); their clamped windows repeat the last rows"""
    rows = (F(2.0) + np.arange(30, dtype=np.float32) * F(0.002)).astype(np.float32)
    img = np.repeat(rows[:, None], 40, axis=1)
    v = one(img)
    assert v.shape == (41, 31, 2)
    assert (v[35:, 12] == v[35, 12]).all() and (v[35:, 12, 1] == F(1.0)).all()      # every tap on row 29
    assert v[35, 12, 0] == pytest.approx(rows[29], abs=1e-6)
    assert v[29, 12, 0] != v[35, 12, 0] and v[32, 12, 0] != v[35, 12, 0]            # no texel's own window: shifted


def test_tap_index_is_the_clamped_offset_for_every_size_used():
    """mvt_accum.vs:70 -- the fp32 coordinate u + float(k) * (1 / n) of a grid vertex, NEAREST-sampled -- is texel clamp(g + k, 0, n - 1),
    for every vertex index g the grids reach (g <= the other dimension) and every image size the tests and tools/mvt_timing.py use"""
    sizes = {(160, 120), (320, 240), (120, 160), (96, 128), (640, 480), (512, 424), (32, 24), (40, 30), (2048, 2048), (2048, 1536)}
    for W, H in sizes:
        for n, m in ((W, H), (H, W)):                                         # u: n = W, g <= H; v: n = H, g <= W
            g = np.arange(m + 1)
            u = M.grid_coord(g, n)
            for k in range(-6, 7):
                np.testing.assert_array_equal(M.nearest(M.tap_coord(u, k, n), n), np.clip(g + k, 0, n - 1), err_msg=f"{W}x{H} n={n} k={k}")
    for n in range(1, 2049):                                                  # and every size up to 2048, every vertex index up to 2048
        u = M.grid_coord(np.arange(2049), n)
        for k in range(-6, 7):
            assert np.array_equal(M.nearest(M.tap_coord(u, k, n), n), np.clip(np.arange(2049) + k, 0, n - 1)), (n, k)


def _plane_scene(W=64, H=64, z=-1.5, lut=8):
    """one sensor seeing the plane z = const: cv_xyz maps (u, v, d) -> (u - 0.5, 0.5 - v, z) (the grid's triangles then face the camera at the origin), cv_uv -> the same (u, v) squeezed into
    [0.05, 0.95]; colour constant"""
    r = np.arange(lut, dtype=np.float32) / F(lut - 1)
    xyz = np.zeros((lut, lut, lut, 3), np.float32)
    xyz[..., 0], xyz[..., 1], xyz[..., 2] = r[None, None, :] - F(0.5), F(0.5) - r[None, :, None], F(z)
    uv = np.zeros((lut, lut, lut, 2), np.float32)
    uv[..., 0], uv[..., 1] = F(0.05) + F(0.9) * r[None, None, :], F(0.05) + F(0.9) * r[None, :, None]
    return dict(n=1, cv_xyz=xyz[None], cv_uv=uv[None], bbox_min=[-1.0, -1.0, -2.0], bbox_max=[1.0, 1.0, 0.0],
                color=np.full((1, 16, 16, 3), 200, np.uint8)), np.full((1, H, W), D, np.float32)


def _image_to_eye(pr, view):
    s = np.diag([view[0] * 0.5, view[1] * 0.5, 0.5, 1.0])
    t = np.eye(4); t[:3, 3] = 1.0
    p = np.asarray(pr, np.float64).reshape(4, 4).T
    return np.linalg.inv(s @ t @ p).T.reshape(16).astype(np.float32)


def test_fronto_parallel_plane_is_covered_once_with_weight_one():
    scene, raw = _plane_scene()
    vtx = M.vertex_stage(raw)
    assert (vtx[..., 0] == D).all() and (vtx[..., 1] == F(1.0)).all()
    view = (64, 64)
    mv = np.eye(4, dtype=np.float32).reshape(16)
    f, n = 1.0, 10.0                                                          # glOrtho(-0.5, 0.5, -0.5, 0.5, 1, 10); cells 1/64 apart: inside min_length
    pr = np.array([2.0, 0, 0, 0, 0, 2.0, 0, 0, 0, 0, -2.0 / (n - f), 0, 0, 0, -(n + f) / (n - f), 1.0], np.float32)
    for mode in (3, 0):
        fc, fd = M.draw_mvt(scene, vtx, mv, pr, view, _image_to_eye(pr, view), shade_mode=mode)
        cov = fd < 1.0
        assert cov.sum() > 1000
        assert (fc[cov][:, 3] == 1.0).all() and (fc[~cov] == 0.0).all()
        want = M.CAMERA_COLORS[0] if mode == 3 else np.full(3, F(200) / F(255), np.float32)
        assert np.abs(fc[cov][:, :3] - want).max() <= 1e-6
        assert np.ptp(fd[cov]) < 1e-6                                         # one plane
    # covered once: the acc weight equals a single fragment's quality lateral_quality / depth = 1 / 2 -- seen through the
    # normalised alpha being exactly 1 above, and through the mesh: every covered pixel lies in exactly one triangle
    assert cov.sum() == pytest.approx(64 * 64 * (63 / 64) ** 2, rel=0.15)
