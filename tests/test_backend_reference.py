"""No GPU: the oracle's point, triangle-grid and MVT draws against the float64 reference of tests/backend_reference.py, under the acceptance
rule of tests/backend_cases.py, and properties of that reference itself on inputs made by hand.  tests/test_gpu_backends.py holds the
kernels to the same reference on the same cases."""
import numpy as np
import pytest

import backend_cases as C
import backend_reference as B
import main_path_cases as MC

VIEW = (16, 16)                 # powers of two: window coordinates with a few fraction bits are exact in clip space and back


def clip_of_window(xy, z=0.5, w=1.0):
    """clip coordinates whose window position in VIEW is xy (pixels) at window depth z"""
    xy = np.asarray(xy, np.float64)
    return np.concatenate([(xy / VIEW * 2.0 - 1.0) * w, np.full((len(xy), 1), (z * 2.0 - 1.0) * w), np.full((len(xy), 1), w)], -1)


def coverage(r):
    m = np.zeros((VIEW[1], VIEW[0]), int)
    if r is not None:
        m[r["rows"], r["cols"]] += r["covered"]
    return m


@pytest.mark.parametrize("corners", [[(2.5, 2.5), (9.5, 2.5), (2.5, 9.5), (9.5, 9.5)],        # the diagonal runs through pixel centres
                                     [(2.0, 3.0), (11.0, 2.0), (3.0, 10.0), (12.0, 9.0)],
                                     [(9.5, 2.5), (2.5, 2.5), (9.5, 9.5), (2.5, 9.5)]],       # mirrored: the other winding
                         ids=["through centres", "skew", "mirrored"])
def test_two_triangles_of_a_cell_share_their_edge_without_gap_or_overlap(corners):
    v00, v10, v01, v11 = corners
    a, b = (coverage(B.rasterise(clip_of_window(t), VIEW)) for t in ((v00, v10, v01), (v10, v11, v01)))      # recon_trigrid.cpp:53-59
    quad = coverage(B.rasterise(clip_of_window((v00, v10, v11)), VIEW)) + coverage(B.rasterise(clip_of_window((v00, v11, v01)), VIEW))
    assert (a + b).max() == 1 and (a + b).sum() > 30
    if corners[0][1] == corners[1][1]:                       # the axis-aligned square: the pixel centres in [2.5, 9.5) x [2.5, 9.5), top-left rule
        want = np.zeros_like(a)
        want[3:10, 2:9] = 1                                  # centres y = 3.5 .. 9.5 (the top edge owns its centres), x = 2.5 .. 8.5 (the left edge does)
        np.testing.assert_array_equal(a + b, want)
    np.testing.assert_array_equal(a + b, quad)               # the other diagonal splits the same pixels


@pytest.mark.parametrize("size", [1, 3, 7, 21])
def test_an_odd_sprite_on_a_pixel_centre_covers_size_squared_pixels(size):
    x0, x1, y0, y1 = B.sprite_pixels(40.5, 30.5, float(size), (96, 54))
    assert (x1 - x0, y1 - y0) == (size, size) and (x0 + x1, y0 + y1) == (81, 61)
    x0, x1, y0, y1 = B.sprite_pixels(40.0, 30.0, 2.0, (96, 54))          # an even one between centres: [39, 41) holds the centres 39.5 and 40.5
    assert (x0, x1, y0, y1) == (39, 41, 29, 31)
    assert B.sprite_pixels(40.0, 30.0, 1.0, (96, 54)) == (39, 40, 29, 30)  # c - s/2 <= p < c + s/2: 39.5 is in, 40.5 is out


def test_clipping_a_triangle_wholly_in_front_changes_nothing():
    tri = clip_of_window([(2.3, 1.7), (13.1, 4.2), (6.4, 10.9)]) * np.array([[1.0], [2.5], [0.7]])           # three different w, all inside near / far
    r = B.rasterise(tri, VIEW)
    assert not r["clipped"] and r["covered"].sum() > 20
    x, y = np.meshgrid(np.arange(VIEW[0]) + 0.5, np.arange(VIEW[1]) + 0.5)
    win = np.array([(2.3, 1.7), (13.1, 4.2), (6.4, 10.9)])
    e = lambda p, q: (q[0] - p[0]) * (y - p[1]) - (q[1] - p[1]) * (x - p[0])
    inside = (e(win[0], win[1]) > 0) & (e(win[1], win[2]) > 0) & (e(win[2], win[0]) > 0)                     # (no centre lies on an edge)
    np.testing.assert_array_equal(coverage(r).astype(bool), inside)
    np.testing.assert_allclose(r["z"][r["covered"]], 0.5, atol=1e-12)                                        # the plane z = 0.5
    lam = r["lam"][r["covered"]]
    assert np.abs(lam.sum(-1) - 1).max() < 1e-12 and lam.min() > 0
    w = np.array([1.0, 2.5, 0.7])                            # perspective-correct: lam w / sum(lam w) are the window-space barycentrics
    scr = lam * w / (lam * w).sum(-1, keepdims=True)
    ys, xs = np.nonzero(r["covered"])
    np.testing.assert_allclose(scr @ win, np.stack([xs + r["x0"] + 0.5, ys + r["y0"] + 0.5], -1), atol=1e-9)


def test_a_triangle_across_the_eye_plane_keeps_its_visible_part():
    """two vertices in front, one behind the eye: the part in front of the near plane is drawn, with the varyings of the whole triangle"""
    proj = B.R.mat(C.S.gl_flat(C.S.perspective(90.0, VIEW[0] / float(VIEW[1]), 0.1, 10.0)))
    eye = np.array([(-0.4, -0.3, -1.0), (0.5, -0.2, -1.0), (0.1, 0.4, 0.5)])            # the third one behind the eye
    r = B.rasterise(B.R._xf(proj, eye), VIEW)
    assert r["clipped"] and r["covered"].sum() > 10
    pos = r["lam"][r["covered"]] @ eye                                                  # every fragment lies on the triangle, in front of the near plane
    assert (pos[:, 2] < -0.1 + 1e-9).all() and pos[:, 2].max() > -0.5
    ys, xs = np.nonzero(r["covered"])
    ndc = np.stack([(xs + r["x0"] + 0.5) / VIEW[0] * 2 - 1, (ys + r["y0"] + 0.5) / VIEW[1] * 2 - 1], -1)
    c = B.R._xf(proj, pos)
    np.testing.assert_allclose(c[:, :2] / c[:, 3:4], ndc, atol=1e-9)                    # ... under its own pixel centre
    np.testing.assert_allclose(c[:, 2] / c[:, 3] * 0.5 + 0.5, r["z"][r["covered"]], atol=1e-9)


def test_normalise_is_the_weighted_mean_of_overlapping_fragments():
    pix = np.array([5, 5, 7])
    rgb = np.array([(1.0, 0.0, 0.25), (0.0, 1.0, 0.75), (0.2, 0.4, 0.6)])
    q = np.array([3.0, 1.0, 0.5])
    zbuf = np.full(9, 1.0)
    zbuf[[5, 7]] = (0.25, 0.75)
    rgba, depth = B.normalise(B.accumulate(9, pix, rgb, q), zbuf)
    np.testing.assert_allclose(rgba[5], (0.75, 0.25, 0.375, 1.0), atol=1e-15)
    np.testing.assert_allclose(rgba[7], (0.2, 0.4, 0.6, 1.0), atol=1e-15)
    assert (rgba[[0, 1, 2, 3, 4, 6, 8]] == 0).all() and (depth == zbuf).all()


def test_phong_on_axis_is_ambient_plus_diffuse_plus_full_specular():
    pos = B.LIGHT_POSITION * -0.5                            # the light straight behind the eye, the normal towards both
    n = B.LIGHT_POSITION / np.linalg.norm(B.LIGHT_POSITION)
    rgb, ok = B.phong(pos[None], n[None])
    np.testing.assert_allclose(rgb[0], B.LIGHT_AMBIENT * 0.5 + B.LIGHT_DIFFUSE * 0.5 + 0.5, atol=1e-12)
    rgb, ok = B.phong(pos[None], -n[None])                   # facing away: ambient only
    np.testing.assert_allclose(rgb[0], B.LIGHT_AMBIENT * 0.5, atol=1e-15)


def _id(case):
    return f"{case[0].__name__.replace('_case', '')} {case[1]}"


@pytest.mark.parametrize("case", list(C.all_cpu_cases()), ids=_id)
def test_oracle_agrees_with_the_reference(case):
    f, name = case
    f(C.only_oracle, name)


def test_oracle_leaves_no_crack_where_pixel_centres_lie_on_shared_edges():
    C.exact_case(C.only_oracle)


def test_the_portrait_frame_runs_the_swapped_bounds_off_the_other_axis():
    """cells x < height with stepX = 1 / width: in the portrait frame u passes 1, in the landscape frames v does"""
    for frame, (u_past, v_past) in (("portrait", (True, False)), ("landscape", (False, True))):
        w, h = C.FRAMES[frame]
        assert (B.buffer_coords(h, w).max() > 1.0, B.buffer_coords(w, h).max() > 1.0) == (u_past, v_past)


def test_a_wrong_side_is_named():
    name = "landscape frontal"
    ref = C.trigrid_reference(name, 3)
    good = (ref[0].astype(np.float32), ref[1].astype(np.float32))
    shifted = (good[0], np.roll(good[1], 1, axis=1))
    with pytest.raises(MC.Mismatch, match=r"the kernel disagrees.*margin"):
        C.check_draw("trigrid", name, ref, {"kernel": shifted, "oracle": good})
