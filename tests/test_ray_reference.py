"""CPU: tests/ray_reference.py (the ray queries' definition in numpy float32) is held to the independent float64 reference of the draw's march
(tests/main_path_reference.py) on the camera rays of tests/main_path_cases.py's views, with the acceptance rule and the march_depth row of its TABLE;
and to cases that can be computed by hand on a plane and on a sphere."""
import numpy as np
import pytest

import main_path_cases as K
import main_path_reference as R
import mesh_reference as M
import ray_reference as Q

f32 = np.float32
BBOX = ((-1.0, 0.0, -1.0), (1.0, 2.2, 1.0))


# ---------------------------------------------------------------------------------------------------------------- camera rays
def camera_rays(V):
    """the pixel rays of a main_path_reference.View, rounded to float32 once: unit-cube origin = CameraPos, direction un-normalised"""
    x, y = R.pixel_centres(V.size)
    d = V.window_to_vol(x, y, np.ones_like(x)) - V.cam
    return Q.make_rays(np.broadcast_to(V.cam, d.shape).reshape(-1, 3), d.reshape(-1, 3))


# every view of main_path_cases.MARCH_EYES; both volumes and both resolutions appear, each view once
CASES = [("sphere", K.MARCH_RES[0], "far"), ("slab", K.MARCH_RES[1], "grazing"), ("sphere", K.MARCH_RES[1], "inside"), ("slab", K.MARCH_RES[0], "axis")]


@pytest.mark.parametrize("kind,res,eye", CASES, ids=[f"{k}-{e}" for k, _, e in CASES])
def test_restatement_agrees_with_the_float64_march_on_camera_rays(kind, res, eye):
    ref = K.march_reference_dense(kind, res, eye)
    V = ref["view"]
    h, w = V.size[1], V.size[0]
    sc = K.small_scene()
    got = Q.cast(K.march_volume(kind, res), K.LIMIT, sc["bbox_min"], sc["bbox_max"], camera_rays(V), unit_cube=True)
    hits = got["hits"].reshape(h, w)
    n = hits["n_samples"].astype(np.float64)
    hit = (hits["status"] & Q.HIT) != 0
    assert not (hits["status"] & Q.INVALID).any()
    t = K.TABLE["march_depth"]
    touched = (ref["n"] > 0) | (n > 0)
    what = f"ray_reference {kind} {res} eye {eye}"
    share, _ = K.compare("march count: " + what, ref["n"], ref["margin"], t["bound"], t["cap"], {"ray_reference": n}, lambda a, b: a == b, count=touched)
    K.compare("march hit: " + what, ref["hit"], ref["margin"], t["bound"], t["cap"], {"ray_reference": hit}, lambda a, b: a == b, count=touched)
    with np.errstate(invalid="ignore"):
        # gl_FragDepth as the framebuffer holds it (main_path_cases.check_march): clamped to [0, 1] -- a hit beside the eye has an eye-space z near 0
        depth = np.where(hit, np.clip(V.frag_depth(got["unit"].reshape(h, w, 3).astype(np.float64)), 0.0, 1.0), 1.0)
        want = np.where(ref["hit"], np.clip(ref["depth"], 0.0, 1.0), 1.0)
    K.compare("march_depth: " + what, want, ref["margin"], t["bound"], t["cap"], {"ray_reference": depth}, K.close_abs(t["tol"]), count=touched)
    print(f"{what}: {int(touched.sum())} rays marched, {int(hit.sum())} hits, {share:.2%} excluded by the reference's margin")
    assert int((ref["hit"] & (ref["margin"] >= t["bound"])).sum()) >= K.MIN_HIT_PIXELS or eye == "axis"


# ---------------------------------------------------------------------------------------------------------------- by hand
LIMIT = 0.04
SD = LIMIT / 2


def plane_volume(res=(32, 24, 16)):
    """f = x - 0.5, clamped to +-limit: positive (inside the surface) for x > 0.5, [rz][ry][rx]"""
    rx, ry, rz = res
    x = (np.arange(rx) + 0.5) / rx - 0.5
    return np.ascontiguousarray(np.broadcast_to(np.clip(x, -LIMIT, LIMIT).astype(f32)[None, None, :], (rz, ry, rx)))


def cast_unit(vol, rays, limit=LIMIT):
    return Q.cast(vol, limit, BBOX[0], BBOX[1], rays, unit_cube=True)["hits"]


def test_axis_parallel_ray_hits_the_plane_where_it_is():
    # zero direction components: infinite inverses, 0 * inf for the origin's y = z = 0.5 never arises, (0 - 0.5) * inf = -inf does
    h = cast_unit(plane_volume(), Q.make_rays([(0.105, 0.5, 0.5)], [(3.0, 0.0, 0.0)]))[0]
    assert h["status"] == Q.HIT
    assert h["n_samples"] == 21                                        # samples at 0.105 + k * 0.02: the first with x > 0.5 is k = 20
    assert abs(h["pos"][0] - 0.5) < 2e-6 and h["pos"][1] == f32(0.5) and h["pos"][2] == f32(0.5)
    assert abs(h["t"] - 0.395 / 3.0) < 1e-6                            # in units of the caller's direction, which has length 3
    # ... and with an origin on the box's face, where 0 * inf = NaN is ignored by fmin / fmax
    h = cast_unit(plane_volume(), Q.make_rays([(0.0, 0.5, 0.5)], [(1.0, 0.0, 0.0)]))[0]
    assert h["status"] == Q.HIT and abs(h["pos"][0] - 0.5) < 2e-6


def test_origin_inside_the_surface_hits_at_the_first_sample():
    h = cast_unit(plane_volume(), Q.make_rays([(0.8, 0.5, 0.5)], [(1.0, 0.0, 0.0)]))[0]
    assert h["status"] == Q.HIT and h["n_samples"] == 1
    # prev = -limit, dens = +limit: (p - s) - s * (-limit / (2 limit)) = p - s / 2
    assert abs(h["pos"][0] - (0.8 - SD / 2)) < 1e-6 and abs(h["t"] + SD / 2) < 1e-6


def test_origin_inside_the_box_outside_the_surface():
    d = np.array([1.0, 0.2, 0.1])
    h = cast_unit(plane_volume(), Q.make_rays([(0.3, 0.4, 0.45)], [d]))[0]
    assert h["status"] == Q.HIT
    assert abs(h["pos"][0] - 0.5) < 2e-6
    assert np.allclose(h["pos"], np.array([0.3, 0.4, 0.45]) + h["t"] * d, atol=2e-6)
    step_x = SD / np.linalg.norm(d)
    assert h["n_samples"] == int(np.floor(0.2 / step_x)) + 2          # k = 0 at the origin, the first sample past x = 0.5


def test_ray_that_misses_the_box():
    h = cast_unit(plane_volume(), Q.make_rays([(-1.0, 2.0, 0.5), (0.5, 0.5, 2.0)], [(1.0, 0.0, 0.0), (0.0, 0.0, 1.0)]))
    for r in h:                                                        # beside the box; behind the origin
        assert r["status"] == Q.OUTSIDE and r["n_samples"] == 0 and r["t"] == f32(-1.0) and (r["pos"] == 0).all()


def test_interval_short_of_the_surface_and_beyond_it():
    vol = plane_volume()
    short = cast_unit(vol, Q.make_rays([(0.105, 0.5, 0.5)], [(1.0, 0.0, 0.0)], t_max=0.2))[0]
    assert short["status"] == 0 and short["n_samples"] == 10 and short["t"] == f32(-1.0)      # ceil(0.2 / 0.02) samples, none positive
    beyond = cast_unit(vol, Q.make_rays([(0.105, 0.5, 0.5)], [(1.0, 0.0, 0.0)], t_min=0.6))[0]
    assert beyond["status"] == Q.HIT and beyond["n_samples"] == 1                              # starts at x = 0.705, inside the surface
    assert abs(beyond["pos"][0] - (0.705 - SD / 2)) < 1e-6
    nothing = cast_unit(vol, Q.make_rays([(0.105, 0.5, 0.5)], [(1.0, 0.0, 0.0)], t_min=0.3, t_max=0.2))[0]
    assert nothing["status"] == Q.OUTSIDE and nothing["n_samples"] == 0
    behind = cast_unit(vol, Q.make_rays([(0.105, 0.5, 0.5)], [(1.0, 0.0, 0.0)], t_min=-5.0))[0]   # a negative t_min starts at the origin
    whole = cast_unit(vol, Q.make_rays([(0.105, 0.5, 0.5)], [(1.0, 0.0, 0.0)]))[0]
    assert behind.tobytes() == whole.tobytes()


def test_the_three_invalid_rays():
    rays = Q.make_rays([(0.1, 0.5, 0.5), (np.nan, 0.5, 0.5), (0.1, 0.5, 0.5), (0.1, 0.5, 0.5), (0.1, 0.5, 0.5)],
                       [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (1.0, np.inf, 0.0), (1.0, 0.0, 0.0), (1e-30, 0.0, 0.0)])
    rays["t_min"][3] = np.nan
    for r in cast_unit(plane_volume(), rays):                          # zero direction; NaN origin; infinite direction; NaN t_min; squares underflow
        assert r["status"] == Q.INVALID and r["n_samples"] == 0 and r["t"] == f32(-1.0) and (r["pos"] == 0).all()


def test_sphere_from_outside_the_box_world_and_unit_cube_agree():
    limit = 0.05
    vol = M.sphere_volume((24, 16, 16), 0.3, limit)
    unit = Q.make_rays([(0.5, 0.5, 1.5)], [(0.0, 0.0, -1.0)])
    hu = Q.cast(vol, limit, BBOX[0], BBOX[1], unit, unit_cube=True)["hits"][0]
    assert hu["status"] == Q.HIT and abs(hu["pos"][2] - 0.8) < 0.01 and hu["pos"][0] == f32(0.5)
    assert abs(hu["t"] - (1.5 - hu["pos"][2])) < 1e-6
    lo, hi = np.array(BBOX[0]), np.array(BBOX[1])
    world = Q.make_rays([lo + np.array([0.5, 0.5, 1.5]) * (hi - lo)], [np.array([0.0, 0.0, -1.0]) * (hi - lo)])
    hw = Q.cast(vol, limit, BBOX[0], BBOX[1], world)["hits"][0]
    assert hw["status"] == Q.HIT and hw["n_samples"] == hu["n_samples"]
    assert np.allclose(hw["pos"], lo + hu["pos"] * (hi - lo), atol=1e-5) and abs(hw["t"] - hu["t"]) < 1e-5


def test_surface_is_the_mesh_sections_normal_at_the_hit():
    limit = 0.05
    vol = M.sphere_volume((24, 16, 16), 0.3, limit)
    res = Q.cast(vol, limit, BBOX[0], BBOX[1], Q.make_rays([(0.5, 0.5, 1.5), (2.0, 2.0, 2.0)], [(0.0, 0.0, -1.0), (1.0, 0.0, 0.0)]), unit_cube=True)
    s = Q.surface(vol, None, limit, BBOX[0], BBOX[1], res, normals=True, colours=False)
    assert np.allclose(s["normal"][0], (0.0, 0.0, 1.0), atol=1e-3)      # out of the sphere, towards the ray's origin
    assert s[1].tobytes() == bytes(32)                                  # no hit: zeros
