"""CPU: tests/texture_tap_reference.py (the texture taps' definition in numpy float32 on the oracle's filters).  The record loses nothing: the receiver's
rule on the taps gives blendColors' colour -- tests/mesh_reference.py's colours() -- bit for bit at the vertices of the reference mesh, on scenes with
different stream counts and LUT resolutions; the not-evaluated rule, the clamping far outside the cube and the world mapping's operation order."""
import numpy as np
import pytest

import main_path_reference as R
import mesh_reference as M
import texture_tap_reference as T

f32 = np.float32
LIMIT = 0.04
RES = (24, 40, 32)
SCENES = [dict(n_streams=3, lut_res=24, inv_res=32), dict(n_streams=5, lut_res=32, inv_res=24)]   # (the two LUT resolutions differ on purpose)


def same_bits(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module", params=SCENES, ids=lambda p: f"{p['n_streams']}-streams")
def case(request):
    """the scene, the reference mesh of its integrated volume, and the taps at the mesh's unit-cube positions -- computed once"""
    import rgbd_recon_amd as rr
    scene = rr.scene.make_scene(color_width=96, color_height=80, **request.param)
    vol, _ = R.integrate(scene, RES, f32(LIMIT))
    mesh = M.extract(vol, LIMIT, scene["bbox_min"], scene["bbox_max"])
    taps, sens = T.records(scene, LIMIT, mesh["unit"], unit_cube=True)
    return dict(scene=scene, mesh=mesh, taps=taps, sensor=sens)


def test_combined_taps_are_blend_colors_bit_for_bit(case):
    scene, unit, taps = case["scene"], case["mesh"]["unit"], case["taps"]
    assert len(unit) > 1000 and taps.shape == (len(unit), scene["n"])
    want = M.colours(scene, LIMIT, unit)
    got = T.combine(scene, taps)
    ok = same_bits(got, want).all(1)
    assert ok.all(), f"{int((~ok).sum())} of {len(ok)} vertices differ, e.g. {got[~ok][0]} against {want[~ok][0]}"
    # the test is not about fallbacks alone (a condition on the scene, not a measurement of the code)
    with_q = (taps["quality"] > 0).sum(1)
    print(f"{scene['n']} streams: {len(unit)} vertices, {100.0 * (with_q >= 1).mean():.1f} % with a stream of quality > 0, {100.0 * (with_q >= 2).mean():.1f} % with two or more; "
          f"alpha +1 on {100.0 * (want[:, 3] > 0).mean():.1f} %")
    assert (with_q >= 1).mean() >= 0.90 and (with_q >= 2).mean() >= 0.30
    assert (taps["dist"] >= 0).all()                                     # every mesh vertex is evaluated
    assert T.stats(taps) == dict(points=len(unit), streams=scene["n"], with_quality=int(with_q.sum()), not_evaluated=0)


def test_sensor_records_are_the_inverse_lut_and_the_nearest_depth(case):
    from oracle import oracle as orc
    scene, unit, taps, sens = case["scene"], case["mesh"]["unit"], case["taps"], case["sensor"]
    ri = [int(x) for x in scene["inv_res"]]
    depth = np.ascontiguousarray(scene["depth"], f32)
    for k in (0, len(unit) // 2, len(unit) - 1):
        for i in range(scene["n"]):
            inv = np.asarray(scene["cv_xyz_inv"][i], f32).reshape(ri[2], ri[1], ri[0], 4)
            pc = orc.tex3d(inv, *unit[k])[:3]
            s = sens[k, i]
            assert (s["x"], s["y"], s["z"]) == tuple(pc)
            assert s["depth"] == f32(orc.tex2d_nearest(depth, i, pc[0], pc[1], 0))
            assert taps[k, i]["dist"] == np.abs(f32(s["depth"] - s["z"]))
            assert taps[k, i]["quality"] == 0 or taps[k, i]["dist"] < f32(LIMIT)


def test_binding_blend_from_taps_is_the_same_rule(rr, case):
    """rgbd_recon_amd.blend_from_taps (numpy alone: what a receiver without the oracle runs) against combine() on the oracle's colour fetch, also on
    coordinates outside the image, not-evaluated records and a NaN"""
    scene = case["scene"]
    taps = case["taps"][:800].copy()
    rng = np.random.default_rng(5)
    taps["u"][:40] = rng.uniform(-0.5, 1.5, (40, scene["n"]))
    taps["v"][40:80] = rng.uniform(-0.5, 1.5, (40, scene["n"]))
    taps[80:90] = np.array((0, 0, 0, -1), T.TEXTURE_TAP_DTYPE)
    taps["u"][90, 0] = np.nan
    assert taps.dtype == rr.TEXTURE_TAP_DTYPE == T.TEXTURE_TAP_DTYPE and rr.SENSOR_TAP_DTYPE == T.SENSOR_TAP_DTYPE
    got, want = rr.blend_from_taps(taps, scene["color"]), T.combine(scene, taps)
    ok = same_bits(got, want).all(1)
    assert ok.all(), f"{int((~ok).sum())} of {len(ok)} differ, e.g. row {np.nonzero(~ok)[0][0]}: {got[~ok][0]} against {want[~ok][0]}"


BAD = [np.nan, np.inf, -np.inf, 1.0e6, -1.0e6]


def test_points_that_are_not_evaluated(case):
    scene = case["scene"]
    pts = np.full((3 * len(BAD) + 2, 3), 0.5, f32)
    for a in range(3):
        for k, v in enumerate(BAD):
            pts[a * len(BAD) + k, a] = v
    pts[-2] = (0.5, 0.5, 0.5)                                            # evaluated ...
    pts[-1] = (np.nextafter(f32(1.0e6), f32(0)), 0.5, -999999.9)         # ... and so is the largest tame point
    taps, sens = T.records(scene, LIMIT, pts, unit_cube=True)
    for row in range(3 * len(BAD)):
        assert taps[row].tobytes() == np.array([(0, 0, 0, -1)] * scene["n"], T.TEXTURE_TAP_DTYPE).tobytes(), row
        assert sens[row].tobytes() == bytes(16 * scene["n"]), row
    assert (taps["dist"][-2:] >= 0).all()
    assert T.stats(taps)["not_evaluated"] == 3 * len(BAD) * scene["n"]
    # world coordinates: the rule applies to u, so a finite point is not evaluated when the mapping overflows it
    bbox = (scene["bbox_min"], scene["bbox_max"])
    world = np.array([(0.0, 1.0, 0.0), (3.0e6, 1.0, 0.0), (1.9e6, 1.0, 0.0), (np.nan, 1.0, 0.0)], f32)    # (the box is 2 wide: u = 1.5e6, then 0.95e6 + 0.5)
    u = T.to_unit(world, bbox)
    assert list(T.evaluated(u)) == [True, False, True, False]
    assert list(T.taps(scene, LIMIT, world, bbox)["dist"][:, 0] >= 0) == [True, False, True, False]


def test_a_tame_point_far_outside_the_cube_is_evaluated_by_clamping(case):
    scene = case["scene"]
    far = np.array([(-7.0, 0.3, 0.6), (0.2, 1234.5, 0.6), (0.2, 0.3, -99999.0)], f32)
    near = np.clip(far, 0.0, 1.0).astype(f32)                           # CLAMP_TO_EDGE: the edge texel, whose centre lies inside the cube
    a, sa = T.records(scene, LIMIT, far, unit_cube=True)
    b, sb = T.records(scene, LIMIT, near, unit_cube=True)
    assert (a["dist"] >= 0).all()
    assert a.tobytes() == b.tobytes() and sa.tobytes() == sb.tobytes()


def test_world_mapping_takes_the_difference_then_the_division(case):
    scene = case["scene"]
    lo, hi = np.asarray(scene["bbox_min"], f32), np.asarray(scene["bbox_max"], f32)
    e = (hi - lo).astype(f32)
    rng = np.random.default_rng(3)
    world = (lo + rng.uniform(0, 1, (2000, 3)) * e).astype(f32)
    u = T.to_unit(world, (lo, hi))
    want = ((world - lo).astype(f32) / e).astype(f32)
    assert u.dtype == f32 and (u.view(np.uint32) == want.view(np.uint32)).all()
    other = (world * (f32(1.0) / e) - lo * (f32(1.0) / e)).astype(f32)  # another order of operations is another result somewhere: the order is part of the definition
    assert (other.view(np.uint32) != want.view(np.uint32)).any()
    assert (T.to_unit(world, None, unit_cube=True).view(np.uint32) == world.view(np.uint32)).all()
    # ... and taps of world points are the taps of the mapped points
    a = T.taps(scene, LIMIT, world[:50], (lo, hi))
    b = T.taps(scene, LIMIT, u[:50], unit_cube=True)
    assert a.tobytes() == b.tobytes()
