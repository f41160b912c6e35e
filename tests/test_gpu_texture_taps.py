"""GPU: texture taps (tsdf_texture_taps / tsdf_texture_taps_dev / tsdf_mesh_texture_taps) against tests/texture_tap_reference.py byte for byte (a NaN
equal to a NaN: ray_reference.same_bytes' rule; no tolerance anywhere -- the path has no pow), the link to the draw through the receiver's rule, the cut
into launches, the mesh form, the device form through the lanes beside a twin that never takes taps, and every error code."""
import numpy as np
import pytest

import main_path_reference as R
import mesh_reference as M
import ray_reference as Q
import texture_tap_reference as T

pytestmark = pytest.mark.gpu

LIMIT = 0.04
KW = dict(brick_size=[2.0 / 8, 2.2 / 8, 2.0 / 8], limit=LIMIT, view=(64, 36))
RES = (37, 43, 35)                                                       # padded tiles on every axis
f32 = np.float32
SCENES = {"3-streams": dict(n_streams=3, lut_res=24, inv_res=32), "5-streams": dict(n_streams=5, lut_res=32, inv_res=24)}
BAD = [np.nan, np.inf, -np.inf, 1.0e6, -1.0e6]


def integrate(hip):
    hip.clearOccupiedBricks()
    hip.markBricks()
    hip.updateOccupiedBricks()
    hip.integrate()


def code(rr, fn):
    with pytest.raises(rr.TsdfError) as e:
        fn()
    return e.value.code


def assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.size == 0:
        return
    ok = Q.same_bytes(got.reshape(-1), want.reshape(-1))
    bad = np.nonzero(~ok)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(ok)} records differ, e.g. {bad[0]}: device {got.reshape(-1)[bad[0]]} reference {want.reshape(-1)[bad[0]]}"


def special_points():
    """unit-cube frame: the not-evaluated kinds in each axis, then tame points outside the cube (evaluated by clamping)"""
    bad = np.full((3 * len(BAD), 3), 0.5, f32)
    for a in range(3):
        for k, v in enumerate(BAD):
            bad[a * len(BAD) + k, a] = v
    out = np.array([(-0.5, 0.5, 0.5), (0.5, 1.5, 0.5), (0.5, 0.5, -3.0), (7.0, -2.0, 1.25), (0.2, 1234.5, 0.6), (0.2, 0.3, -99999.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)], f32)
    return bad, out


_CASES = {}


def case(rr, name):
    """per scene, computed once and left unchanged: the reference mesh of the integrated volume, the unit-cube and world point sets and their reference"""
    if name not in _CASES:
        scene = rr.scene.make_scene(color_width=96, color_height=80, **SCENES[name])
        bbox = (scene["bbox_min"], scene["bbox_max"])
        vol, _ = R.integrate(scene, RES, f32(LIMIT))
        mesh = M.extract(vol, LIMIT, *bbox)
        rng = np.random.default_rng(17)
        bad, outside = special_points()
        unit = np.concatenate([mesh["unit"], rng.uniform(0, 1, (500, 3)).astype(f32), bad, outside]).astype(f32)
        lo, e = np.asarray(bbox[0], np.float64), np.asarray(bbox[1], np.float64) - np.asarray(bbox[0], np.float64)
        world = np.concatenate([mesh["position"][::4], (lo + rng.uniform(0, 1, (500, 3)) * e).astype(f32), bad, (lo + outside.astype(np.float64) * e).astype(f32),
                                np.array([(3.0e6, 1.0, 0.0), (1.9e6, 1.0, 0.0)], f32)]).astype(f32)   # (finite, but u = 1.5e6 is not evaluated; u = 0.95e6 is)
        _CASES[name] = dict(scene=scene, bbox=bbox, mesh=mesh, unit=unit, world=world, n_mesh=len(mesh["unit"]),
                            unit_ref=T.records(scene, LIMIT, unit, unit_cube=True), world_ref=T.records(scene, LIMIT, world, bbox))
    return _CASES[name]


# ---------------------------------------------------------------------------------------------------------------- caller-given points
@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("world", [False, True], ids=["unit-cube", "world"])
def test_points_byte_equal(rr, name, world):
    K = case(rr, name)
    scene = K["scene"]
    pts, (want_t, want_s) = (K["world"], K["world_ref"]) if world else (K["unit"], K["unit_ref"])
    hip = rr.ReconIntegrationHip(scene, res=RES, **KW)                   # (no integrate: the taps need no volume)
    taps, sens = hip.texture_taps(pts, unit_cube=not world, sensor=True)
    st, want_st = hip.texture_tap_stats(), T.stats(want_t)
    print(f"{name} {'world' if world else 'unit cube'}: {len(pts)} points ({K['n_mesh']} mesh vertices), device stats {st}")
    assert_same(taps, want_t, "taps")
    assert_same(sens, want_s, "sensor records")
    assert st == want_st
    # the inputs are what they are meant to be.  Unit cube: all 15 special points are not evaluated.  World: the NaN and the infinities in each axis and
    # (3e6, 1, 0) are not, while +-1e6 maps to |u| of about 5e5 and is evaluated; the points outside the cube are evaluated in both
    assert want_st["not_evaluated"] == (10 if world else 15) * scene["n"] and want_st["with_quality"] > K["n_mesh"] // (8 if world else 2)
    outside = want_t["dist"][-10:-2] if world else want_t["dist"][-8:]
    assert (outside >= 0).all() and (not world or ((want_t["dist"][-2] == -1).all() and (want_t["dist"][-1] >= 0).all()))
    # without the flag: the same taps, and the same counts
    alone = hip.texture_taps(pts, unit_cube=not world)
    assert alone.tobytes() == taps.tobytes() and hip.texture_tap_stats() == want_st
    hip.close()


def test_one_stream_small_counts_and_nothing_written_without_the_sensor_flag(rr):
    import torch
    scene = rr.scene.make_scene(n_streams=1, width=160, height=120, lut_res=16, inv_res=24)
    rng = np.random.default_rng(2)
    vol, _ = R.integrate(scene, (24, 24, 24), f32(LIMIT))
    surface = M.extract(vol, LIMIT, scene["bbox_min"], scene["bbox_max"])["unit"]   # (points on the surface: where a stream has quality)
    pts = np.concatenate([surface[np.linspace(0, len(surface) - 1, 50).astype(np.int64)], rng.uniform(-0.1, 1.1, (15, 3)).astype(f32)]).astype(f32)
    pts[7] = (np.nan, 0.5, 0.5)
    want_t, want_s = T.records(scene, LIMIT, pts, unit_cube=True)
    assert (want_t["quality"] > 0).sum() > 5
    hip = rr.ReconIntegrationHip(scene, res=(32, 32, 32), **KW)
    for n in (1, 63, 64, 65, 0):
        taps, sens = hip.texture_taps(pts[:n], unit_cube=True, sensor=True)
        assert taps.shape == sens.shape == (n, 1)
        assert_same(taps, want_t[:n], f"{n} points, taps")
        assert_same(sens, want_s[:n], f"{n} points, sensor records")
        assert hip.texture_tap_stats() == T.stats(want_t[:n])
        # the device form into arrays with a guard behind them: exactly n records are written, and without the flag no sensor record anywhere
        d_pts = torch.from_numpy(np.concatenate([pts[:n].reshape(-1), np.zeros(3, f32)])).cuda()
        d_taps = torch.full((n * 16 + 256,), 0xAB, dtype=torch.uint8, device="cuda")
        d_sens = torch.full((n * 16 + 256,), 0xCD, dtype=torch.uint8, device="cuda")
        hip.texture_taps_dev(d_pts.data_ptr(), n, d_taps.data_ptr(), unit_cube=True)
        hip.sync()
        got = d_taps.cpu().numpy()
        assert got[:n * 16].tobytes() == taps.tobytes() and (got[n * 16:] == 0xAB).all(), n
        assert (d_sens.cpu().numpy() == 0xCD).all(), n
        hip.texture_taps_dev(d_pts.data_ptr(), n, d_taps.data_ptr(), d_sens.data_ptr(), unit_cube=True)
        hip.sync()
        got = d_sens.cpu().numpy()
        assert got[:n * 16].tobytes() == sens.tobytes() and (got[n * 16:] == 0xCD).all(), n
    hip.close()


# ---------------------------------------------------------------------------------------------------------------- the link to the draw
def test_blend_from_taps_is_the_rays_colour(rr, small_scene):
    """the draw's own rays of the 64 x 36 view, cast with colours; taps at the hits' unit-cube positions; the receiver's rule on the scene's colour images
    gives the rays' rgba bit for bit"""
    hip = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), **KW)
    integrate(hip)
    mv, pr = rr.scene.default_view(64, 36)
    hits, surf = hip.cast_rays(hip.view_rays(mv, pr), colours=True, unit_cube=True)
    hit = (hits["status"] & rr.RAY_HIT) != 0
    assert hit.sum() > 100
    taps = hip.texture_taps(hits["pos"][hit], unit_cube=True)
    assert (taps["dist"] >= 0).all()
    got, want = rr.blend_from_taps(taps, small_scene["color"]), surf["rgba"][hit]
    ok = ((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all(1)
    print(f"{int(hit.sum())} hits, alpha +1 on {int((want[:, 3] > 0).sum())}, streams with quality > 0 per hit: {np.bincount((taps['quality'] > 0).sum(1)).tolist()}")
    assert ok.all(), f"{int((~ok).sum())} of {len(ok)} hits differ, e.g. {got[~ok][0]} against {want[~ok][0]}"
    assert (want[:, 3] > 0).sum() > 50 and ((taps["quality"] > 0).sum(1) >= 2).sum() > 20
    hip.close()


# ---------------------------------------------------------------------------------------------------------------- the cut into launches
def test_launch_cut(rr):
    """1000 distinct points tiled to 2^18 + 3 points: two launches, the second of three points; every copy's records are its original's"""
    K = case(rr, "3-streams")
    scene = K["scene"]
    pick = np.linspace(0, len(K["unit"]) - 1, 1000).astype(np.int64)     # (spread over the set: mesh vertices, random points, the special ones)
    n = (1 << 18) + 3
    idx = np.arange(n) % 1000
    pts = K["unit"][pick][idx]
    want_t, want_s = K["unit_ref"][0][pick], K["unit_ref"][1][pick]
    hip = rr.ReconIntegrationHip(scene, res=RES, **KW)
    taps, sens = hip.texture_taps(pts, unit_cube=True, sensor=True)
    assert_same(taps, want_t[idx], "taps")
    assert_same(sens, want_s[idx], "sensor records")
    assert hip.texture_tap_stats() == T.stats(want_t[idx])
    hip.close()


# ---------------------------------------------------------------------------------------------------------------- the mesh form
def test_mesh_form(rr):
    K = case(rr, "3-streams")
    scene = K["scene"]
    hip = rr.ReconIntegrationHip(scene, res=(24, 40, 32), **KW)
    assert code(rr, lambda: hip.mesh_texture_taps()) == -4               # no extract yet
    integrate(hip)
    for level in (0, 2):
        mesh = hip.extract_mesh(normals=False, colours=False, level=level)
        pos = mesh["position"]
        assert len(pos) > (1000 if level == 0 else 50)
        assert code(rr, lambda: hip.mesh_download_texture_taps(len(pos))) == -4          # an extract leaves no taps behind
        assert hip.mesh_texture_taps(sensor=True, download=False) == (len(pos), scene["n"])
        st = hip.texture_tap_stats()
        taps, sens = hip.mesh_download_texture_taps(len(pos), sensor=True)
        assert hip.mesh_download_texture_taps(len(pos)).tobytes() == taps.tobytes()
        host_t, host_s = hip.texture_taps(pos, sensor=True)             # the host form on the downloaded positions: byte for byte
        assert taps.tobytes() == host_t.tobytes() and sens.tobytes() == host_s.tobytes()
        want_t, want_s = T.records(scene, LIMIT, pos, K["bbox"])
        assert_same(taps, want_t, f"level {level} taps")
        assert_same(sens, want_s, f"level {level} sensor records")
        assert st == T.stats(want_t) and st["with_quality"] > len(pos) // 2
        # without the flag there are no sensor records to download
        assert hip.mesh_texture_taps().tobytes() == taps.tobytes()
        assert code(rr, lambda: hip.mesh_download_texture_taps(len(pos), sensor=True)) == -4
        assert code(rr, lambda: hip._ck(hip._L.tsdf_mesh_texture_taps(hip._c, rr.TAPS_UNIT_CUBE, None, None))) == -1
        assert hip.mesh_download_texture_taps(len(pos)).tobytes() == taps.tobytes()     # (a refused call leaves the results)
    # a second extract invalidates the taps
    hip.extract_mesh(normals=False, colours=False)
    assert code(rr, lambda: hip.mesh_download_texture_taps(1)) == -4
    # an empty mesh: zero counts, nothing to download
    hip.set_tsdf(np.full((32, 40, 24), -LIMIT, f32))
    assert len(hip.extract_mesh(normals=False, colours=False)["position"]) == 0
    assert hip.mesh_texture_taps(sensor=True, download=False) == (0, scene["n"])
    taps, sens = hip.mesh_download_texture_taps(0, sensor=True)
    assert taps.shape == sens.shape == (0, scene["n"])
    assert hip.texture_tap_stats() == dict(points=0, streams=scene["n"], with_quality=0, not_evaluated=0)
    hip.close()


# ---------------------------------------------------------------------------------------------------------------- through the lanes
def test_device_form_through_the_lanes(rr):
    """Two scenes alternate for four frames through tsdf_frame_dev with stage overlap on.  tsdf_texture_taps_dev is queued behind every frame with no host
    wait in between; after the final sync each call's records are the reference's for the frame current at its call, and the presented frames and the
    final volume are those of a twin context that never took taps.  A smoke check of the arrangement: at these sizes the kernels take microseconds."""
    import torch
    mk = dict(n_streams=2, width=160, height=120, lut_res=32, inv_res=32)
    scs = [rr.scene.make_scene(**mk), rr.scene.make_scene(**mk, sphere_c=(0.4, 0.7, -0.3), box_c=(-0.5, 1.5, 0.2))]
    raw = [[torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ("depth", "quality", "silhouette", "color")] for sc in scs]
    mv, pr = rr.scene.default_view(64, 36)
    frames, n = 4, 2048
    bbox = (scs[0]["bbox_min"], scs[0]["bbox_max"])
    lo, e = np.asarray(bbox[0], np.float64), np.asarray(bbox[1], np.float64) - np.asarray(bbox[0], np.float64)
    # points on both scenes' surfaces (where a stream has quality: vertices of the two reference meshes), and random ones in and around the box
    on = [M.extract(R.integrate(sc, (32, 32, 32), f32(LIMIT))[0], LIMIT, *bbox)["position"] for sc in scs]
    on = [p[np.linspace(0, len(p) - 1, 900).astype(np.int64)] for p in on]
    pts = np.concatenate(on + [(lo + np.random.default_rng(9).uniform(-0.05, 1.05, (n - 1800, 3)) * e).astype(f32)]).astype(f32)
    pts[5] = (np.inf, 0.0, 0.0)
    want = [T.records(sc, LIMIT, pts, bbox) for sc in scs]
    assert want[0][0].tobytes() != want[1][0].tobytes()                 # the two frames differ
    d_pts = torch.from_numpy(pts.copy()).cuda()
    d_taps = [torch.zeros((n * 2, 16), dtype=torch.uint8, device="cuda") for _ in range(frames)]
    d_sens = [torch.zeros((n * 2, 16), dtype=torch.uint8, device="cuda") for _ in range(frames)]
    torch.cuda.synchronize()

    def run(with_taps):
        hip = rr.ReconIntegrationHip(scs[0], res=(32, 32, 32), **KW)
        hip.present_config(rr.PRESENT_RGBA8, 0, frames)
        for f in range(frames):                                         # no host wait inside the loop
            hip.frame_dev(mv, pr, [t.data_ptr() for t in raw[f % 2]])
            hip.present(f)
            if with_taps:
                hip.texture_taps_dev(d_pts.data_ptr(), n, d_taps[f].data_ptr(), d_sens[f].data_ptr())
        hip.sync()
        if with_taps:
            assert hip.texture_tap_stats() == T.stats(want[(frames - 1) % 2][0])
        shown = []
        for f in range(frames):
            data, tag, _ = hip.present_acquire()
            assert tag == f
            shown.append(data.tobytes())
            hip.present_release()
        vol = hip.tsdf()
        hip.close()
        return shown, vol

    shown, vol = run(True)
    for f in range(frames):
        taps = d_taps[f].cpu().numpy().reshape(-1).view(rr.TEXTURE_TAP_DTYPE).reshape(n, 2)
        sens = d_sens[f].cpu().numpy().reshape(-1).view(rr.SENSOR_TAP_DTYPE).reshape(n, 2)
        assert (taps["quality"] > 0).sum() > 100, f
        assert_same(taps, want[f % 2][0], f"frame {f} taps")
        assert_same(sens, want[f % 2][1], f"frame {f} sensor records")
    twin_shown, twin_vol = run(False)
    assert shown == twin_shown and shown[0] != shown[1]
    assert vol.tobytes() == twin_vol.tobytes()


# ---------------------------------------------------------------------------------------------------------------- errors
def test_error_codes(rr, small_scene):
    import ctypes as C
    pts = np.array([(0.5, 0.5, 0.5), (0.25, 0.5, 0.75)], f32)
    hip = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), **KW)
    lib, c = hip._L, hip._c
    assert code(rr, lambda: hip.texture_tap_stats()) == -4              # before any call
    whole = hip.texture_taps(pts, unit_cube=True, sensor=True)          # before the first integrate: the taps need no volume
    assert (whole[0]["dist"] >= 0).all()
    p, tap, sen = (C.c_float * 3)(0.5, 0.5, 0.5), (rr.TextureTap * 4)(), (rr.SensorTap * 4)()
    host = lambda x, n, flags, t, s: lib.tsdf_texture_taps(c, x, C.c_uint64(n), C.c_uint32(flags), t, s)
    dev = lambda x, n, flags, t, s: lib.tsdf_texture_taps_dev(c, x, C.c_uint64(n), C.c_uint32(flags), t, s)
    for fn in (host, dev):
        assert fn(p, 1, 4, tap, None) == -1                             # an unknown flag
        assert fn(None, 0, 4, None, None) == -1                         # ... with nothing to do as well
        assert fn(None, 1, 0, tap, None) == -1                          # NULL arrays with n > 0
        assert fn(p, 1, 0, None, None) == -1
        assert fn(p, 1, 0, tap, sen) == -1                              # sensor is given exactly when TSDF_TAPS_SENSOR is set
        assert fn(p, 1, rr.TAPS_SENSOR, tap, None) == -1
        assert fn(p, (1 << 40) + 1, 0, tap, None) == -1                 # more than 2^40 points
        assert fn(None, 0, 0, None, None) == 0                          # n == 0: TSDF_OK, nothing launched
        assert hip.texture_tap_stats() == dict(points=0, streams=4, with_quality=0, not_evaluated=0)
    assert lib.tsdf_mesh_texture_taps(c, C.c_uint32(4), None, None) == -1
    assert lib.tsdf_mesh_texture_taps(c, C.c_uint32(rr.TAPS_UNIT_CUBE), None, None) == -1
    assert lib.tsdf_mesh_texture_taps(c, C.c_uint32(0), None, None) == -4          # no extract
    assert lib.tsdf_mesh_download_texture_taps(c, tap, None) == -4
    assert lib.tsdf_texture_tap_stats(c, None) == -1
    hip.close()

    bare = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), upload=False, **KW)          # a volume, but neither calibration nor frame
    bare.set_tsdf(M.sphere_volume((32, 32, 32), limit=LIMIT))
    assert code(rr, lambda: bare.texture_taps(pts, unit_cube=True)) == -4
    bare.extract_mesh(normals=True, colours=False)
    assert code(rr, lambda: bare.mesh_texture_taps()) == -4
    bare.set_calibration(small_scene)                                   # calibration alone: still no frame
    assert code(rr, lambda: bare.texture_taps(pts, unit_cube=True)) == -4
    bare.upload_frame(small_scene)
    assert bare.texture_taps(pts, unit_cube=True, sensor=True)[0].tobytes() == whole[0].tobytes()
    bare.close()

    slab = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), slab=(0, 16), **KW)           # a Z-slab context holds whole LUTs and frames: it succeeds
    got = slab.texture_taps(pts, unit_cube=True, sensor=True)
    assert got[0].tobytes() == whole[0].tobytes() and got[1].tobytes() == whole[1].tobytes()
    assert code(rr, lambda: slab.mesh_texture_taps()) == -4             # (a slab context extracts no mesh)
    slab.close()
