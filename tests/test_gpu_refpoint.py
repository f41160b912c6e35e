"""-m gpu: the HIP path at the operating point of the program it replaces (tests/refpoint_scene.py: 200 x 221 x 200 voxels, bricks of 10
voxels, 5 streams of 512 x 424 / 1280 x 1080, inverse LUTs of 286 x 315 x 286 texels) against the oracle on identical inputs.  A tile's
LUT texel box is 12^3 there, over the LDS budget of the fast integrate kernels: every test asserts through tsdf_integrate_form that the
generic kernel (k_integrate_tiles) ran.  Comparisons are the project's rule: every value equal (POW_ATOL only where shading calls pow())."""
import os
import sys

import numpy as np
import pytest

import refpoint_scene as rp
from helpers import POW_ATOL, assert_close_abs, assert_frames_identical, assert_same, lut_box_class
from oracle.oracle import OracleRecon

pytestmark = pytest.mark.gpu

SMALL_VIEW = (640, 360)          # the frame sequences: the oracle's march is most of their time, the view is not what they are about
N_TILES = 25 * 28 * 25           # 8^3-voxel tiles of the 200 x 221 x 200 volume


@pytest.fixture(scope="module")
def frames(rr):
    return rp.make_frames(rr)


def run(o, mv, pr):
    """bricks, integrate and the march; the hole filling follows in compare_frame, behind the comparison of the march's own images (the
    library fills in place what the oracle keeps apart)"""
    o.clearOccupiedBricks(); o.markBricks(); r = o.updateOccupiedBricks()
    o.integrate()
    o.draw(mv, pr)
    return r


def generic(hip, culled):
    f = hip.integrate_form()
    assert f["form"] == "generic" and f["culled"] == culled, f
    if culled:
        assert f["items"] == len(hip.active_tiles()[0]) and f["grid"] == min(N_TILES, int(os.environ.get("RR_K1_GRID", 2048)))
    else:
        assert f["items"] == f["grid"] == N_TILES
    return f


def compare_bricks(hip, orc, what):
    cnt, flags = hip.bricks()
    np.testing.assert_array_equal(cnt, orc.counters(), err_msg=f"{what}: brick counters")
    occ = np.zeros(orc.numBricks(), np.uint8)
    occ[orc.occupied()] = 1
    np.testing.assert_array_equal(flags, occ, err_msg=f"{what}: occupied bricks")


def compare_frame(hip, orc, what, colour_atol=0.0, min_hits=5000, drawn=False):
    """TSDF (the whole volume: a tile that emptied out must read -limit), the march's images, then fillColors() on both sides (where colour
    filling is on) and the frame.  drawn: drawF has run already (tsdf_frame_dev) -- volume and frame only"""
    assert_same(hip.tsdf(), orc.tsdf(), f"{what}: tsdf")
    if drawn:
        return assert_frames_identical(hip, orc, what, min_hits=min_hits, colour_atol=colour_atol)
    (ha, hd, hn, hp), (oa, od, on, op) = hip.view_images(), orc.view_images()
    if orc.flags["skip_space"]:
        assert_same(hp[..., :3], op[..., :3], f"{what}: depth peels")
    assert_same(hn, on, f"{what}: sample counts")
    assert_same(hd, od, f"{what}: march depth")
    if colour_atol:
        assert_close_abs(ha, oa, colour_atol, f"{what}: march colour")
    else:
        assert_same(ha, oa, f"{what}: march colour")
    if orc.flags["fill_holes"]:
        hip.fillColors(); orc.fillColors()
    return assert_frames_identical(hip, orc, what, min_hits=min_hits, colour_atol=colour_atol)


def compare_atlas(hip, orc, what):
    (hac, had), (oac, oad) = hip.atlas(), orc.atlas()
    off, lres = orc.lod_tables()
    for l in range(len(off)):
        x0, y0, rx, ry = int(off[l][0]), int(off[l][1]), int(lres[l][0]), int(lres[l][1])
        assert_same(hac[y0:y0 + ry, x0:x0 + rx], oac[y0:y0 + ry, x0:x0 + rx], f"{what}: pyramid colour, level {l}")
        assert_same(had[y0:y0 + ry, x0:x0 + rx], oad[y0:y0 + ry, x0:x0 + rx], f"{what}: pyramid depth, level {l}")


def test_selection_rule_at_the_reference_point():
    assert lut_box_class(rp.RES, rp.INV_RES) == ((12, 12, 12), 0)


def test_one_frame_culled_then_dense_at_the_defaults(rr, frames):
    """brick 0.1 m, 10 voxels per brick at least, space skip and colour fill on, 1280 x 720: every stage's product; then the same context
    dense -- k_march_box leaps over runs of tiles by the classes the generic kernel wrote.  Frame B: its sphere reaches the partial
    tile layer on y (221 = 27 * 8 + 5)."""
    sc = frames[1]
    hip, orc = rr.ReconIntegrationHip(sc, **rp.KW), OracleRecon(sc, **rp.KW)
    assert hip.res == orc.res == rp.RES and hip.res_bricks == orc.res_bricks == rp.RES_BRICKS
    mv, pr = rr.scene.default_view(*rp.KW["view"])
    r_hip, r_orc = run(hip, mv, pr), run(orc, mv, pr)
    f = generic(hip, True)
    assert r_hip == r_orc and 0.01 < r_orc < 0.2 and 500 < f["items"] < N_TILES
    compare_bricks(hip, orc, "culled")
    compare_frame(hip, orc, "culled", min_hits=20000)
    compare_atlas(hip, orc, "culled")
    t = hip.tsdf()
    assert (np.abs(t[:, 216:, :]) < rp.LIMIT).sum() > 0, "no surface voxel in the partial tile layer ty = 27"
    tiles = hip.active_tiles()[0]
    assert (tiles[:, 1] == 27).any()
    for o in (hip, orc):
        o.setUseBricks(False)
        run(o, mv, pr)
    generic(hip, False)
    compare_frame(hip, orc, "dense", min_hits=20000)
    hip.close()


def test_shade_modes(rr, frames):
    """space skip off, colour fill off: one draw per shade mode of one integrated volume"""
    hip, orc = rr.ReconIntegrationHip(frames[0], **rp.KW), OracleRecon(frames[0], **rp.KW)
    mv, pr = rr.scene.default_view(*rp.KW["view"])
    for o in (hip, orc):
        o.setSpaceSkip(False); o.setColorFilling(False)
        o.clearOccupiedBricks(); o.markBricks(); o.updateOccupiedBricks(); o.integrate()
    generic(hip, True)
    for mode in (0, 1, 2, 3):
        for o in (hip, orc):
            o.setShadeMode(mode)
            o.draw(mv, pr)
        compare_frame(hip, orc, f"shade mode {mode}", colour_atol=POW_ATOL if mode == 1 else 0.0, min_hits=20000)
    hip.close()


def sequence(rr, frames, view, brick, min_items_per_workgroup, sparse_pool_tiles=0):
    """scene A, B, C, A through ONE context against a fresh oracle per frame -- TSDF, counters, frame after every one --, then the same
    context dense.  -> the forms of the culled launches.  Raises AssertionError on any difference."""
    kw = dict(rp.KW, view=view, brick_size=brick)
    hip = rr.ReconIntegrationHip(frames[0], sparse_pool_tiles=sparse_pool_tiles, **kw)
    mv, pr = rr.scene.default_view(*view)
    forms, occupied = [], []
    for n, k in enumerate((0, 1, 2, 0)):
        hip.upload_frame(frames[k])
        orc = OracleRecon(frames[k], **kw)
        assert run(hip, mv, pr) == run(orc, mv, pr)
        f = generic(hip, True)
        assert f["items"] >= min_items_per_workgroup * f["grid"], f"frame {n}: {f} -- fewer than {min_items_per_workgroup} tiles per workgroup"
        forms.append(f)
        compare_bricks(hip, orc, f"frame {n}")
        compare_frame(hip, orc, f"frame {n}")
        occupied.append(set(np.flatnonzero(hip.bricks()[1]).tolist()))
    assert occupied[0] - occupied[1] and occupied[1] - occupied[2] and occupied[0] == occupied[3]     # bricks really empty out
    for o in (hip, orc):                                   # (orc: the last frame's oracle)
        o.setUseBricks(False)
        run(o, mv, pr)
    generic(hip, False)
    compare_frame(hip, orc, "dense after the culled sequence")
    hip.close()
    return forms


def test_grid_stride_culled_sequence(rr, frames):
    """bricks of 0.45 m: the occupied bricks reach more than 2 x 2048 tiles in every frame (0.3 m: 4 284 in frame A, but 3 771 and 3 738 in
    B and C), so every workgroup of the culled launch takes a second and a third tile -- the stride loop of k_integrate_tiles with its
    tile-class flags -- over frames in which tiles fill up and empty out"""
    forms = sequence(rr, frames, SMALL_VIEW, 0.45, 2)
    assert all(f["items"] > 2 * f["grid"] and f["grid"] == 2048 for f in forms), forms


def _child_sequence(path, q):
    try:
        import torch  # noqa: F401
        import rgbd_recon_amd as rr
        forms = sequence(rr, rp.load_frames(rr, path), SMALL_VIEW, rp.BRICK, 25)
        q.put(("ok", forms))
    except BaseException as e:  # noqa: BLE001  (reported to the parent, which fails the test)
        q.put(("failed", f"{type(e).__name__}: {e}"))


def test_grid_stride_many_tiles_per_workgroup(rr, frames, tmp_path, monkeypatch):
    """the same sequence at the default brick size in a fresh process with 48 workgroups (RR_K1_GRID is read once per process): every
    workgroup walks 25 tiles and more in every frame (the frames have 1 627, 1 505 and 1 534 active tiles: 64 workgroups would leave
    frames B and C at 23 tiles each)"""
    import torch.multiprocessing as mp
    rp.save_frames(frames, str(tmp_path))
    monkeypatch.setenv("RR_K1_GRID", "48")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_child_sequence, args=(str(tmp_path), q))
    p.start()
    monkeypatch.delenv("RR_K1_GRID")
    p.join(420)
    if p.is_alive():
        p.terminate(); p.join(10)
        pytest.fail("the child process did not finish in 420 s")
    status, forms = q.get(timeout=5)
    assert status == "ok", forms
    assert p.exitcode == 0
    assert all(f["grid"] == 48 and f["items"] >= 25 * f["grid"] for f in forms), forms


def test_frames_through_the_lanes(rr, frames):
    """tsdf_frame_dev with the stage overlap on -- the integrate lane runs the generic kernel beside the other lanes' kernels -- against the
    same calls with every kernel on one stream, and against the oracle, frames queued back to back"""
    import torch
    kw = dict(rp.KW, view=SMALL_VIEW)
    lanes, one = rr.ReconIntegrationHip(frames[0], **kw), rr.ReconIntegrationHip(frames[0], lane_flags=rr.LANES_ONE_STREAM, **kw)
    mv, pr = rr.scene.default_view(*SMALL_VIEW)
    raw = [[torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ("depth", "quality", "silhouette", "color")] for sc in frames]
    torch.cuda.synchronize()
    order = (0, 1, 2, 0, 1)
    for n, k in enumerate(order):
        for o in (lanes, one):
            o.frame_dev(mv, pr, [t.data_ptr() for t in raw[k]])
        if n in (1, 4):                                    # frames 0-1 and 2-4 are queued without a host read in between
            orc = OracleRecon(frames[k], **kw)
            run(orc, mv, pr); orc.fillColors()
            for o, name in ((lanes, "lanes"), (one, "one stream")):
                assert o.integrate_form()["form"] == "generic"
                compare_bricks(o, orc, f"{name}, frame {n}")
                compare_frame(o, orc, f"{name}, frame {n}", drawn=True)
                compare_atlas(o, orc, f"{name}, frame {n}")
            assert_same(lanes.framebuffer()[0], one.framebuffer()[0], f"lanes vs one stream, frame {n}")
    lanes.close(); one.close()


def test_sparse_pool(rr, frames):
    """the generic kernel's pool-slot addressing: two culled frames in a pool exactly as large as the larger of them needs"""
    kw = dict(rp.KW, view=SMALL_VIEW)
    probe = rr.ReconIntegrationHip(frames[0], sparse_pool_tiles=N_TILES, **kw)
    need = []
    for k in (0, 1):
        probe.upload_frame(frames[k])
        probe.clearOccupiedBricks(); probe.markBricks(); probe.updateOccupiedBricks(); probe.integrate()
        need.append(probe.sparse_pool_stats()[0])
    probe.close()
    assert 500 < min(need) and max(need) < N_TILES and need[0] != need[1]
    hip = rr.ReconIntegrationHip(frames[0], sparse_pool_tiles=max(need), **kw)
    mv, pr = rr.scene.default_view(*SMALL_VIEW)
    for n, k in enumerate((0, 1)):
        hip.upload_frame(frames[k])
        orc = OracleRecon(frames[k], **kw)
        assert run(hip, mv, pr) == run(orc, mv, pr)
        generic(hip, True)
        assert hip.sparse_pool_stats() == (need[n], max(need))
        compare_bricks(hip, orc, f"sparse, frame {n}")
        compare_frame(hip, orc, f"sparse, frame {n}")
    hip.close()


def test_inverter_built_lut(rr, frames):
    """stream 0's inverse LUT from the library's own tsdf_invert_calibration at 0.007 m (from the 128^3 forward samples, as
    test_gpu_inverter.py feeds them): nearest-neighbour estimates instead of the closed form, -1 "invalid" texels wherever the tool
    found the voxel outside the frustum -- the filter blends them into their neighbours.  The oracle is handed the array the library
    produced."""
    sc = frames[0]
    xyz = np.ascontiguousarray(np.asarray(sc["cv_xyz"][0], np.float32).reshape(128, 128, 128, 3)[:, ::-1])
    inv, _ = rr.invert_calibration(xyz, sc["bbox_min"], sc["bbox_max"], rp.INV_RES)
    assert inv.shape == (rp.INV_RES[2], rp.INV_RES[1], rp.INV_RES[0], 4)
    ok = inv[..., 3] > 0
    assert 0.2 < ok.mean() < 1.0 and (inv[~ok] == -1).all() and np.isfinite(inv[ok]).all()
    assert not np.array_equal(inv.reshape(-1, 4), sc["cv_xyz_inv"][0])
    sc = rp.with_inverse_lut(sc, 0, inv)
    hip, orc = rr.ReconIntegrationHip(sc, **rp.KW), OracleRecon(sc, **rp.KW)
    mv, pr = rr.scene.default_view(*rp.KW["view"])
    for use_bricks in (True, False):
        for o in (hip, orc):
            o.setUseBricks(use_bricks)
            run(o, mv, pr)
        generic(hip, use_bricks)
        compare_frame(hip, orc, f"inverter-built LUT, use_bricks={use_bricks}", min_hits=20000)
    hip.close()


LADDER_RES = (96, 104, 96)


@pytest.mark.parametrize("inv_res,box,cls,form", [((48, 52, 48), (6, 6, 6), 2, "record"),          # LUT : volume 0.5
                                                  ((67, 73, 67), (7, 7, 7), 1, "lds_direct"),      # 0.7: 343 of 384 texels, 7 planes
                                                  ((82, 88, 82), (8, 8, 8), 0, "generic"),         # 0.85: 512 texels
                                                  ((137, 149, 137), (12, 13, 12), 0, "generic"),   # 1.43: the reference's ratio
                                                  ((48, 52, 140), (6, 6, 13), 0, "generic")])      # one axis alone pushes the box over
def test_ladder_of_lut_to_volume_ratios(rr, inv_res, box, cls, form):
    """the selection rule between the tested sizes: which kernel a LUT : volume ratio gets (box and class restated in helpers.lut_box_class
    from the LDS budget of 384 texels / 512 rows), and that kernel's volume, culled and dense, and one frame"""
    assert lut_box_class(LADDER_RES, inv_res) == (box, cls)
    sc = rp.scene_with_lut(rr, inv_res, n_streams=3, width=160, height=120, lut_res=24)
    kw = dict(res=LADDER_RES, brick_size=0.21, limit=0.03, view=(320, 180))
    hip, orc = rr.ReconIntegrationHip(sc, **kw), OracleRecon(sc, **kw)
    mv, pr = rr.scene.default_view(*kw["view"])
    for use_bricks in (True, False):
        for o in (hip, orc):
            o.setUseBricks(use_bricks)
            run(o, mv, pr)
        f = hip.integrate_form()
        assert f["form"] == form and f["culled"] == use_bricks, f
        compare_frame(hip, orc, f"LUT {inv_res}, use_bricks={use_bricks}", min_hits=500)
    hip.close()
