"""-m gpu: the occupied-brick wireframes (tsdf_draw_bricks / tsdf_set_draw_bricks; ReconIntegration::drawOccupiedBricks) against
tests/brick_overlay_reference.py fed the brick flags tsdf_download_bricks returns and the framebuffer downloaded just before the overlay.
Every comparison is bit for bit, colour and depth, every pixel.  No test passes on an empty picture: the list is not empty and the
reference overlay changes at least one pixel per drawn brick on average (checked on the reference's own output before the comparison)."""
import numpy as np
import pytest

import brick_overlay_reference as B
import refpoint_scene as rp

pytestmark = pytest.mark.gpu

TSDF_ERR_STATE = -4
VIEW = (160, 90)
KW = dict(res=(64, 64, 64), brick_size=[2.0 / 8, 2.2 / 8, 2.0 / 8], limit=0.04, view=VIEW)
# bricks of 4 voxels, and of 10 voxels (never aligned with the 8-voxel storage tiles; 6.4 bricks per axis: the last one is clipped by the
# box and drawn at full size), the y size different from x and z in both
BRICKS_4 = [2.0 / 16, 2.2 / 16, 2.0 / 16]
BRICKS_10 = [10 * 2.0 / 64, 10 * 2.2 / 64, 10 * 2.0 / 64]


def views(rr, w=VIEW[0], h=VIEW[1], near=0.1):
    pr = rr.scene.gl_flat(rr.scene.perspective(50.0, w / float(h), near, 200.0))
    eyes = [(0.0, 1.1, 3.0), (1.6, 1.4, 2.4), (-2.2, 2.6, -1.5)]
    return [(rr.scene.gl_flat(rr.scene.look_at(e, (0.0, 1.1, 0.0))), pr) for e in eyes]


def inside_view(rr, sc):
    """an eye inside the volume, beside the box and looking at the sphere: bricks straddle the near plane and lie behind the eye (checked
    with the oracle's brick list and framebuffer on the CPU: 15 / 32 of 247 bricks of 4 voxels, 9 / 5 of 49 bricks of 10 voxels, and
    2587 / 1522 pixels changed)"""
    pr = rr.scene.gl_flat(rr.scene.perspective(70.0, VIEW[0] / float(VIEW[1]), 0.3, 200.0))
    return rr.scene.gl_flat(rr.scene.look_at((0.45, 0.45, 0.55), (0.0, 1.1, 0.0))), pr


def along_z_view():
    """orthographic, along -z: the front and back edges of every brick of a column fall on the same pixels"""
    pr = np.zeros(16, np.float32)
    pr[0], pr[5], pr[10], pr[13], pr[15] = 0.9, 0.8, -0.4, -0.88, 1.0
    return np.eye(4, dtype=np.float32).reshape(16), pr


def frame(o, mv, pr):
    o.clearOccupiedBricks(); o.markBricks(); o.updateOccupiedBricks(); o.integrate(); o.drawF(mv, pr)


def same(a, b):
    return ((a == b) | (np.isnan(a) & np.isnan(b))).all()


def reference(hip, sc, mv, pr, fc, fd, per_brick=True):
    st = {}
    wc, wd = B.draw_bricks(hip.bricks()[1], hip.res_bricks, hip.brick_size, sc["bbox_min"], mv, pr, hip.view, fc, fd, stats=st)
    assert st["bricks"] > 0, "no occupied brick"
    if per_brick:
        assert st["changed"] >= st["bricks"], st
    else:
        assert st["changed"] > 0, st
    return wc, wd, st


def overlay_and_check(hip, sc, mv, pr, per_brick=True):
    fc, fd = hip.framebuffer()
    wc, wd, st = reference(hip, sc, mv, pr, fc, fd, per_brick)
    hip.drawOccupiedBricks(mv, pr)
    gc, gd = hip.framebuffer()
    print(f"bricks {st['bricks']} fragments {st['fragments']} failed {st['failed']} tie pixels {st['tie_pixels']} changed {st['changed']} "
          f"depths off {int((~((gd == wd) | np.isnan(gd) & np.isnan(wd))).sum())}")
    assert same(gd, wd), f"{int((gd != wd).sum())} depths differ"
    assert same(gc, wc), "colours differ"
    return gc, gd, st


# ---------------------------------------------------------------------- 1. after drawF
@pytest.mark.parametrize("bricks", [BRICKS_4, BRICKS_10], ids=["bricks4", "bricks10"])
@pytest.mark.parametrize("fill", [True, False], ids=["fill", "nofill"])
def test_after_drawf_three_views_and_an_eye_inside_the_volume(rr, small_scene, bricks, fill):
    hip = rr.ReconIntegrationHip(small_scene, **dict(KW, brick_size=bricks))
    hip.setColorFilling(fill)
    for mv, pr in views(rr) + [inside_view(rr, small_scene)]:
        frame(hip, mv, pr)
        overlay_and_check(hip, small_scene, mv, pr)
    mv, pr = inside_view(rr, small_scene)
    ids = B.brick_ids(hip.bricks()[1], hip.numBricks())
    near_in = (lambda c: c[2] + c[3] >= 0)(B.vertex_clip(ids, hip.res_bricks, hip.brick_size, small_scene["bbox_min"], mv, pr))
    assert (near_in.any(1) & ~near_in.all(1)).any(), "no brick straddles the near plane"
    assert (~near_in.any(1)).any(), "no brick behind the eye"


# ---------------------------------------------------------------------- 2. crafted framebuffers
def test_crafted_depth_equal_one_ulp_behind_and_ties_along_a_brick_axis(rr, small_scene):
    hip = rr.ReconIntegrationHip(small_scene, **KW)
    mv, pr = along_z_view()
    hip.clearOccupiedBricks(); hip.markBricks(); hip.updateOccupiedBricks()
    ids = B.brick_ids(hip.bricks()[1], hip.numBricks())
    prim, px, py, z = B.brick_fragments(ids, hip.res_bricks, hip.brick_size, small_scene["bbox_min"], mv, pr, VIEW)
    rng = np.random.default_rng(11)
    fc = rng.uniform(0, 1, (VIEW[1], VIEW[0], 4)).astype(np.float32)
    fd = np.ones((VIEW[1], VIEW[0]), np.float32)
    k = np.arange(prim.size)
    eq, ulp = k % 7 == 0, k % 7 == 1
    fd[py[ulp], px[ulp]] = np.nextafter(z[ulp], np.float32(1))            # one ulp behind that fragment: it passes
    fd[py[eq], px[eq]] = z[eq]                                            # its own depth: strict < fails
    assert eq.sum() > 20 and ulp.sum() > 20
    hip.set_framebuffer(fc, fd)
    _, _, st = overlay_and_check(hip, small_scene, mv, pr)
    assert st["failed"] >= 1, "no fragment failed the strict depth test"
    assert st["tie_pixels"] >= 1, "no pixel was decided by the primitive index"


# ---------------------------------------------------------------------- 3. the flag
def test_flag_in_drawf_equals_drawf_then_overlay(rr, small_scene):
    a, b = rr.ReconIntegrationHip(small_scene, **KW), rr.ReconIntegrationHip(small_scene, **KW)
    a.setDrawBricks(True)
    for mv, pr in views(rr)[:2]:
        frame(a, mv, pr)
        frame(b, mv, pr)
        gc, gd, _ = overlay_and_check(b, small_scene, mv, pr)
        fc, fd = a.framebuffer()
        assert same(fd, gd) and same(fc, gc)


def test_flag_through_frame_dev_with_and_without_stage_overlap(rr, small_scene):
    moved = rr.scene.make_scene(n_streams=4, width=160, height=120, lut_res=32, inv_res=32, sphere_c=(0.4, 0.7, -0.3), box_c=(-0.5, 1.5, 0.2))
    on, off, never = (rr.ReconIntegrationHip(small_scene, **KW) for _ in range(3))
    off.set_stage_overlap(False)
    on.setDrawBricks(True); off.setDrawBricks(True)
    vs = views(rr)
    for f in range(6):
        mv, pr = vs[f % 3]
        sc = moved if f % 2 else small_scene
        for o in (on, off, never):
            o.upload_frame(sc)
            o.frame_dev(mv, pr)
        if f == 4:                                                        # switched off again: the next frame is a context's that never had it on
            on.setDrawBricks(False); off.setDrawBricks(False)
        nc, nd = never.framebuffer()
        (ac, ad), (bc, bd) = on.framebuffer(), off.framebuffer()
        assert same(ad, bd) and same(ac, bc), f"frame {f}: stage overlap changes the picture"
        if f < 5:
            wc, wd, _ = reference(never, sc, mv, pr, nc, nd)
            assert same(ad, wd) and same(ac, wc), f"frame {f}"
        else:
            assert same(ad, nd) and same(ac, nc), "the frame after the flag was switched off"


def test_after_the_other_back_ends_and_in_the_clients_order(rr, small_scene):
    mv, pr = views(rr)[1]
    pts = rr.ReconIntegrationHip(small_scene, **KW)
    pts.upload_normals(small_scene["normals"])
    pts.clearOccupiedBricks(); pts.markBricks(); pts.updateOccupiedBricks()
    pts.drawPoints(mv, pr)
    overlay_and_check(pts, small_scene, mv, pr)
    tri = rr.ReconIntegrationHip(small_scene, **KW)
    tri.clearOccupiedBricks(); tri.markBricks(); tri.updateOccupiedBricks()
    tri.drawTrigrid(mv, pr)
    overlay_and_check(tri, small_scene, mv, pr)
    hip = rr.ReconIntegrationHip(small_scene, **KW)
    frame(hip, mv, pr)
    hip.drawCalibVis(mv, pr)
    hip.drawFrustums(mv, pr)
    gc, gd, _ = overlay_and_check(hip, small_scene, mv, pr)
    hip.drawBBox(mv, pr)
    import client_overlay_reference as R
    wc, wd = R.draw_bbox(small_scene["bbox_min"], small_scene["bbox_max"], mv, pr, hip.view, gc, gd)
    fc, fd = hip.framebuffer()
    assert same(fd, wd) and same(fc, wc)


# ---------------------------------------------------------------------- 4. sparse pool, Z slab
def test_sparse_pool_and_z_slab_give_the_unpartitioned_pixels(rr, small_scene):
    mv, pr = views(rr)[1]
    dense = rr.ReconIntegrationHip(small_scene, **KW)
    frame(dense, mv, pr)
    before = dense.framebuffer()
    gc, gd, _ = overlay_and_check(dense, small_scene, mv, pr)
    sparse = rr.ReconIntegrationHip(small_scene, sparse_pool_tiles=4096, **KW)
    frame(sparse, mv, pr)
    sparse.drawOccupiedBricks(mv, pr)
    sc_, sd_ = sparse.framebuffer()
    assert same(sd_, gd) and same(sc_, gc)
    slab = rr.ReconIntegrationHip(small_scene, slab=(32, 64), recompute_halo=True, **KW)
    slab.clearOccupiedBricks(); slab.markBricks(); slab.updateOccupiedBricks()
    assert (slab.bricks()[1] == dense.bricks()[1]).all()
    slab.set_framebuffer(*before)
    slab.drawOccupiedBricks(mv, pr)
    lc, ld = slab.framebuffer()
    assert same(ld, gd) and same(lc, gc)


# ---------------------------------------------------------------------- 5. no list, stereo state
def test_no_list_draws_nothing_and_stereo_state_is_refused(rr, small_scene):
    mv, pr = views(rr)[0]
    rng = np.random.default_rng(2)
    fc = rng.uniform(0, 1, (VIEW[1], VIEW[0], 4)).astype(np.float32)
    fd = rng.uniform(0.5, 1, (VIEW[1], VIEW[0])).astype(np.float32)

    def unchanged(o):
        c, d = o.framebuffer()
        return same(c, fc) and same(d, fd)
    fresh = rr.ReconIntegrationHip(small_scene, **KW)
    fresh.set_framebuffer(fc, fd)
    fresh.drawOccupiedBricks(mv, pr)                                      # no update yet: TSDF_OK, nothing drawn
    assert unchanged(fresh)
    hip = rr.ReconIntegrationHip(small_scene, **KW)
    frame(hip, mv, pr)
    overlay_and_check(hip, small_scene, mv, pr)
    hip.setBrickSize(BRICKS_4)                                            # a new grid: no list until the next update
    hip.set_framebuffer(fc, fd)
    hip.drawOccupiedBricks(mv, pr)
    assert unchanged(hip)
    frame(hip, mv, pr)                                                    # ... which brings it back
    overlay_and_check(hip, small_scene, mv, pr)
    hip.set_framebuffer(fc, fd)
    for setup, undo in ((lambda: hip.setColorMaskMode(1), lambda: hip.setColorMaskMode(0)),
                        (lambda: hip.setViewportOrigin(8, 0), lambda: hip.setViewportOrigin(0, 0)),
                        (lambda: hip.setViewportOffset(0.5, 0), lambda: hip.setViewportOffset(0, 0))):
        setup()
        hip.setDrawBricks(False)
        with pytest.raises(rr.TsdfError) as e:
            hip.drawOccupiedBricks(mv, pr)
        assert e.value.code == TSDF_ERR_STATE
        hip.setDrawBricks(True)
        with pytest.raises(rr.TsdfError) as e:
            hip.drawF(mv, pr)
        assert e.value.code == TSDF_ERR_STATE
        undo()
        assert unchanged(hip), "a refused call queued something"
    hip.drawF(mv, pr)
    assert not unchanged(hip)


# ---------------------------------------------------------------------- 6. at size
def test_at_the_reference_operating_point(rr):
    """200 x 221 x 200 voxels, 20 x 22 x 20 bricks of 10 voxels, 1280 x 720 (tests/refpoint_scene.py; the occupied bricks depend on the
    forward LUTs and the frame only, so a small inverse LUT serves)"""
    sc = rp.make_frames(rr, n_frames=1, inv_res=(64, 64, 64))[0]
    hip = rr.ReconIntegrationHip(sc, **rp.KW)
    assert tuple(hip.res) == rp.RES and tuple(hip.res_bricks) == rp.RES_BRICKS
    mv, pr = rr.scene.default_view(*rp.KW["view"])
    frame(hip, mv, pr)
    overlay_and_check(hip, sc, mv, pr)


def test_at_the_headline_configuration(rr):
    """512^3 voxels, bricks of 8 voxels, 1280 x 720: the benchmark's scene, brick size and view"""
    sc = rr.scene.make_scene(n_streams=4, width=640, height=480, lut_res=128, inv_res=128)
    ext = np.asarray(sc["bbox_max"], np.float64) - np.asarray(sc["bbox_min"], np.float64)
    hip = rr.ReconIntegrationHip(sc, res=(512, 512, 512), brick_size=[float(ext[a]) / 512 * 8 for a in range(3)], limit=0.01, view=(1280, 720))
    assert tuple(hip.res) == (512, 512, 512) and all(b in (64, 65) for b in hip.res_bricks)   # (fp32: 2.2 / (2.2 / 512 * 8) rounds up to a 65th layer in y)
    mv, pr = rr.scene.default_view(1280, 720)
    frame(hip, mv, pr)
    _, _, st = overlay_and_check(hip, sc, mv, pr)
    assert st["bricks"] > 1000


# ---------------------------------------------------------------------- the C++ adapter, headless
def test_frame_harness_shows_the_wireframes(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host, lib = os.path.join(root, "rgbd-recon_amd", "host"), os.path.join(root, "rgbd-recon_amd")
    exe = str(tmp_path / "frame_harness")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(host, "frame_harness.cpp"), "-o", exe,
                           "-L" + lib, "-lrgbd_recon_hip", "-Wl,-rpath," + lib])
    plain = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and "wireframe" not in plain.stdout, plain.stdout + plain.stderr
    wire = subprocess.run([exe, "--draw-bricks"], capture_output=True, text=True, timeout=120)
    assert wire.returncode == 0, wire.stdout + wire.stderr
    assert int(wire.stdout.split(" wireframe pixels")[0].split()[-1]) > 0
