"""-m gpu: the client's overlays, "Draw TSDF" (tsdf_draw_calibvis, kinect::ReconCalibs::draw) and "Draw frustums" (tsdf_draw_frustums,
Frustum::draw), against the CPU reference tests/overlay_reference.py.  Every case compares the framebuffer bit for bit with the reference
fed the downloaded TSDF and the framebuffer as it was before the overlay."""
import ctypes as C

import numpy as np
import pytest

import overlay_reference as O

pytestmark = pytest.mark.gpu

TSDF_ERR_INVALID_ARGUMENT, TSDF_ERR_STATE = -1, -4
VIEW = (160, 90)
KW = dict(res=(64, 64, 64), brick_size=[2.0 / 8, 2.2 / 8, 2.0 / 8], limit=0.04, view=VIEW)
MOVED = [dict(), dict(sphere_c=(0.4, 0.7, -0.3), box_c=(-0.5, 1.5, 0.2)), dict(sphere_c=(-0.45, 1.5, 0.4), box_c=(0.2, 0.3, -0.6))]
_cache = {}


def scene_of(rr, n=4, inv_res=32, k=0):
    key = (n, inv_res, k)
    if key not in _cache:
        _cache[key] = rr.scene.make_scene(n_streams=n, width=160, height=120, lut_res=32, inv_res=inv_res, **MOVED[k % 3])
    return _cache[key]


def views(rr, w=VIEW[0], h=VIEW[1], near=0.1):
    pr = rr.scene.gl_flat(rr.scene.perspective(50.0, w / float(h), near, 200.0))
    eyes = [(0.0, 1.1, 3.0), (1.6, 1.4, 2.4), (-2.2, 2.6, -1.5)]
    return [(rr.scene.gl_flat(rr.scene.look_at(e, (0.0, 1.1, 0.0))), pr) for e in eyes]


def frame(o, mv, pr):
    o.clearOccupiedBricks(); o.markBricks(); o.updateOccupiedBricks(); o.integrate(); o.drawF(mv, pr)


def same(a, b):
    return ((a == b) | (np.isnan(a) & np.isnan(b))).all()


def calibvis_and_check(hip, sc, mv, pr, min_changed=50):
    vol = hip.tsdf()
    fc, fd = hip.framebuffer()
    hip.drawCalibVis(mv, pr)
    gc, gd = hip.framebuffer()
    wc, wd = O.draw_calibvis(vol, sc["inv_res"], sc["bbox_min"], sc["bbox_max"], mv, pr, hip.view, fc, fd)
    assert same(gd, wd), f"{(~((gd == wd) | np.isnan(gd) & np.isnan(wd))).sum()} depths differ"
    assert same(gc, wc), "colours differ"
    assert (wd != fd).sum() >= min_changed
    return wc, wd


def frustum_inputs(rr, sc):
    r = sc["lut_res"]
    corners = [O.frustum_corners(sc["cv_xyz"][i], r) for i in range(sc["n"])]
    cams = [rr.frustum_from_volume(np.asarray(sc["cv_xyz"][i], np.float32).reshape(int(r[2]), int(r[1]), int(r[0]), 3))[1] for i in range(sc["n"])]
    return corners, cams


def frustums_and_check(rr, hip, sc, mv, pr, min_changed=50):
    fc, fd = hip.framebuffer()
    hip.drawFrustums(mv, pr)
    gc, gd = hip.framebuffer()
    wc, wd = O.draw_frustums(*frustum_inputs(rr, sc), mv, pr, hip.view, fc, fd)
    assert same(gd, wd) and same(gc, wc)
    assert (wd != fd).sum() >= min_changed
    return wc, wd


def test_calibvis_after_drawf_three_views(rr, small_scene):
    hip = rr.ReconIntegrationHip(small_scene, **KW)
    for mv, pr in views(rr):
        frame(hip, mv, pr)
        calibvis_and_check(hip, small_scene, mv, pr)


@pytest.mark.parametrize("inv_res", [96, 16])
def test_calibvis_grid_finer_and_coarser_than_the_volume(rr, inv_res):
    sc = scene_of(rr, n=2, inv_res=inv_res)
    hip = rr.ReconIntegrationHip(sc, **KW)
    mv, pr = views(rr)[0]
    frame(hip, mv, pr)
    calibvis_and_check(hip, sc, mv, pr, min_changed=5)                   # (16^3: 17 pixels in front of the surface in this view)
    assert hip.calibvis_stats()[0] == inv_res ** 3


def test_calibvis_empty_space_skip_and_green_clear_value(rr, small_scene):
    mv, pr = views(rr)[1]
    hip = rr.ReconIntegrationHip(small_scene, **KW)                       # clear value -0.04: discarded, whole blocks skipped
    frame(hip, mv, pr)
    calibvis_and_check(hip, small_scene, mv, pr)
    n, skipped = hip.calibvis_stats()
    assert n == 32 ** 3 and 0 < skipped < n
    lo = rr.ReconIntegrationHip(small_scene, **dict(KW, limit=0.005))    # clear value -0.005 > -0.01: every empty tile is drawn green
    frame(lo, mv, pr)
    wc, wd = calibvis_and_check(lo, small_scene, mv, pr)
    assert lo.calibvis_stats() == (n, 0)
    green = (wc[..., 1] == np.float32(0.5)) & (wc[..., 0] == 0) & (wc[..., 2] == 0)
    assert green.sum() > 100
    lo.setTsdfLimit(0.04)                                                 # the limit changes after the integrate: no stale skip
    lo.drawF(mv, pr)
    calibvis_and_check(lo, small_scene, mv, pr)
    assert lo.calibvis_stats() == (n, 0)


def test_calibvis_sparse_pool(rr, small_scene):
    hip = rr.ReconIntegrationHip(small_scene, sparse_pool_tiles=4096, **KW)
    for mv, pr in views(rr)[:2]:
        frame(hip, mv, pr)
        calibvis_and_check(hip, small_scene, mv, pr)


def test_calibvis_crafted_volume_and_framebuffer(rr, small_scene):
    """every colour branch, a depth tie with the framebuffer (not drawn) and ties between points (the lower index wins)"""
    hip = rr.ReconIntegrationHip(small_scene, **KW)
    rng = np.random.default_rng(3)
    values = np.array([-0.04, -0.01, -0.005, 0.0, 0.005, 0.01, 0.02], np.float32)
    blocks = rng.choice(values, size=(32, 32, 32)).astype(np.float32)
    mask = rng.random((32, 32, 32)) < 0.2
    blocks[mask] = rng.uniform(-0.03, 0.03, int(mask.sum()))
    vol = np.kron(blocks, np.ones((2, 2, 2), np.float32))                 # 2^3 blocks: the 32^3 grid samples each block's value exactly
    hip.set_tsdf(vol)
    mv, pr = views(rr)[0]
    ids, d, ok, xw, yw, zw = O.calibvis_points(hip.tsdf(), small_scene["inv_res"], small_scene["bbox_min"], small_scene["bbox_max"], mv, pr, VIEW)
    assert all((d[ok] == np.float32(v)).any() for v in values if v > -0.01) and (d == np.float32(-0.01)).any()
    fc = rng.uniform(0, 1, (VIEW[1], VIEW[0], 4)).astype(np.float32)
    fd = rng.uniform(0.5, 1.0, (VIEW[1], VIEW[0])).astype(np.float32)
    # ties with the framebuffer: the nearest passing point's own depth at some pixels (GL_LESS fails there)
    ties = 0
    for i in np.flatnonzero(ok)[::97]:
        for px, py in O.point_pixels(xw[i], yw[i], 1, VIEW):
            fd[py, px] = zw[i]
            ties += 1
    assert ties > 10
    hip.set_framebuffer(fc, fd)
    calibvis_and_check(hip, small_scene, mv, pr, min_changed=200)
    # every point on at most four pixels at z = 0.5 exactly: P = diag(1e-6, 1e-6, 1e-20, 1)
    flat = np.diag([1e-6, 1e-6, 1e-20, 1.0]).astype(np.float32).T.reshape(16)
    hip.set_framebuffer(fc, np.ones_like(fd))
    wc, wd = calibvis_and_check(hip, small_scene, np.eye(4, dtype=np.float32).reshape(16), flat, min_changed=1)
    assert 1 <= (wd == np.float32(0.5)).sum() <= 4                      # window (80 -/+ 1e-5, 45 + 1e-5): pixels 79 / 80 x 44 / 45


def test_frustums_three_views_and_near_plane(rr, small_scene):
    hip = rr.ReconIntegrationHip(small_scene, **KW)
    for mv, pr in views(rr):
        frame(hip, mv, pr)
        frustums_and_check(rr, hip, small_scene, mv, pr)
    # an eye inside stream 0's frustum, looking away from its camera: the lines from its near corners cross the near plane
    _, cams = frustum_inputs(rr, small_scene)
    eye = 0.6 * cams[0] + 0.4 * np.array([0.0, 1.1, 0.0], np.float32)
    pr = rr.scene.gl_flat(rr.scene.perspective(70.0, VIEW[0] / float(VIEW[1]), 0.5, 200.0))
    mv = rr.scene.gl_flat(rr.scene.look_at(tuple(eye), (-3 * cams[0][0], 1.1, -3 * cams[0][2])))
    corners, _ = frustum_inputs(rr, small_scene)
    clipped = 0
    for i, j in O.FRUSTUM_LINES:
        a, b = O.frustum_clip(mv, pr, corners[0][i]), O.frustum_clip(mv, pr, corners[0][j])
        clipped += ((a[2] + a[3] < 0) != (b[2] + b[3] < 0))
    assert clipped >= 2
    frame(hip, mv, pr)
    frustums_and_check(rr, hip, small_scene, mv, pr)


def test_calibvis_then_frustums_in_the_clients_order(rr, small_scene):
    hip = rr.ReconIntegrationHip(small_scene, **KW)
    mv, pr = views(rr)[1]
    frame(hip, mv, pr)
    vol = hip.tsdf()
    fc, fd = hip.framebuffer()
    hip.drawCalibVis(mv, pr)
    hip.drawFrustums(mv, pr)
    gc, gd = hip.framebuffer()
    wc, wd = O.draw_calibvis(vol, small_scene["inv_res"], small_scene["bbox_min"], small_scene["bbox_max"], mv, pr, VIEW, fc, fd)
    wc, wd = O.draw_frustums(*frustum_inputs(rr, small_scene), mv, pr, VIEW, wc, wd)
    assert same(gd, wd) and same(gc, wc)


def test_overlay_after_every_frame_through_the_lanes(rr):
    """eight frames of a moving scene through tsdf_frame_dev, an overlay after each, stage overlap on and off: the same framebuffers"""
    import torch
    scs = [scene_of(rr, k=k) for k in range(3)]
    mvs = views(rr)
    dev = []
    for sc in scs:
        ts = [torch.from_numpy(np.ascontiguousarray(sc[key])).cuda() for key in ("depth", "quality", "silhouette", "color")]
        dev.append((ts, tuple(t.data_ptr() for t in ts)))
    torch.cuda.synchronize()
    out = {}
    for overlap in (True, False):
        hip = rr.ReconIntegrationHip(scs[0], **KW)
        hip.set_stage_overlap(overlap)
        got = []
        for n in range(8):
            mv, pr = mvs[n % 3]
            hip.frame_dev(mv, pr, new_frame=dev[n % 3][1], complete=True)
            hip.drawCalibVis(mv, pr)
            if n % 2:
                hip.drawFrustums(mv, pr)
            got.append(hip.framebuffer())
        out[overlap] = got
        hip.close()
    for (ac, ad), (bc, bd) in zip(out[True], out[False]):
        assert same(ad, bd) and same(ac, bc)
    # and the last frame against the reference (its own TSDF from a context that draws nothing else)
    ref = rr.ReconIntegrationHip(scs[7 % 3], **KW)
    mv, pr = mvs[7 % 3]
    frame(ref, mv, pr)
    vol = ref.tsdf()
    fc, fd = ref.framebuffer()
    wc, wd = O.draw_calibvis(vol, scs[0]["inv_res"], scs[0]["bbox_min"], scs[0]["bbox_max"], mv, pr, VIEW, fc, fd)
    wc, wd = O.draw_frustums(*frustum_inputs(rr, scs[0]), mv, pr, VIEW, wc, wd)
    assert same(out[True][7][1], wd) and same(out[True][7][0], wc)


def test_overlay_errors(rr, small_scene):
    mv, pr = views(rr)[0]
    bare = rr.ReconIntegrationHip(small_scene, upload=False, **KW)         # no calibration
    for call in (bare.drawCalibVis, bare.drawFrustums):
        with pytest.raises(rr.TsdfError) as e:
            call(mv, pr)
        assert e.value.code == TSDF_ERR_STATE
    slab = rr.ReconIntegrationHip(small_scene, slab=(0, 32), **KW)
    with pytest.raises(rr.TsdfError) as e:
        slab.drawCalibVis(mv, pr)
    assert e.value.code == TSDF_ERR_STATE
    hip = rr.ReconIntegrationHip(small_scene, **KW)
    frame(hip, mv, pr)
    for setup, undo in ((lambda: hip.setColorMaskMode(1), lambda: hip.setColorMaskMode(0)),
                        (lambda: hip.setViewportOrigin(8, 0), lambda: hip.setViewportOrigin(0, 0)),
                        (lambda: hip.setViewportOffset(0.5, 0), lambda: hip.setViewportOffset(0, 0))):
        setup()
        for call in (hip.drawCalibVis, hip.drawFrustums):
            with pytest.raises(rr.TsdfError) as e:
                call(mv, pr)
            assert e.value.code == TSDF_ERR_STATE
        undo()
    L, c = rr.load_library(), hip._c
    m = np.ascontiguousarray(mv, np.float32)
    fp = m.ctypes.data_as(C.POINTER(C.c_float))
    zero = np.zeros(16, np.float32)
    zp = zero.ctypes.data_as(C.POINTER(C.c_float))
    for fn in (L.tsdf_draw_calibvis, L.tsdf_draw_frustums):
        assert fn(c, None, fp) == TSDF_ERR_INVALID_ARGUMENT and fn(c, fp, None) == TSDF_ERR_INVALID_ARGUMENT
        assert fn(c, zp, fp) == TSDF_ERR_INVALID_ARGUMENT and fn(c, fp, zp) == TSDF_ERR_INVALID_ARGUMENT
    with pytest.raises(rr.TsdfError) as e:
        hip.setActiveKinect(small_scene["n"])
    assert e.value.code == TSDF_ERR_INVALID_ARGUMENT
    # setActiveKinect changes no output
    before = hip.framebuffer()
    hip.drawCalibVis(mv, pr)
    a = hip.framebuffer()
    hip.set_framebuffer(*before)
    hip.setActiveKinect(small_scene["n"] - 1)
    hip.drawCalibVis(mv, pr)
    b = hip.framebuffer()
    assert same(a[0], b[0]) and same(a[1], b[1])
