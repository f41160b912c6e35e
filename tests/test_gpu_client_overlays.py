"""-m gpu: the client's bounding-box wireframe (tsdf_draw_bbox, gloost::BoundingBox::draw) and texture view (tsdf_draw_textures,
TextureBlitter::blit), against tests/client_overlay_reference.py fed the framebuffer downloaded just before the overlay.  Every comparison
is bit for bit; the atlas of the texture view is the oracle's literal two-atlas sequence."""
import ctypes as C

import numpy as np
import pytest

import client_overlay_reference as R
import overlay_reference as O
from oracle.oracle import OracleRecon

pytestmark = pytest.mark.gpu

TSDF_ERR_INVALID_ARGUMENT, TSDF_ERR_STATE = -1, -4
VIEW = (160, 90)
KW = dict(res=(64, 64, 64), brick_size=[2.0 / 8, 2.2 / 8, 2.0 / 8], limit=0.04, view=VIEW)


def views(rr, w=VIEW[0], h=VIEW[1], near=0.1):
    pr = rr.scene.gl_flat(rr.scene.perspective(50.0, w / float(h), near, 200.0))
    eyes = [(0.0, 1.1, 3.0), (1.6, 1.4, 2.4), (-2.2, 2.6, -1.5)]
    return [(rr.scene.gl_flat(rr.scene.look_at(e, (0.0, 1.1, 0.0))), pr) for e in eyes]


def frame(o, mv, pr):
    o.clearOccupiedBricks(); o.markBricks(); o.updateOccupiedBricks(); o.integrate(); o.drawF(mv, pr)


def same(a, b):
    return ((a == b) | (np.isnan(a) & np.isnan(b))).all()


def limits_image(hip):
    """unit 16 as GL holds it: tsdf_download_image's peels are (min z, min(-z), min back-face z, 0), the MIN blend of bricks.fs"""
    return hip.view_images()[3]


def bbox_and_check(hip, sc, mv, pr, min_changed=50):
    fc, fd = hip.framebuffer()
    hip.drawBBox(mv, pr)
    gc, gd = hip.framebuffer()
    wc, wd = R.draw_bbox(sc["bbox_min"], sc["bbox_max"], mv, pr, hip.view, fc, fd)
    assert same(gd, wd), f"{int((gd != wd).sum())} depths differ"
    assert same(gc, wc), "colours differ"
    assert (wd != fd).sum() >= min_changed
    return wc, wd


def textures_and_check(hip, which, src):
    fc, fd = hip.framebuffer()
    hip.drawTextures(which)
    gc, gd = hip.framebuffer()
    wc = R.blit(src, hip.view, fc)
    assert same(gd, fd), "the texture view wrote depth"
    assert same(gc, wc), f"{int((~((gc == wc) | np.isnan(gc) & np.isnan(wc))).sum())} colour values differ"


def test_bbox_after_drawf_three_views_and_an_eye_inside_the_box(rr, small_scene):
    hip = rr.ReconIntegrationHip(small_scene, **KW)
    for mv, pr in views(rr):
        frame(hip, mv, pr)
        bbox_and_check(hip, small_scene, mv, pr)
    lo, hi = np.asarray(small_scene["bbox_min"], np.float32), np.asarray(small_scene["bbox_max"], np.float32)
    eye = lo + 0.3 * (hi - lo)
    pr = rr.scene.gl_flat(rr.scene.perspective(70.0, VIEW[0] / float(VIEW[1]), 0.3, 200.0))
    mv = rr.scene.gl_flat(rr.scene.look_at(tuple(eye), tuple(eye + np.array([0.3, 0.1, -1.0], np.float32))))
    crossing = sum((a[2] + a[3] < 0) != (b[2] + b[3] < 0)
                   for a, b in ((O.frustum_clip(mv, pr, p), O.frustum_clip(mv, pr, q)) for p, q in R.bbox_segments(lo, hi)))
    assert crossing >= 4                                                  # segments that cross the near plane
    frame(hip, mv, pr)
    bbox_and_check(hip, small_scene, mv, pr)


def test_bbox_after_the_other_back_ends(rr, small_scene):
    mv, pr = views(rr)[1]
    pts = rr.ReconIntegrationHip(small_scene, **KW)
    pts.upload_normals(small_scene["normals"])
    pts.drawPoints(mv, pr)
    bbox_and_check(pts, small_scene, mv, pr)
    tri = rr.ReconIntegrationHip(small_scene, **KW)
    tri.drawTrigrid(mv, pr)
    bbox_and_check(tri, small_scene, mv, pr)
    mvt = rr.ReconIntegrationHip(small_scene, **KW)
    mvt.upload_raw_frame(small_scene)
    mvt.drawMVT(mv, pr)
    bbox_and_check(mvt, small_scene, mv, pr)


def test_bbox_after_calibvis_and_frustums_in_the_clients_order(rr, small_scene):
    hip = rr.ReconIntegrationHip(small_scene, **KW)
    mv, pr = views(rr)[0]
    frame(hip, mv, pr)
    hip.drawCalibVis(mv, pr)
    hip.drawFrustums(mv, pr)
    bbox_and_check(hip, small_scene, mv, pr)


def test_bbox_over_crafted_depth_ties_and_near_misses(rr, small_scene):
    hip = rr.ReconIntegrationHip(small_scene, **KW)
    mv, pr = views(rr)[1]
    frame(hip, mv, pr)
    rng = np.random.default_rng(11)
    fc = rng.uniform(0, 1, (VIEW[1], VIEW[0], 4)).astype(np.float32)
    fd = np.ones((VIEW[1], VIEW[0]), np.float32)
    frags = R.bbox_fragments(small_scene["bbox_min"], small_scene["bbox_max"], mv, pr, VIEW)
    ties = misses = 0
    for n, (s, px, py, z) in enumerate(frags):
        if n % 5 == 0:
            fd[py, px] = z; ties += 1                                     # GL_LESS fails at its own depth
        elif n % 5 == 1:
            fd[py, px] = np.nextafter(z, np.float32(1)); misses += 1      # ... and passes one ulp above it
    assert ties > 20 and misses > 20
    hip.set_framebuffer(fc, fd)
    bbox_and_check(hip, small_scene, mv, pr, min_changed=20)


def test_bbox_sparse_pool(rr, small_scene):
    hip = rr.ReconIntegrationHip(small_scene, sparse_pool_tiles=4096, **KW)
    for mv, pr in views(rr)[:2]:
        frame(hip, mv, pr)
        bbox_and_check(hip, small_scene, mv, pr)
        textures_and_check(hip, 1, limits_image(hip))


def test_textures_unit15_is_the_oracles_atlas(rr, small_scene):
    """two frames from different views (the atlas of the second is the other one of the pair), then a frame without colour filling: the
    view keeps showing the last filled atlas"""
    hip, orc = rr.ReconIntegrationHip(small_scene, **KW), OracleRecon(small_scene, **KW)
    vs = views(rr)
    for mv, pr in vs[:2]:
        for o in (hip, orc):
            frame(o, mv, pr)
        atlas = orc.atlas()[0]
        assert (atlas[..., 1] == 1).any() and (atlas[..., 3] > 0).any()
        textures_and_check(hip, 0, atlas)
        bbox_and_check(hip, small_scene, mv, pr)
        textures_and_check(hip, 0, atlas)                                 # the client's order: the bbox, then the texture view
    for o in (hip, orc):
        o.setColorFilling(False)
        frame(o, *vs[2])
    textures_and_check(hip, 0, atlas)


def test_textures_unit16_with_and_without_space_skipping(rr, small_scene):
    hip = rr.ReconIntegrationHip(small_scene, **KW)
    vs = views(rr)
    frame(hip, *vs[0])
    frame(hip, *vs[1])
    img = limits_image(hip)
    assert (img[..., 0] < 1).sum() > 500 and (img[..., 1] < 0).any()
    textures_and_check(hip, 1, img)
    hip.setSpaceSkip(False)                                               # drawF no longer redraws m_view_depth: the old image stays
    frame(hip, *vs[2])
    textures_and_check(hip, 1, img)


def test_texture_view_and_bbox_errors(rr, small_scene):
    mv, pr = views(rr)[0]
    fresh = rr.ReconIntegrationHip(small_scene, **KW)
    for which in (0, 1):
        with pytest.raises(rr.TsdfError) as e:
            fresh.drawTextures(which)
        assert e.value.code == TSDF_ERR_STATE
    with pytest.raises(rr.TsdfError) as e:
        fresh.drawTextures(2)
    assert e.value.code == TSDF_ERR_INVALID_ARGUMENT
    plain = rr.ReconIntegrationHip(small_scene, **KW)
    plain.setColorFilling(False); plain.setSpaceSkip(False)
    frame(plain, mv, pr)
    for which in (0, 1):
        with pytest.raises(rr.TsdfError) as e:
            plain.drawTextures(which)
        assert e.value.code == TSDF_ERR_STATE
    hip = rr.ReconIntegrationHip(small_scene, **KW)
    frame(hip, mv, pr)
    for setup, undo in ((lambda: hip.setColorMaskMode(1), lambda: hip.setColorMaskMode(0)),
                        (lambda: hip.setViewportOrigin(8, 0), lambda: hip.setViewportOrigin(0, 0)),
                        (lambda: hip.setViewportOffset(0.5, 0), lambda: hip.setViewportOffset(0, 0))):
        setup()
        for call in (lambda: hip.drawBBox(mv, pr), lambda: hip.drawTextures(0), lambda: hip.drawTextures(1)):
            with pytest.raises(rr.TsdfError) as e:
                call()
            assert e.value.code == TSDF_ERR_STATE
        undo()
    hip.drawBBox(mv, pr); hip.drawTextures(0); hip.drawTextures(1)
    hip.resize(*VIEW)
    for which in (0, 1):
        with pytest.raises(rr.TsdfError) as e:
            hip.drawTextures(which)
        assert e.value.code == TSDF_ERR_STATE
    L, c = rr.load_library(), hip._c
    m = np.ascontiguousarray(mv, np.float32)
    fp = m.ctypes.data_as(C.POINTER(C.c_float))
    zero = np.zeros(16, np.float32)
    zp = zero.ctypes.data_as(C.POINTER(C.c_float))
    assert L.tsdf_draw_bbox(c, None, fp) == TSDF_ERR_INVALID_ARGUMENT and L.tsdf_draw_bbox(c, fp, None) == TSDF_ERR_INVALID_ARGUMENT
    assert L.tsdf_draw_bbox(c, zp, fp) == TSDF_ERR_INVALID_ARGUMENT and L.tsdf_draw_bbox(c, fp, zp) == TSDF_ERR_INVALID_ARGUMENT
