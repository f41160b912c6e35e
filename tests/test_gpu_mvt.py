"""-m gpu: the MVT back-end (tsdf_draw_mvt, kinect::ReconMVT::draw) against the CPU reference tests/mvt_reference.py.  The vertex stage's
filtered depth is bit-exact, its lateral quality within 1e-5 relative (powf); the framebuffer's coverage and depth are bit-exact, its colours
sums of fp32 atomics in arrival order (2e-5, 5e-5 with the Phong pow of shade mode 1), as in test_gpu_trigrid.py."""
import numpy as np
import pytest

import mvt_reference as M
from oracle.oracle import OracleRecon

pytestmark = pytest.mark.gpu

TSDF_ERR_STATE = -4
KW = dict(res=(64, 64, 64), brick_size=[2.0 / 8, 2.2 / 8, 2.0 / 8], limit=0.04, view=(320, 180))
_cache = {}


def scene_of(rr, w, h, n=3, cw=None, ch=None, **kw):
    key = (w, h, n, cw, ch, tuple(sorted((k, tuple(v)) for k, v in kw.items())))
    if key not in _cache:
        _cache[key] = rr.scene.make_scene(n_streams=n, width=w, height=h, lut_res=32, inv_res=16, color_width=cw, color_height=ch, **kw)
    return _cache[key]


def ref_vertices(sc):
    k = ("vtx", id(sc))
    if k not in _cache:
        _cache[k] = M.vertex_stage(sc["depth_raw"])
    return _cache[k]


def views(rr, w, h):
    pr = rr.scene.gl_flat(rr.scene.perspective(50.0, w / float(h), 0.1, 200.0))
    return [(rr.scene.gl_flat(rr.scene.look_at(e, (0.0, 1.1, 0.0))), pr) for e in [(0.0, 1.1, 3.0), (1.6, 1.4, 2.4)]]


def ref_frame(sc, mv, pr, mode=0, min_length=0.0125, view=KW["view"]):
    i2e = OracleRecon(sc, **dict(KW, view=view)).view_matrices(mv, pr)[0]       # draw()'s image_to_eye, as the library forms it
    return M.draw_mvt(sc, ref_vertices(sc), mv, pr, view, i2e, min_length=min_length, shade_mode=mode)


def hip_of(rr, sc, **kw):
    h = rr.ReconIntegrationHip(sc, **dict(KW, **kw))
    h.upload_raw_frame(sc)
    return h


def check_vertices(got, want):
    np.testing.assert_array_equal(got[..., 0], want[..., 0])
    np.testing.assert_allclose(got[..., 1], want[..., 1], rtol=1e-5, atol=0)
    assert (want[..., 0] > 0).sum() > 500 and (want[..., 1] > 0).sum() > 500


def check_frame(got, want, tol=2e-5, min_cov=2000):
    (fc, fd), (gc, gd) = got, want
    np.testing.assert_array_equal(fd, gd)                                  # coverage + depth: exact
    assert np.abs(fc - gc).max() <= tol
    assert (gd < 1).sum() >= min_cov and (gc[gd < 1][:, 3] == 1.0).all()


@pytest.mark.parametrize("w, h, cw, ch", [(160, 120, None, None), (320, 240, None, None), (96, 128, None, None), (160, 120, 200, 150)])
def test_vertex_stage_matches_reference(rr, w, h, cw, ch):
    """W > H (two sizes), W < H (vertex columns past the image), colour resolution != depth resolution"""
    sc = scene_of(rr, w, h, cw=cw, ch=ch)
    hip = hip_of(rr, sc)
    hip.drawMVT(*views(rr, *KW["view"])[0])
    got = hip.mvt_vertices()
    assert got.shape == (3, w + 1, h + 1, 2)
    check_vertices(got, ref_vertices(sc))


@pytest.mark.parametrize("mode, tol", [(0, 2e-5), (1, 5e-5), (3, 2e-5)])
def test_framebuffer_matches_reference(rr, mode, tol):
    sc = scene_of(rr, 320, 240)
    hip = hip_of(rr, sc)
    hip.setShadeMode(mode)
    for mv, pr in views(rr, *KW["view"]):
        hip.drawMVT(mv, pr)
        check_frame(hip.framebuffer(), ref_frame(sc, mv, pr, mode), tol)


def test_min_length_controls_the_mesh(rr):
    sc = scene_of(rr, 320, 240)
    hip = hip_of(rr, sc)
    hip.setShadeMode(3)
    mv, pr = views(rr, *KW["view"])[0]
    counts = []
    for ml in (0.0125, 0.001):                                             # 0.001 m * 2.5 m + 0.005 m: below the cells' 12 mm diagonals
        hip.setMinLength(ml)
        hip.drawMVT(mv, pr)
        want = ref_frame(sc, mv, pr, 3, min_length=ml)
        check_frame(hip.framebuffer(), want, min_cov=0)
        counts.append((want[1] < 1).sum())
    assert counts[0] > 2000 and counts[1] < counts[0] * 0.7


def test_input_paths_agree(rr):
    """raw upload with and without processTextures, the device-array upload, other setPreprocess flags: the same draw"""
    import torch
    sc = scene_of(rr, 160, 120)
    mv, pr = views(rr, 160, 90)[1]
    kw = dict(view=(160, 90))
    want_v = ref_vertices(sc)
    want_f = ref_frame(sc, mv, pr, 0, view=(160, 90))
    dev = (torch.from_numpy(np.ascontiguousarray(sc["depth_raw"], np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(sc["color"], np.uint8)).cuda())
    torch.cuda.synchronize()
    for path in ("raw", "raw+process", "dev", "dev+process", "flags"):
        hip = rr.ReconIntegrationHip(sc, **dict(KW, **kw))
        if path.startswith("dev"):
            hip.set_preprocess_calibration(sc)
            hip.upload_raw_frame_dev(dev[0].data_ptr(), dev[1].data_ptr(), complete=True)
        else:
            hip.upload_raw_frame(sc)
        if path == "flags":
            hip.setPreprocess(False, False, False)
        if path.endswith("process") or path == "flags":
            hip.processTextures()
        hip.drawMVT(mv, pr)
        check_vertices(hip.mvt_vertices(), want_v)
        check_frame(hip.framebuffer(), want_f, min_cov=200)
        hip.close()


def test_no_raw_frame_is_a_state_error(rr):
    sc = scene_of(rr, 160, 120)
    hip = rr.ReconIntegrationHip(sc, **dict(KW, view=(160, 90)))           # a pre-processed frame only
    with pytest.raises(rr.TsdfError) as e:
        hip.drawMVT(*views(rr, 160, 90)[0])
    assert e.value.code == TSDF_ERR_STATE
    with pytest.raises(rr.TsdfError) as e:
        hip.mvt_vertices()
    assert e.value.code == TSDF_ERR_STATE


def test_next_raw_upload_waits_for_the_draw(rr):
    """stage overlap on: draw frame A, upload frame B on the lane ahead (it rewrites the raw depth buffer A's draw reads), then read A,
    draw B: each result is its own frame's"""
    a, b = scene_of(rr, 320, 240), scene_of(rr, 320, 240, sphere_c=(0.25, 1.0, 0.2))
    assert not np.array_equal(a["depth_raw"], b["depth_raw"])
    mv, pr = views(rr, *KW["view"])[0]
    hip = hip_of(rr, a)
    hip.set_stage_overlap(True)
    hip.setShadeMode(3)
    hip.drawMVT(mv, pr)
    hip.upload_raw_frame(b)
    check_frame(hip.framebuffer(), ref_frame(a, mv, pr, 3))
    check_vertices(hip.mvt_vertices(), ref_vertices(a))
    hip.drawMVT(mv, pr)
    check_frame(hip.framebuffer(), ref_frame(b, mv, pr, 3))
    check_vertices(hip.mvt_vertices(), ref_vertices(b))


def test_tsdf_path_is_untouched_by_an_mvt_draw(rr):
    sc = rr.scene.make_scene(n_streams=2, width=160, height=120, lut_res=32, inv_res=32)
    kw = dict(res=(64, 64, 64), brick_size=[2.0 / 8, 2.2 / 8, 2.0 / 8], limit=0.04, view=(160, 90))
    hip, orc = rr.ReconIntegrationHip(sc, **kw), OracleRecon(sc, **kw)
    mv, pr = rr.scene.default_view(160, 90)
    hip.upload_raw_frame(sc)
    hip.drawMVT(mv, pr)
    hip.upload_frame(sc)
    for o in (hip, orc):
        o.clearOccupiedBricks(); o.markBricks(); o.updateOccupiedBricks(); o.integrate(); o.drawF(mv, pr)

    def same(x, y):
        return (x == y) | (np.isnan(x) & np.isnan(y))
    assert same(hip.tsdf(), orc.tsdf()).all()
    (fc, fd), (gc, gd) = hip.framebuffer(), orc.framebuffer()
    assert (fd < 1).sum() > 100 and same(fd, gd).all() and same(fc, gc).all()
