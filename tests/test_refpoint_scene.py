"""CPU: the scene helper of the reference's operating point (tests/refpoint_scene.py) makes what the GPU tests of
tests/test_gpu_refpoint.py assume -- sizes, formats, a frame with hits, frames whose occupied bricks differ."""
import numpy as np
import pytest

import refpoint_scene as rp
from oracle.oracle import OracleRecon


@pytest.fixture(scope="module")
def frames(rr):
    return rp.make_frames(rr)


def test_analytic_inverse_lut_is_make_scenes_at_a_cubic_size(rr):
    """known answer: at a cubic size the slab-wise evaluation gives make_scene's own inverse LUT, bit for bit, whatever the slab height"""
    sc = rr.scene.make_scene(n_streams=3, width=96, height=72, lut_res=2, inv_res=20)
    for planes in (8, 7):
        lut = rp.analytic_inverse_lut(rr.scene, 3, 96, 72, (20, 20, 20), planes=planes)
        assert lut.dtype == np.float32 and lut.shape == sc["cv_xyz_inv"].shape
        assert np.array_equal(lut, sc["cv_xyz_inv"])
    # ... and per axis: texel (i, j, k) of a 5 x 7 x 3 grid is x fastest and holds the projection of ITS centre
    lut = rp.analytic_inverse_lut(rr.scene, 1, 96, 72, (5, 7, 3)).reshape(3, 7, 5, 4)
    cam = rr.scene.Camera(0, 1, 96, 72, 570.0 * 96 / 640.0)
    ext = rr.scene.BBOX_MAX - rr.scene.BBOX_MIN
    for (i, j, k) in ((0, 0, 0), (4, 6, 2), (2, 5, 1)):
        u, v, d = cam.project(rr.scene.BBOX_MIN + (np.array([i, j, k]) + 0.5) / np.array([5, 7, 3]) * ext)
        want = np.array([u, v, (d - 0.5) / 4.0, 1.0])
        if not (0 <= want[0] <= 1 and 0 <= want[1] <= 1 and 0 <= want[2] <= 1):
            want[:] = -1.0
        assert np.array_equal(lut[k, j, i], want.astype(np.float32))


def test_refpoint_frames_have_the_reference_shape(rr, frames):
    assert rr.inverse_volume_resolution(rr.scene.BBOX_MIN, rr.scene.BBOX_MAX, rp.LUT_VOXEL) == rp.INV_RES == (286, 315, 286)
    assert len(frames) >= 3
    n, (w, h), (cw, ch) = rp.N_STREAMS, rp.DEPTH_WH, rp.COLOR_WH
    n_inv = rp.INV_RES[0] * rp.INV_RES[1] * rp.INV_RES[2]
    for sc in frames:
        assert (sc["n"], sc["width"], sc["height"], sc["color_width"], sc["color_height"]) == (5, 512, 424, 1280, 1080)
        assert tuple(sc["inv_res"]) == rp.INV_RES and tuple(sc["lut_res"]) == (128, 128, 128)
        want = dict(cv_xyz_inv=((n, n_inv, 4), np.float32), cv_xyz=((n, 128 ** 3, 3), np.float32), cv_uv=((n, 128 ** 3, 2), np.float32),
                    depth=((n, h, w, 2), np.float32), quality=((n, h, w), np.float32), silhouette=((n, h, w), np.float32),
                    color=((n, ch, cw, 3), np.uint8))
        for key, (shape, dtype) in want.items():
            assert sc[key].shape == shape and sc[key].dtype == dtype and sc[key].flags["C_CONTIGUOUS"], key
        assert sc["cv_xyz_inv"] is frames[0]["cv_xyz_inv"]                                  # one calibration, shared
    inv = frames[0]["cv_xyz_inv"]
    valid = inv[:, :, 3] == 1.0
    assert np.isin(inv[:, :, 3], (1.0, -1.0)).all() and 0.3 < valid.mean() < 1.0
    assert (inv[valid][:, :3] >= 0).all() and (inv[valid][:, :3] <= 1).all() and (inv[~valid] == -1.0).all()


def test_refpoint_oracle_frames(rr, frames):
    """the oracle at the reference's defaults: 200 x 221 x 200 voxels, 20 x 22 x 20 bricks, a frame with hits from the default view, and
    occupied sets that differ from frame to frame in both directions (bricks fill up AND empty out)"""
    mv, pr = rr.scene.default_view(*rp.KW["view"])
    occupied = []
    for i, sc in enumerate(frames):
        orc = OracleRecon(sc, **rp.KW)
        assert orc.res == rp.RES and orc.res_bricks == rp.RES_BRICKS
        orc.clearOccupiedBricks(); orc.markBricks(); ratio = orc.updateOccupiedBricks()
        occupied.append(set(orc.occupied().tolist()))
        assert 0.01 < ratio < 0.2 and len(occupied[-1]) > 100
        if i < 2:
            orc.integrate()
            t = orc.tsdf()
            surface = np.abs(t) < rp.LIMIT
            assert surface.sum() > 10000
            if i == 1:                                                                      # frame B reaches the partial tile layer on y (221 = 27 * 8 + 5)
                assert surface[:, 216:, :].sum() > 0
        if i == 0:
            orc.drawF(mv, pr)
            assert (orc.framebuffer()[1] < 1).sum() > 20000
    for a, b in zip(occupied, occupied[1:]):
        assert a - b and b - a
