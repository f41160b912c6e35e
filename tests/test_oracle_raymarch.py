"""K2 on an analytic sphere SDF (CPU only): hit position within half a step, gradient normal, depth formula,
sample counts, and the space-skipping interval (tsdf_raymarch.fs:62-134,363-398; bricks.* depth limits)."""
import numpy as np

import rgbd_recon_amd as rr
from helpers import tiny_scene
from oracle.oracle import OracleRecon

f32 = np.float32
LIMIT = 0.05
RES = 48
VIEW = (48, 32)


def sphere_recon(skip):
    sc = tiny_scene([(0.5, 0.5, 0.5)], [0.5], [1.0], [1.0])
    sc["color"][:] = (255, 128, 0)
    o = OracleRecon(sc, res=(RES,) * 3, brick_size=[0.125] * 3, limit=LIMIT, view=VIEW)
    c = (np.arange(RES) + 0.5) / RES
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    r = np.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2)
    o.set_tsdf(np.clip(0.3 - r, -LIMIT, LIMIT))                        # negative outside, positive inside
    cnt = np.zeros(o.numBricks(), np.uint32)
    bc = (np.arange(8) + 0.5) / 8
    bz, by, bx = np.meshgrid(bc, bc, bc, indexing="ij")
    br = np.sqrt((bx - 0.5) ** 2 + (by - 0.5) ** 2 + (bz - 0.5) ** 2)
    cnt[(np.abs(br - 0.3) < 0.12).ravel()] = 50                        # shell of occupied bricks around the surface
    o.set_counters(cnt)
    o.updateOccupiedBricks()
    o.setSpaceSkip(skip)
    o.setColorFilling(False)
    return o


def view():
    mv = rr.scene.look_at((0.5, 0.5, 2.5), (0.5, 0.5, 0.5))
    pr = rr.scene.perspective(40.0, VIEW[0] / VIEW[1], 0.1, 50.0)
    return mv, pr, rr.scene.gl_flat(mv), rr.scene.gl_flat(pr)


def test_sphere_hit_depth_and_mask():
    for skip in (False, True):
        o = sphere_recon(skip)
        mv, pr, mvf, prf = view()
        o.draw(mvf, prf)
        rgba, depth, ns, peels = o.view_images()
        hit = depth < 1
        cx, cy = VIEW[0] // 2, VIEW[1] // 2
        assert hit[cy, cx] and not hit[0, 0] and 120 < hit.sum() < 160   # pi * (43.96 px * tan(asin(.15)))^2 = 140
        # central ray hits the sphere at eye distance 2.0 - 0.3 = 1.7; gl_FragDepth of that z (tsdf_raymarch.fs:133)
        ze = -1.7
        want = (pr[2, 2] * ze + pr[2, 3]) / -ze * 0.5 + 0.5
        step_world = LIMIT * 0.5
        tol = abs((pr[2, 2] * (ze + step_world) + pr[2, 3]) / -(ze + step_world) * 0.5 + 0.5 - want)
        assert abs(depth[cy, cx] - want) < tol                         # within half a step of the true crossing
        assert np.allclose(rgba[cy, cx, :3], [1.0, 128 / 255, 0.0], atol=1e-6) and rgba[cy, cx, 3] == 1.0
        if skip:
            assert (peels[..., 0][hit] < 1).all() and (ns[~hit & (peels[..., 0] >= 1)] == 0).all()


def test_skip_space_takes_fewer_samples_and_same_surface():
    a, b = sphere_recon(False), sphere_recon(True)
    _, _, mvf, prf = view()
    a.draw(mvf, prf); b.draw(mvf, prf)
    (_, da, na, _), (_, db, nb, _) = a.view_images(), b.view_images()
    both = (da < 1) & (db < 1)
    assert both.sum() > 120 and ((da < 1) != (db < 1)).mean() < 0.02
    assert np.abs(da[both] - db[both]).max() < 2e-3                    # same surface, different sampling phase
    assert nb[both].mean() < na[both].mean()


def test_normal_shading_mode_points_at_camera_on_axis():
    o = sphere_recon(False)
    o.setShadeMode(2)                                                   # shading.glsl:64-66
    _, _, mvf, prf = view()
    o.draw(mvf, prf)
    rgba, depth, _, _ = o.view_images()
    n = rgba[VIEW[1] // 2, VIEW[0] // 2, :3]
    assert n[2] > 0.99 and abs(n[0]) < 0.1 and abs(n[1]) < 0.1


def test_view_matrices_match_their_definitions():
    o = sphere_recon(False)
    mv, pr, mvf, prf = view()
    img_to_eye, normal, cam = o.view_matrices(mvf, prf)
    S = np.diag([VIEW[0] * 0.5, VIEW[1] * 0.5, 0.5, 1.0]); T = np.eye(4); T[:3, 3] = 1
    np.testing.assert_allclose(img_to_eye.reshape(4, 4).T, np.linalg.inv(S @ T @ pr), rtol=2e-6, atol=1e-6)
    np.testing.assert_allclose(cam, [0.5, 0.5, 2.5], atol=1e-6)        # unit bbox: volume space == world
    np.testing.assert_allclose(normal.reshape(4, 4).T, np.linalg.inv(mv).T, rtol=2e-6, atol=1e-6)


def test_skip_space_takes_no_sample_beside_the_volume():
    """The fragments of the march are those of the unit cube (UnitCube::draw, recon_integration.cpp:223-225).  A brick size that does not
    divide the bounding box leaves a last column of bricks that reaches past it (to_world of bricks.vs draws every brick whole), so the
    depth limits cover pixels beside the cube: no fragment there, no sample, whatever the depth limits say."""
    import main_path_reference as R
    sc = tiny_scene([(0.5, 0.5, 0.5)], [0.5], [1.0], [1.0])
    view = (192, 128)                                                   # the overhang is 1 / 48 of the box: a good two pixels wide here
    o = OracleRecon(sc, res=(RES,) * 3, brick_size=[0.145] * 3, limit=LIMIT, view=view)      # snaps to 7 voxels: 7 bricks span 49 / 48 of the box
    assert o.res_bricks == (7, 7, 7) and o.brick_size[0] * 7 > 1.0
    o.set_tsdf(np.full((RES,) * 3, 0.01, np.float32))                   # positive everywhere: any sample is a hit
    cnt = np.zeros(o.numBricks(), np.uint32)
    cnt[6::7] = 50                                                     # the whole last column in x
    o.set_counters(cnt)
    o.updateOccupiedBricks()
    o.setSpaceSkip(True)
    o.setColorFilling(False)
    mvf = rr.scene.gl_flat(rr.scene.look_at((0.5, 0.5, 2.5), (0.5, 0.5, 0.5)))
    prf = rr.scene.gl_flat(rr.scene.perspective(40.0, view[0] / view[1], 0.1, 50.0))
    o.draw(mvf, prf)
    _, depth, ns, peels = o.view_images()
    V = R.View(mvf, prf, view, (0, 0, 0), (1, 1, 1))
    covered, _, _, margin = R.box_interval(V, V.ray_directions() * (LIMIT * 0.5))
    beside = (peels[..., 0] < 1) & ~covered & (margin > 1e-3)          # under the overhanging bricks, clearly off the cube
    under = (peels[..., 0] < -peels[..., 1]) & covered & (margin > 1e-3)     # a non-empty interval between the nearest and the farthest face
    assert beside.sum() >= 10 and under.sum() >= 10
    assert (ns[beside] == 0).all() and (depth[beside] == 1).all()
    assert (ns[under] > 0).all() and (depth[under] < 1).all()
