"""The scene at the operating point of the program this library replaces (a helper for tests, not a conftest).

The reference client's defaults (source/kinect_client.cpp:86-88,206-207,250, source/calib_inverter.cpp:10-18,56-63): bounding box
(-1, 0, -1) .. (1, 2.2, 1), voxels of 0.01 m -> 200 x 221 x 200, bricks of 0.1 m = 10 voxels (never aligned with the 8-voxel storage
tiles), TSDF limit 0.01, 5 streams of 512 x 424 depth with 1280 x 1080 colour, inverse LUTs built at 0.007 m -> 286 x 315 x 286 texels.
An 8^3-voxel tile then touches a box of 12 texels per axis of every stream's LUT, far over what the integrate kernels keep in
LDS: tsdf_integrate runs the generic kernel (every tap from global memory).

`rgbd_recon_amd.scene.make_scene` only makes cubic LUTs; everything but the inverse LUT comes from it unchanged (same random stream
order), the inverse LUT from `analytic_inverse_lut` below: the same camera projection, evaluated in float64 a few z-planes at a time
(5 x 25.8 M texels x 16 B = 2.06 GB as float32; a float64 copy of one stream's grid alone would be 3.3 GB).
"""
import numpy as np

VOXEL, LUT_VOXEL, BRICK, LIMIT = 0.01, 0.007, 0.1, 0.01
N_STREAMS, DEPTH_WH, COLOR_WH, LUT_RES = 5, (512, 424), (1280, 1080), 128
RES, RES_BRICKS, INV_RES = (200, 221, 200), (20, 22, 20), (286, 315, 286)
KW = dict(voxel_size=VOXEL, brick_size=BRICK, limit=LIMIT, view=(1280, 720))         # res=None: the volume follows the voxel size

# the sphere and the box of frames A, B, C (A: make_scene's own places): bricks and tiles empty out from one frame to the next.  B's sphere
# reaches y = 2.18: surface voxels in the partial tile layer ty = 27 (221 = 27 * 8 + 5)
PLACES = [dict(), dict(sphere_c=(0.4, 1.73, -0.3), box_c=(-0.5, 1.5, 0.2)), dict(sphere_c=(-0.45, 1.5, 0.4), box_c=(0.2, 0.3, -0.6))]


def analytic_inverse_lut(scene_mod, n_streams, width, height, inv_res, planes=8):
    """[n][rz * ry * rx][4] float32, x fastest: texel (i, j, k) holds the (u, v, normalised depth, 1) camera `n` of make_scene sees the
    world point of the texel centre at, (-1, -1, -1, -1) outside its frustum -- make_scene's own rule, for any resolution per axis."""
    rx, ry, rz = (int(r) for r in inv_res)
    focal = 570.0 * width / 640.0
    lo, ext = scene_mod.BBOX_MIN, scene_mod.BBOX_MAX - scene_mod.BBOX_MIN
    dmin, dmax = scene_mod.DEPTH_MIN, scene_mod.DEPTH_MAX
    cx, cy, cz = [(np.arange(r) + 0.5) / r for r in (rx, ry, rz)]
    out = np.empty((n_streams, rz, ry, rx, 4), np.float32)
    for k in range(n_streams):
        cam = scene_mod.Camera(k, n_streams, width, height, focal)
        for z0 in range(0, rz, planes):
            wz, wy, wx = np.meshgrid(cz[z0:z0 + planes], cy, cx, indexing="ij")
            world = lo + np.stack([wx, wy, wz], -1) * ext
            u, v, d = cam.project(world)
            dnorm = (d - dmin) / (dmax - dmin)
            ok = (u >= 0) & (u <= 1) & (v >= 0) & (v <= 1) & (dnorm >= 0) & (dnorm <= 1)
            val = np.stack([u, v, dnorm, np.ones_like(u)], -1)
            val[~ok] = -1.0
            out[k, z0:z0 + planes] = val
    return out.reshape(n_streams, -1, 4)


def make_frames(rr, n_frames=3, inv_res=None):
    """-> list of scene dicts (make_scene's format), one per entry of PLACES: the same calibration (the LUT arrays are shared, not
    copied), different depth / colour images.  inv_res None: the reference's 0.007 m grid, from the library's own rule."""
    sm = rr.scene
    if inv_res is None:
        inv_res = rr.inverse_volume_resolution(sm.BBOX_MIN, sm.BBOX_MAX, LUT_VOXEL)
    frames = []
    for i, place in enumerate(PLACES[:n_frames]):
        # (the forward LUTs are made once; the 2^3 inverse LUT of make_scene is replaced below)
        sc = sm.make_scene(n_streams=N_STREAMS, width=DEPTH_WH[0], height=DEPTH_WH[1], lut_res=LUT_RES if i == 0 else 2, inv_res=2,
                           color_width=COLOR_WH[0], color_height=COLOR_WH[1], **place)
        frames.append(sc)
    inv = analytic_inverse_lut(sm, N_STREAMS, DEPTH_WH[0], DEPTH_WH[1], inv_res)
    for sc in frames:
        sc.update(cv_xyz=frames[0]["cv_xyz"], cv_uv=frames[0]["cv_uv"], lut_res=frames[0]["lut_res"],
                  cv_xyz_inv=inv, inv_res=np.array(inv_res, np.uint32))
    return frames


def with_inverse_lut(scene, stream, lut):
    """a copy of the scene dict whose stream `stream` uses `lut` ([rz][ry][rx][4] or flat) as its inverse LUT; the other streams' arrays
    are shared (both the binding and the oracle index cv_xyz_inv per stream, so a list of arrays serves)"""
    luts = [scene["cv_xyz_inv"][i] for i in range(scene["n"])]
    luts[stream] = np.ascontiguousarray(lut, np.float32).reshape(-1, 4)
    assert luts[stream].shape == luts[(stream + 1) % scene["n"]].shape
    return dict(scene, cv_xyz_inv=luts)


def save_frames(frames, path):
    """the arrays of make_frames' result as .npy files under `path`, for a child process (load_frames maps them instead of rebuilding)"""
    import os
    for key in ("cv_xyz", "cv_uv", "cv_xyz_inv"):
        np.save(os.path.join(path, f"{key}.npy"), frames[0][key])
    for i, sc in enumerate(frames):
        for key in ("depth", "quality", "silhouette", "color"):
            np.save(os.path.join(path, f"{key}_{i}.npy"), sc[key])


def load_frames(rr, path, n_frames=3):
    import os
    sm = rr.scene
    luts = {key: np.load(os.path.join(path, f"{key}.npy"), mmap_mode="r") for key in ("cv_xyz", "cv_uv", "cv_xyz_inv")}
    frames = []
    for i in range(n_frames):
        sc = dict(n=N_STREAMS, width=DEPTH_WH[0], height=DEPTH_WH[1], color_width=COLOR_WH[0], color_height=COLOR_WH[1],
                  bbox_min=sm.BBOX_MIN.astype(np.float32), bbox_max=sm.BBOX_MAX.astype(np.float32),
                  depth_limits=np.array([sm.DEPTH_MIN, sm.DEPTH_MAX], np.float32),
                  lut_res=np.array([LUT_RES] * 3, np.uint32), inv_res=np.array(INV_RES, np.uint32), **luts)
        for key in ("depth", "quality", "silhouette", "color"):
            sc[key] = np.load(os.path.join(path, f"{key}_{i}.npy"))
        frames.append(sc)
    return frames


def scene_with_lut(rr, inv_res, **make_scene_kw):
    """make_scene(**make_scene_kw) with an inverse LUT of any size per axis (the ladder of LUT : volume ratios in test_gpu_refpoint.py)"""
    sc = rr.scene.make_scene(inv_res=2, **make_scene_kw)
    sc.update(cv_xyz_inv=analytic_inverse_lut(rr.scene, sc["n"], sc["width"], sc["height"], inv_res), inv_res=np.array(inv_res, np.uint32))
    return sc
