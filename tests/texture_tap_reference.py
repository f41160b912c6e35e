"""numpy restatement of the texture taps' definition (include/rgbd_recon_hip.h, "texture taps"), float32 throughout.

Per point and stream: pc = texture(cv_xyz_inv[i], u).xyz, pcol = texture(cv_uv[i], pc).xy, the NEAREST depth and the LINEAR quality of the frame at
pc.xy, dist = |depth - pc.z|, quality = dist < limit ? quality : 0 -- the per-stream intermediates of blendColors (tsdf_raymarch.fs:295-330) as
tests/mesh_reference.py's colours() forms them, through the oracle's sampling primitives (oracle.tex3d, tex2d_linear, tex2d_nearest).  combine() is the
receiver's rule: the colour fetch at (u, v) and blendColors' two sums in stream order.
"""
import numpy as np

f32 = np.float32
UNIT_CUBE, SENSOR = 1, 2
TEXTURE_TAP_DTYPE = np.dtype([("u", f32), ("v", f32), ("quality", f32), ("dist", f32)])
SENSOR_TAP_DTYPE = np.dtype([("x", f32), ("y", f32), ("z", f32), ("depth", f32)])
TAME = f32(1.0e6)


def to_unit(points, bbox=None, unit_cube=False):
    """the point in the volume's unit cube: u = p, or per axis (p - bbox_min) / e with e = bbox_max - bbox_min -- the difference, then the division"""
    p = np.asarray(points, f32).reshape(-1, 3)
    if unit_cube:
        return p.copy()
    lo = np.asarray(bbox[0], f32)
    e = (np.asarray(bbox[1], f32) - lo).astype(f32)
    with np.errstate(all="ignore"):
        return ((p - lo[None, :]).astype(f32) / e[None, :]).astype(f32)


def evaluated(u):
    """every component finite and |component| < 1.0e6f"""
    with np.errstate(invalid="ignore"):
        return (np.abs(np.asarray(u, f32)) < TAME).all(1)              # (a NaN and an infinity compare false)


def records(scene, limit, points, bbox=None, unit_cube=False):
    """-> (taps TEXTURE_TAP_DTYPE [n][N], sensor SENSOR_TAP_DTYPE [n][N]).  A point that is not evaluated: taps {0, 0, 0, -1}, sensor records zero."""
    from oracle import oracle as orc
    u = to_unit(points, bbox, unit_cube)
    n, N = len(u), scene["n"]
    limit = f32(limit)
    taps, sens = np.zeros((n, N), TEXTURE_TAP_DTYPE), np.zeros((n, N), SENSOR_TAP_DTYPE)
    taps["dist"] = f32(-1.0)
    idx = np.nonzero(evaluated(u))[0]
    if len(idx) == 0:
        return taps, sens
    depth = np.ascontiguousarray(scene["depth"], f32)
    quality = np.ascontiguousarray(np.asarray(scene["quality"], f32)[..., None])
    ri, rl = [int(x) for x in scene["inv_res"]], [int(x) for x in scene["lut_res"]]
    with np.errstate(all="ignore"):
        for i in range(N):
            inv = np.ascontiguousarray(np.asarray(scene["cv_xyz_inv"][i], f32).reshape(ri[2], ri[1], ri[0], 4))
            uv = np.ascontiguousarray(np.asarray(scene["cv_uv"][i], f32).reshape(rl[2], rl[1], rl[0], 2))
            pc = np.stack([orc.tex3d(inv, *p)[:3] for p in u[idx]]).astype(f32)
            pcol = np.stack([orc.tex3d(uv, *p) for p in pc]).astype(f32)
            d = np.array([orc.tex2d_nearest(depth, i, p[0], p[1], 0) for p in pc], f32)
            q = np.array([orc.tex2d_linear(quality, i, p[0], p[1])[0] for p in pc], f32)
            dist = np.abs((d - pc[:, 2]).astype(f32)).astype(f32)
            q = np.where(dist < limit, q, f32(0.0)).astype(f32)
            taps["u"][idx, i], taps["v"][idx, i], taps["quality"][idx, i], taps["dist"][idx, i] = pcol[:, 0], pcol[:, 1], q, dist
            sens["x"][idx, i], sens["y"][idx, i], sens["z"][idx, i], sens["depth"][idx, i] = pc[:, 0], pc[:, 1], pc[:, 2], d
    return taps, sens


def taps(scene, limit, points, bbox=None, unit_cube=False):
    return records(scene, limit, points, bbox, unit_cube)[0]


def sensor(scene, limit, points, bbox=None, unit_cube=False):
    return records(scene, limit, points, bbox, unit_cube)[1]


def combine(scene, taps):
    """the receiver's rule on the scene's colour images: rgba [n][4], alpha +1 (tw > 0) / -1 (fallback); sums left to right in stream order"""
    from oracle import oracle as orc
    taps = np.asarray(taps)
    n, N = taps.shape
    rgb = (np.asarray(scene["color"], np.uint8).astype(f32) / f32(255.0)).astype(f32)
    tc, tc2 = np.zeros((n, 3), f32), np.zeros((n, 3), f32)
    tw, tw2 = np.zeros(n, f32), np.zeros(n, f32)
    with np.errstate(all="ignore"):
        for i in range(N):
            col = np.stack([orc.tex2d_linear(rgb, i, t["u"], t["v"]) for t in taps[:, i]]).astype(f32) if n else np.zeros((0, 3), f32)
            q, dist = taps["quality"][:, i], taps["dist"][:, i]
            de = dist + f32(0.01)
            tc = tc + col * q[:, None] / de[:, None]
            tw = tw + q / de
            tc2 = tc2 + col / dist[:, None]
            tw2 = tw2 + f32(1.0) / dist
        valid = tw > 0
        out = np.zeros((n, 4), f32)
        out[:, :3] = np.where(valid[:, None], tc / tw[:, None], tc2 / tw2[:, None])
        out[:, 3] = np.where(valid, f32(1.0), f32(-1.0))
    return out


def stats(taps):
    """what tsdf_texture_tap_stats reports of a call with these results"""
    taps = np.asarray(taps)
    with np.errstate(invalid="ignore"):
        return dict(points=int(taps.shape[0]), streams=int(taps.shape[1]), with_quality=int((taps["quality"] > 0).sum()),
                    not_evaluated=int((taps["dist"] == f32(-1.0)).sum()))
