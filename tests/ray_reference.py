"""numpy restatement of the ray queries' definition (include/rgbd_recon_hip.h, "ray queries"), float32 throughout.

A ray is mapped into the volume's unit cube, clipped against it with the draw's intersectBox and against the caller's [t_min, t_max], and marched by the
reference's rule: chained `pos += step`, hit test dens > 0, prev starting at -limit, the refinement (p - s) - s * (prev / (dens - prev)).  Every tap goes
through the oracle's sampling primitive (oracle.tex3d's orc_tex3d); the surface at the hits is tests/mesh_reference.py's normals() and colours().  Nothing
here skips space: n_samples is the number of samples the definition takes.
"""
import ctypes as C

import numpy as np

import mesh_reference as M

f32 = np.float32
UNIT_CUBE, NORMALS, COLOURS = 1, 2, 4
HIT, OUTSIDE, INVALID = 1, 2, 4
RAY_DTYPE = np.dtype([("origin", f32, 3), ("t_min", f32), ("dir", f32, 3), ("t_max", f32)])
RAY_HIT_DTYPE = np.dtype([("pos", f32, 3), ("t", f32), ("n_samples", np.uint32), ("status", np.uint32), ("pad", np.uint32, 2)])
RAY_SURFACE_DTYPE = np.dtype([("normal", f32, 3), ("pad", f32), ("rgba", f32, 4)])


class Sampler:
    """texture(volume_tsdf, p).r of a volume [rz][ry][rx]: LINEAR, CLAMP_TO_EDGE, the oracle's orc_tex3d"""

    def __init__(self, vol):
        from oracle import oracle as orc
        self.t = np.ascontiguousarray(np.asarray(vol, f32)[..., None])
        rz, ry, rx, _ = self.t.shape
        self.res = (C.c_uint32 * 3)(rx, ry, rz)
        self.ptr = self.t.ctypes.data_as(C.POINTER(C.c_float))
        self.out = np.zeros(1, f32)
        self.outp = self.out.ctypes.data_as(C.POINTER(C.c_float))
        self.fn = orc.lib().orc_tex3d

    def __call__(self, p):
        self.fn(self.ptr, 1, self.res, C.c_float(p[0]), C.c_float(p[1]), C.c_float(p[2]), self.outp)
        return self.out[0]


def sample_cap(limit):
    """the bound on a ray's sample count: 4.0f / limit + 2.0f"""
    return f32(f32(4.0) / f32(limit) + f32(2.0))


def make_rays(origin, direction, t_min=0.0, t_max=np.inf):
    origin = np.asarray(origin, f32).reshape(-1, 3)
    rays = np.zeros(len(origin), RAY_DTYPE)
    rays["origin"], rays["dir"] = origin, np.asarray(direction, f32).reshape(-1, 3)
    rays["t_min"], rays["t_max"] = t_min, t_max
    return rays


def setup(rays, limit, bbox_min, bbox_max, unit_cube):
    """everything of the definition before the first sample: dict(valid, status, o, d, len2, step, pos, max_n)"""
    rays = np.asarray(rays)
    assert rays.dtype == RAY_DTYPE
    o, d = rays["origin"].astype(f32), rays["dir"].astype(f32)
    t_min, t_max = rays["t_min"].astype(f32), rays["t_max"].astype(f32)
    limit = f32(limit)
    sd = f32(limit * f32(0.5))
    with np.errstate(all="ignore"):
        if not unit_cube:
            lo = np.asarray(bbox_min, f32)
            e = (np.asarray(bbox_max, f32) - lo).astype(f32)
            o = ((o - lo[None, :]) / e[None, :]).astype(f32)
            d = (d / e[None, :]).astype(f32)
        len2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).astype(f32)
        length = np.sqrt(len2).astype(f32)
        valid = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (length > 0) & np.isfinite(length) & ~np.isnan(t_min)
        dn = (d * (f32(1.0) / length)[:, None]).astype(f32)
        step = (dn * sd).astype(f32)
        inv = (f32(1.0) / step).astype(f32)
        tbot = (inv * (f32(0.0) - o)).astype(f32)
        ttop = (inv * (f32(1.0) - o)).astype(f32)
        tmn, tmx = np.fmin(ttop, tbot), np.fmax(ttop, tbot)               # minNum / maxNum: a NaN operand is ignored
        t0 = np.fmax(np.fmax(tmn[:, 0], tmn[:, 1]), np.fmax(tmn[:, 0], tmn[:, 2]))
        t1 = np.fmin(np.fmin(tmx[:, 0], tmx[:, 1]), np.fmin(tmx[:, 0], tmx[:, 2]))
        miss = ~(t0 <= t1) | (t1 < 0)
        t_near = np.where(t0 < 0, f32(0.0), t0).astype(f32)
        per = (length / sd).astype(f32)
        s_min, s_max = (t_min * per).astype(f32), (t_max * per).astype(f32)
        t_near = np.where(s_min > t_near, s_min, t_near).astype(f32)
        t1 = np.where(s_max < t1, s_max, t1).astype(f32)
        miss |= ~(t_near <= t1)
        pos = (o + step * t_near[:, None]).astype(f32)
        marched = valid & ~miss
        count = np.minimum(np.ceil(np.abs(t1 - t_near)), sample_cap(limit))
        max_n = np.where(marched, count, 0).astype(np.uint32)            # (truncation; the count is finite wherever it is used)
    status = np.where(valid, np.where(miss, OUTSIDE, 0), INVALID).astype(np.uint32)
    return dict(valid=valid, status=status, o=o, d=d, len2=len2, step=step, pos=np.where(marched[:, None], pos, f32(0.0)).astype(f32), max_n=max_n)


def cast(vol, limit, bbox_min, bbox_max, rays, unit_cube=False):
    """-> dict(hits RAY_HIT_DTYPE [n], unit [n][3]: the hit's unit-cube position (zeros without a hit))"""
    rays = np.asarray(rays)
    n_rays = len(rays)
    hits = np.zeros(n_rays, RAY_HIT_DTYPE)
    unit = np.zeros((n_rays, 3), f32)
    hits["t"] = f32(-1.0)
    if n_rays == 0:
        return dict(hits=hits, unit=unit)
    S = setup(rays, limit, bbox_min, bbox_max, unit_cube)
    tex = Sampler(vol)
    limit = f32(limit)
    pos, step, max_n = S["pos"].copy(), S["step"], S["max_n"]
    prev = np.full(n_rays, -limit, f32)
    n = np.zeros(n_rays, np.uint32)
    hit = np.zeros(n_rays, bool)
    with np.errstate(all="ignore"):
        while True:
            active = np.nonzero((n < max_n) & ~hit)[0]
            if len(active) == 0:
                break
            dens = np.array([tex(pos[i]) for i in active], f32)
            n[active] += 1
            h = dens > 0                                                 # (a NaN density compares as no hit)
            hi, mi = active[h], active[~h]
            k = (prev[hi] / (dens[h] - prev[hi])).astype(f32)
            unit[hi] = ((pos[hi] - step[hi]) - step[hi] * k[:, None]).astype(f32)
            hit[hi] = True
            prev[mi] = dens[~h]
            pos[mi] = (pos[mi] + step[mi]).astype(f32)
        o, d = S["o"], S["d"]
        t = ((unit[:, 0] - o[:, 0]) * d[:, 0] + (unit[:, 1] - o[:, 1]) * d[:, 1] + (unit[:, 2] - o[:, 2]) * d[:, 2]).astype(f32) / S["len2"]
        if unit_cube:
            world = unit
        else:
            lo = np.asarray(bbox_min, f32)
            e = (np.asarray(bbox_max, f32) - lo).astype(f32)
            world = (lo[None, :] + unit * e[None, :]).astype(f32)
    hits["pos"] = np.where(hit[:, None], world, f32(0.0))
    hits["t"] = np.where(hit, t, f32(-1.0))
    hits["n_samples"] = n
    hits["status"] = S["status"] | np.where(hit, HIT, 0).astype(np.uint32)
    return dict(hits=hits, unit=unit)


def surface(vol, scene, limit, bbox_min, bbox_max, result, normals=True, colours=True):
    """RAY_SURFACE_DTYPE [n] of cast()'s result: mesh_reference's normal and colour at the hits' unit-cube positions, zeros elsewhere"""
    hits, unit = result["hits"], result["unit"]
    out = np.zeros(len(hits), RAY_SURFACE_DTYPE)
    idx = np.nonzero(hits["status"] & HIT)[0]
    if len(idx) == 0:
        return out
    if normals:
        out["normal"][idx] = M.normals(vol, limit, bbox_min, bbox_max, unit[idx])
    if colours:
        out["rgba"][idx] = M.colours(scene, limit, unit[idx])
    return out


def same_bytes(a, b):
    """per record: every field equal bit for bit, a NaN equal to any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    ok = np.ones(a.shape, bool)
    for name in a.dtype.names:
        x, y = a[name].reshape(len(a), -1), b[name].reshape(len(b), -1)
        if x.dtype.kind == "f":
            eq = (x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))
        else:
            eq = x == y
        ok &= eq.all(1)
    return ok
