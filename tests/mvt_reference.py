"""CPU reference of the MVT back-end, kinect::ReconMVT::draw() (framework/reconstruction/recon_mvt.cpp:84-150 with
glsl/mvt_accum.{vs,gs,fs} and trigrid_normalize.fs).  numpy, fp32 throughout (every operation restated in the shaders' order;
nothing is promoted to float64 except where the reference host code itself computes in double).

* vertex_stage(raw): mvt_accum.vs:43-115, the 13 x 13 bilateral filter of the raw depth at every grid vertex, with the LITERAL
  fp32 texture coordinates of the taps and GL NEAREST + CLAMP_TO_EDGE lookups.
* draw_mvt(...): the z pre-pass, the ONE/ONE blend and the normalise pass, restating the oracle's Trigrid rasteriser
  (oracle/tsdf_oracle.cpp, orc_draw_trigrid and its helpers) with MVT's validSurface (mvt_accum.gs:29-41) and fragment quality
  (mvt_accum.fs:53).  LUT and colour lookups go through the oracle's sampling primitives (oracle.tex3d / tex2d_linear).
  A triangle that reaches behind the eye is dropped whole here; the oracle and the kernels cut it at the near plane (tri_clip_near).
  The check that shares nothing with the oracle is tests/backend_reference.draw_mvt_raster, through tests/test_gpu_backends.py.
"""
import numpy as np

from oracle.oracle import tex2d_linear, tex3d

F = np.float32
KERNEL = 6                      # kernel_size, mvt_accum.vs:22
CV_MIN_D, CV_MAX_D = F(0.5), F(4.5)   # recon_mvt.cpp:35-36 (constants, not the sensors' limits)
CAMERA_COLORS = np.array([[228, 26, 28], [55, 126, 184], [77, 175, 74], [152, 78, 163], [255, 127, 0], [255, 255, 51], [166, 86, 40],
                          [247, 129, 191]], np.float32) / F(255.0)   # shading.glsl:24-30, extended past 5 streams


def grid_coord(g, n):
    """recon_mvt.cpp:51-56: (x + 0.5) * stepX with a float stepX = 1.0f / n, evaluated in double, stored as float"""
    step = F(1.0) / F(n)
    return ((np.asarray(g, np.float64) + 0.5) * np.float64(step)).astype(np.float32)


def nearest(u, n):
    """GL NEAREST + CLAMP_TO_EDGE texel index of fp32 coordinate u in a texture of n texels"""
    return np.clip(np.floor(np.asarray(u, np.float32) * F(n)), 0, n - 1).astype(np.int64)


def tap_coord(u, k, n):
    """mvt_accum.vs:70: coords.s + float(x) * tex_size_inv.x, tex_size_inv = 1.0f / size (recon_mvt.cpp:42), fp32"""
    return (np.asarray(u, np.float32) + F(k) * (F(1.0) / F(n))).astype(np.float32)


def vertex_stage(raw):
    """raw [N][H][W] fp32 metres -> [N][W+1][H+1][2] (filtered depth, lateral quality) of grid vertex (gx, gy) at [l][gy][gx];
    gx in [0, H], gy in [0, W] (recon_mvt.cpp:53-54's swapped loop bounds)."""
    raw = np.ascontiguousarray(raw, np.float32)
    N, H, W = raw.shape
    u, v = grid_coord(np.arange(H + 1), W), grid_coord(np.arange(W + 1), H)
    out = np.zeros((N, W + 1, H + 1, 2), np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for l in range(N):
            img = raw[l]
            depth = img[nearest(v, H)[:, None], nearest(u, W)[None, :]]                  # :50
            outside = (depth < CV_MIN_D) | (depth > CV_MAX_D)                            # is_outside, :43-45 / :51
            d_dmax = depth / F(4.5)                                                      # :56-57
            drm = F(0.35) * d_dmax
            drm_inv = F(1.0) / drm
            depth_bf, w, w_range, border, num = (np.zeros_like(depth) for _ in range(5))
            for y in range(-KERNEL, KERNEL + 1):                                         # :66
                rows = nearest(tap_coord(v, y, H), H)
                for x in range(-KERNEL, KERNEL + 1):                                     # :67
                    num += F(1.0)
                    ds = img[rows[:, None], nearest(tap_coord(u, x, W), W)[None, :]]
                    dr = np.abs(ds - depth)
                    rej = (ds < CV_MIN_D) | (ds > CV_MAX_D) | (dr > drm)                 # :74-77
                    border = np.where(rej, border + F(1.0), border)
                    gs = F(1.0) - np.sqrt(F(x * x + y * y)) * (F(1.0) / F(KERNEL))        # computeGaussSpace(length(vec2(x, y)))
                    gr = F(1.0) - np.minimum(dr, drm) * drm_inv                          # computeGaussRange
                    ws = gs * gr
                    depth_bf = np.where(rej, depth_bf, depth_bf + ws * ds)
                    w = np.where(rej, w, w + ws)
                    w_range = np.where(rej, w_range, w_range + gr)
            lq = F(1.0) - border / num                                                   # :88
            fd = np.where(w > F(0.0), depth_bf / w, F(0.0))                              # :89-93
            fd = np.where(w_range < num * F(0.65), F(0.0), fd)                           # :95-99
            out[l, ..., 0] = np.where(outside, F(0.0), fd)
            out[l, ..., 1] = np.where(outside, F(0.0), np.power(lq, F(30.0)))
    assert out.dtype == np.float32
    return out


def _mul(m, x, y, z, w):
    """column-major mat4 (float32[16]) times (x, y, z, w), fp32, the shaders' / kernels' sum order"""
    return [m[r] * x + m[4 + r] * y + m[8 + r] * z + m[12 + r] * w for r in range(4)]


def _len3(x, y, z):
    return np.sqrt(x * x + y * y + z * z)


def _normalize(x, y, z):
    s = F(1.0) / np.sqrt(x * x + y * y + z * z)
    return x * s, y * s, z * s


def pmv(mv, pr):
    """P * MV formed in double, rounded once (the draw calls' host product)"""
    a, b = np.asarray(pr, np.float64).reshape(16), np.asarray(mv, np.float64).reshape(16)
    out = np.zeros(16, np.float64)
    for c in range(4):
        for r in range(4):
            s = 0.0
            for k in range(4):
                s += a[k * 4 + r] * b[c * 4 + k]
            out[c * 4 + r] = s
    return out.astype(np.float32)


def _shade(mode, px, py, pz, nx, ny, nz, cr, cg, cb):
    """shading.glsl:32-69 for shade modes 0 and 1"""
    if mode == 0:
        return cr, cg, cb
    assert mode == 1
    lp, ld = (F(1.5), F(1.0), F(1.0)), (F(1.0), F(0.9), F(0.7))
    la_ = tuple(d * F(0.2) for d in ld)
    tx, ty, tz = _normalize(lp[0] - px, lp[1] - py, lp[2] - pz)
    la = nx * tx + ny * ty + nz * tz
    lit = ~(la <= F(0.0))
    diff = np.where(lit, np.maximum(la, F(0.0)), F(0.0))
    vx, vy, vz = _normalize(-px, -py, -pz)
    hx, hy, hz = _normalize(tx + vx, ty + vy, tz + vz)
    with np.errstate(invalid="ignore"):
        spec = np.power(hx * nx + hy * ny + hz * nz, F(20.0))
    a = (F(1.0) - la) * (F(1.0) - la)
    spec = np.where(lit, spec * (F(1.0) - a * a * a), F(0.0))
    return tuple(la_[i] * F(0.5) + ld[i] * F(0.5) * diff + F(1.0) * F(0.5) * spec for i in range(3))


def _volume(scene, key, l):
    """calibration volume `key` of sensor l as [rz][ry][rx][channels] (scenes store it flat, [texels][channels], with lut_res = (rx, ry, rz))"""
    t = np.asarray(scene[key][l], np.float32)
    if t.ndim == 2:
        rx, ry, rz = (int(r) for r in scene["lut_res"])
        t = t.reshape(rz, ry, rx, t.shape[-1])
    return np.ascontiguousarray(t)


def draw_mvt(scene, vtx, mv, pr, view, img_to_eye, min_length=0.0125, shade_mode=0):
    """The MVT draw of the vertex stage `vtx` (vertex_stage()) -> (colour [vh][vw][4], depth [vh][vw]), the framebuffer of
    trigrid_normalize.fs.  img_to_eye: draw()'s image-to-eye matrix (float32[16], column major)."""
    N, Wp, Hp, _ = vtx.shape
    W, H = Wp - 1, Hp - 1
    vw, vh = view
    mv = np.asarray(mv, np.float32).reshape(16)
    PMV, I2E = pmv(mv, pr), np.asarray(img_to_eye, np.float32).reshape(16)
    bmin, bmax = np.asarray(scene["bbox_min"], np.float32), np.asarray(scene["bbox_max"], np.float32)
    u, v = grid_coord(np.arange(H + 1), W), grid_coord(np.arange(W + 1), H)
    # ---- per grid vertex: the rest of mvt_accum.vs main() (:104-115)
    depth, lq = vtx[..., 0], vtx[..., 1]
    pos = np.full((N, W + 1, H + 1, 5), np.nan, np.float32)     # pos_cs xyz, texcoord st
    for l in range(N):
        xyz, uvt = (_volume(scene, key, l) for key in ("cv_xyz", "cv_uv"))
        for gy, gx in zip(*np.nonzero(depth[l] >= CV_MIN_D)):  # (a vertex below 0.5 m is in no valid triangle: its lookups are never read)
            d_idx = (depth[l, gy, gx] - CV_MIN_D) / (CV_MAX_D - CV_MIN_D)
            pos[l, gy, gx, :3] = tex3d(xyz, u[gx], v[gy], d_idx)
            pos[l, gy, gx, 3:] = tex3d(uvt, u[gx], v[gy], d_idx)
    X, Y, Z = pos[..., 0], pos[..., 1], pos[..., 2]
    es = _mul(mv, X, Y, Z, F(1.0))[:3]
    cx, cy, cz, cw = _mul(PMV, X, Y, Z, F(1.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        front, iw = cw > F(0.0), F(1.0) / cw
        xw = (cx / cw * F(0.5) + F(0.5)) * F(vw)
        yw = (cy / cw * F(0.5) + F(0.5)) * F(vh)
        zw = cz / cw * F(0.5) + F(0.5)
    V = dict(pcs=(X, Y, Z), pes=tuple(es), tc=(pos[..., 3], pos[..., 4]), depth=depth, lq=lq, front=front, iw=iw, xw=xw, yw=yw, zw=zw)
    # ---- triangles (recon_mvt.cpp:53-62): cells x < H, y < W; (x, y) (x+1, y) (x, y+1) and (x+1, y) (x+1, y+1) (x, y+1)
    l_, y_, x_ = np.meshgrid(np.arange(N), np.arange(W), np.arange(H), indexing="ij")
    l_, y_, x_ = l_.ravel(), y_.ravel(), x_.ravel()
    corners = [((x_, y_), (x_ + 1, y_), (x_, y_ + 1)), ((x_ + 1, y_), (x_ + 1, y_ + 1), (x_, y_ + 1))]
    tri = {k: [] for k in ("l", "a", "b", "d")}
    for (a, b, d) in corners:
        tri["l"].append(l_)
        for key, (gx, gy) in zip("abd", (a, b, d)):
            tri[key].append((l_, gy, gx))
    L = np.concatenate(tri["l"])
    idx = {k: tuple(np.concatenate([t[i] for t in tri[k]]) for i in range(3)) for k in "abd"}
    g = {k: {name: (tuple(c[idx[k]] for c in val) if isinstance(val, tuple) else val[idx[k]]) for name, val in V.items()} for k in "abd"}
    a, b, d = g["a"], g["b"], g["d"]
    # ---- validSurface (mvt_accum.gs:29-41) + set-up
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = ~((a["depth"] < CV_MIN_D) | (b["depth"] < CV_MIN_D) | (d["depth"] < CV_MIN_D))
        avg = (a["depth"] + b["depth"] + d["depth"]) / F(3.0)
        lim = F(min_length) * avg + F(0.005)
        e = lambda p, q: _len3(*(q["pcs"][i] - p["pcs"][i] for i in range(3)))
        ok &= (e(a, b) < lim) & (e(a, d) < lim) & (e(b, d) < lim)
        ok &= a["front"] & b["front"] & d["front"]
        ea = [b["pes"][i] - a["pes"][i] for i in range(3)]
        eb = [d["pes"][i] - a["pes"][i] for i in range(3)]
        normal = _normalize(ea[1] * eb[2] - eb[1] * ea[2], ea[2] * eb[0] - eb[2] * ea[0], ea[0] * eb[1] - eb[0] * ea[1])
        area = (b["xw"] - a["xw"]) * (d["yw"] - a["yw"]) - (d["xw"] - a["xw"]) * (b["yw"] - a["yw"])
        ok &= area != F(0.0)
        minx = np.fmin(np.fmin(a["xw"], b["xw"]), d["xw"]); maxx = np.fmax(np.fmax(a["xw"], b["xw"]), d["xw"])
        miny = np.fmin(np.fmin(a["yw"], b["yw"]), d["yw"]); maxy = np.fmax(np.fmax(a["yw"], b["yw"]), d["yw"])
        ok &= (maxx >= F(0)) & (maxy >= F(0)) & (minx <= F(vw)) & (miny <= F(vh))
    t = np.nonzero(ok)[0]
    x0 = np.maximum(np.floor(minx[t] - F(0.5)), F(0)).astype(np.int64); x1 = np.minimum(np.ceil(maxx[t] - F(0.5)), F(vw - 1)).astype(np.int64)
    y0 = np.maximum(np.floor(miny[t] - F(0.5)), F(0)).astype(np.int64); y1 = np.minimum(np.ceil(maxy[t] - F(0.5)), F(vh - 1)).astype(np.int64)
    nx, ny = np.maximum(x1 - x0 + 1, 0), np.maximum(y1 - y0 + 1, 0)
    cnt = nx * ny
    T = np.repeat(t, cnt)
    k = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    rnx = np.repeat(nx, cnt)
    PX, PY = np.repeat(x0, cnt) + k % np.maximum(rnx, 1), np.repeat(y0, cnt) + k // np.maximum(rnx, 1)
    A, B, D = ({n: (tuple(c[T] for c in val) if isinstance(val, tuple) else val[T]) for n, val in q.items()} for q in (a, b, d))
    ar = area[T]
    # ---- coverage + interpolation (tri_fragment)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        x, y = PX.astype(np.float32) + F(0.5), PY.astype(np.float32) + F(0.5)
        e0 = (D["xw"] - B["xw"]) * (y - B["yw"]) - (D["yw"] - B["yw"]) * (x - B["xw"])
        e1 = (A["xw"] - D["xw"]) * (y - D["yw"]) - (A["yw"] - D["yw"]) * (x - D["xw"])
        e2 = (B["xw"] - A["xw"]) * (y - A["yw"]) - (B["yw"] - A["yw"]) * (x - A["xw"])
        sgn = np.where(ar > F(0), F(1), F(-1))
        exs = [(D["xw"] - B["xw"]) * sgn, (A["xw"] - D["xw"]) * sgn, (B["xw"] - A["xw"]) * sgn]
        eys = [(D["yw"] - B["yw"]) * sgn, (A["yw"] - D["yw"]) * sgn, (B["yw"] - A["yw"]) * sgn]
        cov = np.ones(T.shape, bool)
        for ee, ex, ey in zip((e0 * sgn, e1 * sgn, e2 * sgn), exs, eys):
            cov &= ~(ee < F(0))
            cov &= ~((ee == F(0)) & ~((ey > F(0)) | ((ey == F(0)) & (ex < F(0)))))
            cov &= ee >= F(0)
        l0, l1, l2 = e0 / ar, e1 / ar, e2 / ar
        z = l0 * A["zw"] + l1 * B["zw"] + l2 * D["zw"]
        cov &= (z >= F(0)) & (z <= F(1))
        w0, w1, w2 = l0 * A["iw"], l1 * B["iw"], l2 * D["iw"]
        iw = w0 + w1 + w2
        ip = lambda p, q, r: (w0 * p + w1 * q + w2 * r) / iw
        tcx, tcy = ip(A["tc"][0], B["tc"][0], D["tc"][0]), ip(A["tc"][1], B["tc"][1], D["tc"][1])
        fq, fd = ip(A["lq"], B["lq"], D["lq"]), ip(A["depth"], B["depth"], D["depth"])
        fes = [ip(A["pes"][i], B["pes"][i], D["pes"][i]) for i in range(3)]
        fcs = [ip(A["pcs"][i], B["pcs"][i], D["pcs"][i]) for i in range(3)]
        # ---- tests of every stage (mvt_accum.fs:35-50)
        cov &= (fcs[0] >= bmin[0]) & (fcs[1] >= bmin[1]) & (fcs[2] >= bmin[2]) & (fcs[0] <= bmax[0]) & (fcs[1] <= bmax[1]) & (fcs[2] <= bmax[2])
        cov &= ~((tcx > F(0.99)) | (tcx < F(0.01)) | (tcy > F(0.99)) | (tcy < F(0.01)))
        nn = _normalize(*(c[T] for c in normal))
        n = tuple(-c for c in nn)
        pe = _normalize(*fes)
        cov &= ~(n[0] * pe[0] + n[1] * pe[1] + n[2] * pe[2] > F(0))
    s = np.nonzero(cov)[0]
    pix = PY[s] * vw + PX[s]
    # ---- stage 0: z pre-pass (GL_LESS)
    zbuf = np.ones(vw * vh, np.float32)
    np.minimum.at(zbuf, pix, z[s])
    # ---- stage 1: within epsilon of the front surface, ONE/ONE blend of quality-weighted colour
    with np.errstate(invalid="ignore", divide="ignore"):
        dc = zbuf[pix]
        pc = _mul(I2E, (PX[s].astype(np.float32) + F(0.5)) + F(0.5), (PY[s].astype(np.float32) + F(0.5)) + F(0.5), dc, F(1.0))   # sic, :61
        near = ~(F(0.075) < _len3(*(pc[i] / pc[3] - fes[i][s] for i in range(3))))
        q = fq[s] / fd[s]                                                                # mvt_accum.fs:53
    s, pix, q = s[near], pix[near], q[near]
    lyr = L[T[s]]
    if shade_mode == 3:
        col = tuple(CAMERA_COLORS[lyr & 7, i] for i in range(3))
    else:
        colf = np.ascontiguousarray(scene["color"], np.uint8).astype(np.float32) / F(255.0)
        rgb = np.array([tex2d_linear(colf, int(li), tcx[j], tcy[j]) for li, j in zip(lyr, s)], np.float32).reshape(-1, 3)
        col = _shade(shade_mode, *(c[s] for c in fes), *(c[s] for c in n), rgb[:, 0], rgb[:, 1], rgb[:, 2])
    acc = np.zeros((vw * vh, 4), np.float32)
    for i in range(3):
        np.add.at(acc[:, i], pix, (col[i] * q).astype(np.float32))
    np.add.at(acc[:, 3], pix, q)
    # ---- normalise (trigrid_normalize.fs)
    fb_c, fb_d = np.zeros((vw * vh, 4), np.float32), np.ones(vw * vh, np.float32)
    hit = acc[:, 3] > F(0)
    fb_c[hit] = acc[hit] / acc[hit, 3:4]
    fb_d[hit] = zbuf[hit]
    return fb_c.reshape(vh, vw, 4), fb_d.reshape(vh, vw)
