"""CPU reference of the client's two overlays (source/kinect_client.cpp:672-683), as defined in include/rgbd_recon_hip.h.  numpy,
fp32 throughout, every operation in the order the header states it.

* draw_calibvis(...): "Draw TSDF", kinect::ReconCalibs::draw() (framework/reconstruction/recon_calibs.cpp:54-61, glsl/calib_vis.{vs,fs}).
  The TSDF is sampled by this module's own vectorised trilinear filter (sample_tsdf; cross-checked against oracle.tex3d by the tests).
* draw_frustums(...): "Draw frustums", Frustum::draw() (framework/calibration/frustum.cpp:45-95): the lines rasterised by the
  x-major / y-major half-open column or row walk that GL 4.4 section 14.5.1's diamond-exit rule reduces to for width 1.
The depth test of both is the literal in-order GL_LESS loop over primitives (first passing fragment at the smallest depth wins), not
the GPU's atomic key scheme.
"""
import numpy as np

F = np.float32
CALIB_LIMIT = F(0.01)           # recon_calibs.cpp:20
FRUSTUM_LINES = [(0, 4), (1, 5), (2, 6), (3, 7), (0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4)]   # frustum.cpp:48-84
LINE_COLOR = np.array([0, 1, 0, 1], np.float32)
POINT_COLOR = np.array([1, 0, 0, 1], np.float32)


# ---------------------------------------------------------------------- sampling and matrices
def axis_linear(u, n):
    """GL LINEAR + CLAMP_TO_EDGE along one axis: f = u * n - 0.5, taps clamp(floor(f)) and clamp(floor(f) + 1), weight fract(f)"""
    f = np.asarray(u, np.float32) * F(n) - F(0.5)
    fl = np.floor(f)
    a = (f - fl).astype(np.float32)
    i0 = np.clip(fl, 0, n - 1).astype(np.int64)
    i1 = np.clip(fl + F(1), 0, n - 1).astype(np.int64)
    return i0, i1, a


def lerp(a, b, t):
    return (a + (b - a) * t).astype(np.float32)


def sample_tsdf(vol, u, v, w):
    """texture(volume_tsdf, (u, v, w)).r of a [z][y][x] fp32 volume: x, then y, then z"""
    vol = np.asarray(vol, np.float32)
    nz, ny, nx = vol.shape
    x0, x1, ax = axis_linear(u, nx)
    y0, y1, ay = axis_linear(v, ny)
    z0, z1, az = axis_linear(w, nz)
    c00 = lerp(vol[z0, y0, x0], vol[z0, y0, x1], ax)
    c10 = lerp(vol[z0, y1, x0], vol[z0, y1, x1], ax)
    c01 = lerp(vol[z1, y0, x0], vol[z1, y0, x1], ax)
    c11 = lerp(vol[z1, y1, x0], vol[z1, y1, x1], ax)
    return lerp(lerp(c00, c10, ay), lerp(c01, c11, ay), az)


def mat_mul(m, x, y, z, w):
    """column-major m (16 fp32) times (x, y, z, w): sum_k m[k][row] * v[k], left to right"""
    m = np.asarray(m, np.float32).reshape(16)
    return tuple(m[r] * x + m[4 + r] * y + m[8 + r] * z + m[12 + r] * w for r in range(4))


def vol_to_world(bbox_min, bbox_max):
    """translate(bbox_min) * scale(bbox_max - bbox_min), fp32 (recon_calibs.cpp:38-45)"""
    m = np.zeros(16, np.float32)
    for a in range(3):
        m[a * 5] = F(bbox_max[a]) - F(bbox_min[a])
        m[12 + a] = F(bbox_min[a])
    m[15] = F(1)
    return m


def grid_coords(n):
    """(x + 0.5f) * stepX with stepX = 1.0f / n (volume_sampler.cpp:33-45)"""
    return (np.arange(n, dtype=np.float32) + F(0.5)) * (F(1) / F(n))


def window(clip, view):
    """whole-point clip test + window coordinates; returns (ok, xw, yw, zw)"""
    cx, cy, cz, cw = clip
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = (cw > 0) & ~(np.abs(cx) > cw) & ~(np.abs(cy) > cw) & ~(np.abs(cz) > cw)
        xw = (cx / cw * F(0.5) + F(0.5)) * F(view[0])
        yw = (cy / cw * F(0.5) + F(0.5)) * F(view[1])
        zw = cz / cw * F(0.5) + F(0.5)
    return ok & (zw < 1), xw, yw, zw


def point_pixels(xw, yw, size, view):
    """the pixels a point of `size` covers (k_points_scatter's rule), inside the view"""
    half = F(size) * F(0.5)
    x0, x1 = int(np.ceil((F(xw) - half) - F(0.5))), int(np.ceil((F(xw) + half) - F(0.5))) - 1
    y0, y1 = int(np.ceil((F(yw) - half) - F(0.5))), int(np.ceil((F(yw) + half) - F(0.5))) - 1
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, view[0] - 1), min(y1, view[1] - 1)
    return [(px, py) for py in range(y0, y1 + 1) for px in range(x0, x1 + 1)]


def gl_less(fragments, fb_c, fb_d):
    """the literal in-order depth test: fragments = iterable of (px, py, z, colour) in primitive order"""
    c, d = np.array(fb_c, np.float32, copy=True), np.array(fb_d, np.float32, copy=True)
    for px, py, z, col in fragments:
        if F(z) < d[py, px]:
            d[py, px] = F(z)
            c[py, px] = col
    return c, d


# ---------------------------------------------------------------------- "Draw TSDF"
def calib_color(d):
    """calib_vis.fs:17-30 (None: discarded)"""
    d = F(d)
    if d <= -CALIB_LIMIT:
        return None
    inv = F(abs(d)) / CALIB_LIMIT
    c = np.array([F(1) - inv, 0, 0, 1], np.float32) if d > 0 else np.array([0, F(1) - inv, 0, 1], np.float32)
    if d >= CALIB_LIMIT:
        c = np.array([0, 0, 1, 1], np.float32)
    return c


def calibvis_points(vol, gres, bbox_min, bbox_max, mv, pr, view):
    """every grid point in draw order -> (id, d, ok, xw, yw, zw); ok = not discarded and inside the whole-point clip"""
    gx, gy, gz = grid_coords(gres[0]), grid_coords(gres[1]), grid_coords(gres[2])
    w_, v_, u_ = np.meshgrid(gz, gy, gx, indexing="ij")          # [z][y][x]: the linear index is x fastest
    u, v, w = u_.reshape(-1), v_.reshape(-1), w_.reshape(-1)
    d = sample_tsdf(vol, u, v, w)
    one = F(1)
    pw = mat_mul(vol_to_world(bbox_min, bbox_max), u, v, w, one)
    pe = mat_mul(mv, pw[0], pw[1], pw[2], one)
    clip = mat_mul(pr, pe[0], pe[1], pe[2], one)
    ok, xw, yw, zw = window(clip, view)
    ok &= ~(d <= -CALIB_LIMIT)
    return np.arange(d.size), d, ok, xw, yw, zw


def draw_calibvis(vol, gres, bbox_min, bbox_max, mv, pr, view, fb_c, fb_d):
    ids, d, ok, xw, yw, zw = calibvis_points(vol, gres, bbox_min, bbox_max, mv, pr, view)

    def frags():
        for i in ids[ok]:
            col = calib_color(d[i])
            for px, py in point_pixels(xw[i], yw[i], 1, view):
                yield px, py, zw[i], col
    return gl_less(frags(), fb_c, fb_d)


# ---------------------------------------------------------------------- "Draw frustums"
def frustum_corners(cv_xyz, res):
    """getCornerPoints of a forward volume of resolution res = (rx, ry, rz), texels x fastest (CalibVolumes.cpp:98-113):
    (0,0), (0,ey), (ex,ey), (ex,0) at z = 0, then the same at ez"""
    v = np.asarray(cv_xyz, np.float32).reshape(int(res[2]), int(res[1]), int(res[0]), 3)
    ez, ey, ex = v.shape[0] - 1, v.shape[1] - 1, v.shape[2] - 1
    cx, cy = [0, 0, ex, ex], [0, ey, ey, 0]
    return np.array([v[0, cy[i], cx[i]] for i in range(4)] + [v[ez, cy[i], cx[i]] for i in range(4)], np.float32)


def clip_plane(a, b, da, db):
    if not (da >= 0) and not (db >= 0):
        return None
    if not (da >= 0):
        t = F(da) / F(da - db)
        a = [F(a[k] + (b[k] - a[k]) * t) for k in range(4)]
    elif not (db >= 0):
        t = F(db) / F(db - da)
        b = [F(b[k] + (a[k] - b[k]) * t) for k in range(4)]
    return a, b


def line_fragments(a, b, view):
    """fragments (px, py, z) of the width-1 line between clip-space points a -> b, in the walk's order"""
    a, b = [F(x) for x in a], [F(x) for x in b]
    r = clip_plane(a, b, a[2] + a[3], b[2] + b[3])                     # near
    if r is None:
        return []
    a, b = r
    r = clip_plane(a, b, a[3] - a[2], b[3] - b[2])                     # far
    if r is None:
        return []
    a, b = r
    if not (a[3] > 0) or not (b[3] > 0):
        return []
    W, H = F(view[0]), F(view[1])
    ax, ay, az = (a[0] / a[3] * F(0.5) + F(0.5)) * W, (a[1] / a[3] * F(0.5) + F(0.5)) * H, a[2] / a[3] * F(0.5) + F(0.5)
    bx, by, bz = (b[0] / b[3] * F(0.5) + F(0.5)) * W, (b[1] / b[3] * F(0.5) + F(0.5)) * H, b[2] / b[3] * F(0.5) + F(0.5)
    return window_line_fragments((ax, ay, az), (bx, by, bz), view)


def window_line_fragments(a, b, view):
    """the diamond-exit walk between window points a -> b (x, y, z)"""
    ax, ay, az = [F(x) for x in a]
    bx, by, bz = [F(x) for x in b]
    xmajor = abs(F(bx - ax)) >= abs(F(by - ay))
    s0, s1, o0, o1 = (ax, bx, ay, by) if xmajor else (ay, by, ax, bx)
    n_major, n_minor = (view[0], view[1]) if xmajor else (view[1], view[0])
    out = []
    for i in range(n_major):
        c = F(i) + F(0.5)
        if not ((c >= s0 and c < s1) if s1 > s0 else (c <= s0 and c > s1)):
            continue
        ds, dm = F(s1 - s0), F(o1 - o0)
        t = F(c - s0) / ds
        m = np.floor(F(o0 + F(dm * t)))
        tz = F(F(F(c - s0) * ds) + F(F(F(m + F(0.5)) - o0) * dm)) / F(F(ds * ds) + F(dm * dm))   # eq. 14.5: the fragment's centre projected onto the segment
        if not (m >= 0 and m < n_minor):
            continue
        z = F(az + F(F(bz - az) * tz))
        if z != z:
            continue
        z = z if z > 0 else F(0)
        z = z if z < 1 else F(1)
        out.append((i, int(m), z) if xmajor else (int(m), i, z))
    return out


def frustum_clip(mv, pr, p):
    e = mat_mul(mv, F(p[0]), F(p[1]), F(p[2]), F(1))
    return mat_mul(pr, e[0], e[1], e[2], e[3])


def draw_frustums(corners, cams, mv, pr, view, fb_c, fb_d):
    """corners [N][8][3], cams [N][3] (Frustum::getCameraPos): stream after stream, the 12 lines then the camera point"""
    def frags():
        for s in range(len(corners)):
            for i, j in FRUSTUM_LINES:
                for px, py, z in line_fragments(frustum_clip(mv, pr, corners[s][i]), frustum_clip(mv, pr, corners[s][j]), view):
                    yield px, py, z, LINE_COLOR
            ok, xw, yw, zw = window(frustum_clip(mv, pr, cams[s]), view)
            if ok:
                for px, py in point_pixels(xw, yw, 3, view):
                    yield px, py, zw, POINT_COLOR
    return gl_less(frags(), fb_c, fb_d)
