"""float64 numpy reference of the main path: integrate, brick depth limits, march and shade.  HIP-free, and written from the reference's
shaders alone -- not from oracle/tsdf_oracle.cpp and not from the kernels, whose operand order, binning and helpers it does not share:

* integrate     glsl/tsdf_integration.vs:23-59 over the voxel centres (i + .5) / res of VolumeSampler
* depth_limits  glsl/bricks.vs:16-20, bricks.gs:21-50, bricks.fs:5-7 with inc_bricks.glsl:22-38,60-62 over UnitCube::drawInstanced
                (unit_cube.cpp:20-29,53-62: one 14-index triangle strip) under drawDepthLimits (recon_integration.cpp:408-428: no culling,
                MIN blending over the clear colour (1, 0, 1, 0) of :144).  A real rasteriser: triangles, homogeneous near / far clipping,
                pixel-centre coverage by edge functions with a top-left rule, window z from the triangle's plane, gl_FrontFacing from the
                projected winding.
* march         glsl/tsdf_raymarch.fs:62-114 with intersectBox :363-374 and getStartPos / screenToVol :376-393
* shade         submitFragment :116-134, get_gradient :140-149, getWeights :151-166, blendColors :295-330, blendCameras :346-361 and
                shading.glsl:24-30,54-69 (modes 0, 2, 3)

Sampler state as in SURVEY.md Appendix A: LINEAR for the LUTs, silhouette, quality, colour and the TSDF, NEAREST for depth, CLAMP_TO_EDGE
everywhere.  A linear fetch is the weighted sum of its 2^d taps (weights = products of the per-axis fractions), not a chain of lerps.

Everything is float64, vectorised over voxels / pixels and looped over streams, faces and march steps.  Matrices are the 16 column-major
floats GL hands out (scene.gl_flat).  Images are [row][column] with row 0 = gl_FragCoord.y 0.5.

Every part also returns its own *decision margin*: how close the float64 value came to a branch, a texel boundary, an integer under a
ceil() or a triangle edge.  Where that margin is below the fp32 error of the operation, an fp32 implementation may legitimately decide the
other way; the tests exclude those elements and nothing else.
"""
import numpy as np

INF = np.inf


# ---------------------------------------------------------------------------------------------------------------- sampling
def _axis(u, n):
    """LINEAR + CLAMP_TO_EDGE along one axis: (i0, i1, fraction)"""
    f = np.clip(np.asarray(u, np.float64) * n - 0.5, -1.0, float(n))           # outside [-1, n] both taps are the edge texel anyway
    fl = np.floor(f)
    a = f - fl
    i = np.nan_to_num(fl, nan=-1.0).astype(np.int64)
    return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), a


def tex3d(t, p):
    """t [nz][ny][nx][c] (or [nz][ny][nx]), p [..., 3] normalised (x, y, z) -> [..., c]"""
    t = np.asarray(t, np.float64)
    if t.ndim == 3:
        return tex3d(t[..., None], p)[..., 0]
    nz, ny, nx = t.shape[:3]
    x0, x1, ax = _axis(p[..., 0], nx)
    y0, y1, ay = _axis(p[..., 1], ny)
    z0, z1, az = _axis(p[..., 2], nz)
    out = 0.0
    for zi, wz in ((z0, 1.0 - az), (z1, az)):
        for yi, wy in ((y0, 1.0 - ay), (y1, ay)):
            for xi, wx in ((x0, 1.0 - ax), (x1, ax)):
                out = out + t[zi, yi, xi] * (wz * wy * wx)[..., None]
    return out


def tex2d_linear(t, u, v, taps=False):
    """t [h][w][c] or [h][w] -> [..., c] / [...]; taps=True also returns the four texels [..., 4(, c)]"""
    t = np.asarray(t, np.float64)
    h, w = t.shape[:2]
    x0, x1, ax = _axis(u, w)
    y0, y1, ay = _axis(v, h)
    tp = [t[y0, x0], t[y0, x1], t[y1, x0], t[y1, x1]]
    ws = [(1 - ax) * (1 - ay), ax * (1 - ay), (1 - ax) * ay, ax * ay]
    if t.ndim == 3:
        ws = [k[..., None] for k in ws]
    out = sum(a * b for a, b in zip(tp, ws))
    return (out, np.stack(tp, -1 if t.ndim == 2 else -2)) if taps else out


def nearest_index(u, n):
    f = np.floor(np.clip(np.asarray(u, np.float64) * n, -1.0, float(n)))
    return np.clip(np.nan_to_num(f, nan=-1.0).astype(np.int64), 0, n - 1)


def tex2d_nearest(t, u, v):
    h, w = t.shape[:2]
    return np.asarray(t, np.float64)[nearest_index(v, h), nearest_index(u, w)]


def texel_boundary_distance(u, n):
    """distance of u * n to the next texel boundary of a nearest fetch; boundaries are the integers 1 .. n-1 (outside the image the
    coordinate is clamped: no boundary there)"""
    x = np.asarray(u, np.float64) * n
    return np.abs(x - np.clip(np.rint(x), 1, n - 1)) if n > 1 else np.full(np.shape(x), INF)


def _lut(scene, key, i, res_key, nc):
    r = [int(x) for x in scene[res_key]]
    return np.asarray(scene[key][i], np.float64).reshape(r[2], r[1], r[0], nc)


# ---------------------------------------------------------------------------------------------------------------- integrate
def voxel_positions(res):
    """in_Position of the integration draw: the voxel centres, [z][y][x][3]"""
    cz, cy, cx = [(np.arange(int(r)) + 0.5) / int(r) for r in (res[2], res[1], res[0])]
    z, y, x = np.meshgrid(cz, cy, cx, indexing="ij")
    return np.stack([x, y, z], -1)


def integrate(scene, res, limit, order=None):
    """tsdf_integration.vs:23-59 -> (volume [z][y][x], margin [z][y][x]).  `limit` is the fp32 uniform.  `order`: stream order (default
    0 .. n-1).  The margin is the smallest distance of a compared value to what it was compared with, over all streams:
    |silhouette - 1| (:33) unless all four taps are exactly 1, |weighted_tsd - limit| (:35) unless weighted_tsd is an assigned +-limit,
    |sdist + limit| and |sdist - limit| (:42, :46), and the distance of u w / v h to the next texel boundary of the nearest depth fetch
    (:40), in texels.  A NaN compares false in every precision: it has no margin."""
    limit = float(np.float32(limit))
    pos = voxel_positions(res)
    shape = pos.shape[:3]
    tsd = np.full(shape, limit)
    tw = np.zeros(shape)
    assigned = np.ones(shape, bool)                       # weighted_tsd holds an assigned +-limit, not a computed mean
    margin = np.full(shape, INF)
    w, h = int(scene["width"]), int(scene["height"])
    for i in (range(int(scene["n"])) if order is None else order):
        pc = tex3d(_lut(scene, "cv_xyz_inv", i, "inv_res", 4), pos)                                  # :31
        u, v, z = pc[..., 0], pc[..., 1], pc[..., 2]
        sil, taps = tex2d_linear(scene["silhouette"][i], u, v, taps=True)                             # :32
        ones = (taps == 1.0).all(-1)
        sil = np.where(ones, 1.0, sil)                    # a filter returns a constant exactly; a weighted sum in float64 need not
        margin = np.fmin(margin, np.where(ones, INF, np.abs(sil - 1.0)))
        cut = sil < 1.0                                                                               # :33
        margin = np.fmin(margin, np.where(cut & ~assigned, np.abs(tsd - limit), INF))
        skip = cut & (tsd >= limit)                                                                   # :35-38
        tsd = np.where(skip, -limit, tsd)
        assigned = assigned | skip
        live = ~skip
        depth = tex2d_nearest(np.asarray(scene["depth"][i])[..., 0], u, v)                            # :40
        margin = np.fmin(margin, np.where(live, np.minimum(texel_boundary_distance(u, w), texel_boundary_distance(v, h)), INF))
        sd = z - depth                                                                                # :41
        margin = np.fmin(margin, np.where(live, np.minimum(np.abs(sd + limit), np.abs(sd - limit)), INF))
        front = live & (sd <= -limit)                                                                 # :42-45
        band = live & ~front & ~(sd >= limit)                                                         # :49-54
        wt = tex2d_linear(scene["quality"][i], u, v)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = (tsd * tw + wt * sd) / (tw + wt)
        tsd = np.where(front, -limit, np.where(band, mean, tsd))
        tw = np.where(band, tw + wt, tw)
        assigned = (assigned | front) & ~band
    return tsd, margin


def brick_voxel_mask(res, ranges, occupied):
    """voxels a culled integrate() writes: the union of the occupied bricks' voxel ranges ([lo3, hi3) per brick, the brick layout of
    divideBox); every other voxel keeps the cleared -limit (recon_integration.cpp:249-258)"""
    m = np.zeros((int(res[2]), int(res[1]), int(res[0])), bool)
    for b in np.flatnonzero(occupied):
        lo, hi = ranges[b][:3], ranges[b][3:]
        m[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = True
    return m


# ---------------------------------------------------------------------------------------------------------------- matrices
def mat(m16):
    """16 column-major floats -> 4x4 (row, col) float64"""
    return np.asarray(m16, np.float64).reshape(4, 4).T.copy()


def vol_to_world(bbox_min, bbox_max):
    """recon_integration.cpp:66-72"""
    lo, hi = np.asarray(bbox_min, np.float64), np.asarray(bbox_max, np.float64)
    m = np.eye(4)
    m[:3, :3] = np.diag(hi - lo)
    m[:3, 3] = lo
    return m


def _xf(m, p, w=1.0):
    """m . (p, w) for p [..., 3] -> [..., 4]"""
    return p @ m[:, :3].T + w * m[:, 3]


def pixel_centres(view):
    w, h = view
    y, x = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    return x, y


# ---------------------------------------------------------------------------------------------------------------- depth limits
CUBE = np.array([(1, 1, 1), (0, 1, 1), (1, 1, 0), (0, 1, 0), (1, 0, 1), (0, 0, 1), (0, 0, 0), (1, 0, 0)], np.float64)   # unit_cube.cpp:20-29
STRIP = (3, 2, 6, 7, 4, 2, 0, 3, 1, 6, 5, 4, 1, 0)                                                                        # unit_cube.cpp:56-59


def strip_triangles():
    """The 12 triangles GL assembles from the strip, every one with the winding of the first (odd triangles swap their first two
    vertices), each with the neighbour bricks.gs:24-43 tests: (vertex ids, axis, direction)"""
    out = []
    for k in range(len(STRIP) - 2):
        ids = (STRIP[k + 1], STRIP[k], STRIP[k + 2]) if k & 1 else (STRIP[k], STRIP[k + 1], STRIP[k + 2])
        s = CUBE[list(ids)].sum(0)
        axis = next(a for a in range(3) if s[a] < 1.0 or s[a] > 2.0)
        out.append((ids, axis, int(s[axis] / 3.0 * 2.0 - 1.0)))
    return out


def _clip(poly):
    """Sutherland-Hodgman of a convex clip-space polygon [n][4] against near (z >= -w) and far (z <= w)"""
    for sign in (1.0, -1.0):
        if len(poly) == 0:
            break
        d = poly[:, 3] + sign * poly[:, 2]
        out = []
        for k in range(len(poly)):
            a, b, da, db = poly[k], poly[(k + 1) % len(poly)], d[k], d[(k + 1) % len(poly)]
            if da >= 0:
                out.append(a)
            if (da >= 0) != (db >= 0):
                out.append(a + (b - a) * (da / (da - db)))
        poly = np.array(out).reshape(-1, 4)
    return poly


def _window(poly, view):
    ndc = poly[:, :3] / poly[:, 3:4]
    return np.stack([(ndc[:, 0] * 0.5 + 0.5) * view[0], (ndc[:, 1] * 0.5 + 0.5) * view[1], ndc[:, 2] * 0.5 + 0.5], -1)


def _pixel_box(win, view, pad):
    x0 = max(int(np.floor(win[:, 0].min() - pad)), 0)
    x1 = min(int(np.ceil(win[:, 0].max() + pad)), view[0])
    y0 = max(int(np.floor(win[:, 1].min() - pad)), 0)
    y1 = min(int(np.ceil(win[:, 1].max() + pad)), view[1])
    if x0 >= x1 or y0 >= y1:
        return None
    y, x = np.meshgrid(np.arange(y0, y1) + 0.5, np.arange(x0, x1) + 0.5, indexing="ij")
    return (slice(y0, y1), slice(x0, x1)), x, y


def _covered(win, x, y):
    """pixel centres inside the convex window polygon -> (mask, counter-clockwise?).  A centre exactly on an edge belongs to the polygon
    only if that is a left edge or a horizontal top edge (top-left rule: of two polygons that share an edge exactly one owns its points)"""
    n = len(win)
    area = sum(win[k, 0] * win[(k + 1) % n, 1] - win[(k + 1) % n, 0] * win[k, 1] for k in range(n))
    if area == 0.0:
        return np.zeros(x.shape, bool), False
    p = win if area > 0 else win[::-1]                 # counter-clockwise (y up): the interior is on the left of every edge
    m = np.ones(x.shape, bool)
    for k in range(n):
        a, b = p[k], p[(k + 1) % n]
        ex, ey = b[0] - a[0], b[1] - a[1]
        e = ex * (y - a[1]) - ey * (x - a[0])
        m &= (e > 0) | ((e == 0) & bool(ey < 0 or (ey == 0 and ex < 0)))       # a left edge runs downwards, a top edge leftwards
    return m, bool(area > 0)


def _segment_distance(a, b, x, y):
    dx, dy = b[0] - a[0], b[1] - a[1]
    l2 = dx * dx + dy * dy
    t = np.clip(((x - a[0]) * dx + (y - a[1]) * dy) / l2, 0.0, 1.0) if l2 > 0 else 0.0
    return np.hypot(x - (a[0] + t * dx), y - (a[1] + t * dy))


def exposed_faces(counters, occupied_ids, res_bricks):
    """(brick id, axis, direction) of every face bricks.gs lets through: the neighbour's index is the uvec3 sum of :28,34,40 (it wraps),
    its id get_id of inc_bricks.glsl:26-28 in 32-bit arithmetic, and a read past the counters gives 0 (robust buffer access)"""
    counters = np.asarray(counters, np.int64)
    rx, ry = int(res_bricks[0]), int(res_bricks[1])
    stride = (1, rx, rx * ry)
    out = []
    for b in np.asarray(occupied_ids, np.int64):
        for axis in range(3):
            for d in (-1, 1):
                nb = (int(b) + d * stride[axis]) % (1 << 32)
                if not (nb < counters.size and counters[nb] > 10):                                  # brick_occupied, inc_bricks.glsl:60-62
                    out.append((int(b), axis, d))
    return out


def depth_limits(counters, occupied_ids, res_bricks, brick_size, bbox_min, mv, proj, view):
    """-> (peels [h][w][3] = the RGB of m_view_depth, covered [h][w], edge distance [h][w] in pixels).  occupied_ids: the Occupied buffer
    (updateOccupiedBricks, recon_integration.cpp:430-445); counters: the Bricks buffer the geometry shader reads."""
    w, h = view
    pmv = mat(proj) @ mat(mv)
    rx, ry = int(res_bricks[0]), int(res_bricks[1])
    bs, lo = np.asarray(brick_size, np.float64), np.asarray(bbox_min, np.float64)
    peels = np.empty((h, w, 3))
    peels[...] = (1.0, 0.0, 1.0)
    covered = np.zeros((h, w), bool)
    edge = np.full((h, w), INF)
    tris = strip_triangles()
    live = set(exposed_faces(counters, occupied_ids, res_bricks))
    for b in np.asarray(occupied_ids, np.int64):
        b = int(b)
        idx = np.array([b % (rx * ry) % rx, b % (rx * ry) // rx, b // (rx * ry)], np.float64)        # index_3d
        clip = _xf(pmv, idx * bs + lo + CUBE * bs)                                                   # to_world, bricks.vs:19
        for ids, axis, d in tris:
            if (b, axis, d) not in live:
                continue
            poly = _clip(clip[list(ids)])
            if len(poly) < 3:
                continue
            win = _window(poly, view)
            box = _pixel_box(win, view, 0.0)
            if box is None:
                continue
            sl, x, y = box
            m, ccw = _covered(win, x, y)
            if not m.any():
                continue
            c = win.mean(0)
            plane = np.linalg.lstsq(np.c_[win[:, :2] - c[:2], np.ones(len(win))], win[:, 2], rcond=None)[0]
            z = plane[0] * (x - c[0]) + plane[1] * (y - c[1]) + plane[2]
            frag = np.stack([z, -z, np.ones_like(z) if ccw else z], -1)                              # bricks.fs:6, glFrontFace default CCW
            peels[sl] = np.where(m[..., None], np.minimum(peels[sl], frag), peels[sl])               # glBlendEquation(GL_MIN)
            covered[sl] |= m
        for axis in range(3):
            for d in (-1, 1):
                if (b, axis, d) not in live:
                    continue
                a1, a2 = (axis + 1) % 3, (axis + 2) % 3
                q = np.zeros((4, 3))
                q[:, axis] = (d + 1) // 2
                q[:, a1] = (0, 1, 1, 0)
                q[:, a2] = (0, 0, 1, 1)
                poly = _clip(_xf(pmv, idx * bs + lo + q * bs))
                if len(poly) < 2:
                    continue
                win = _window(poly, view)
                box = _pixel_box(win, view, 2.0)
                if box is None:
                    continue
                sl, x, y = box
                for k in range(len(win)):
                    edge[sl] = np.minimum(edge[sl], _segment_distance(win[k], win[(k + 1) % len(win)], x, y))
    return peels, covered, edge


# ---------------------------------------------------------------------------------------------------------------- march
class View:
    """the matrix block of draw(), recon_integration.cpp:182-205, and tsdf_raymarch.vs:14"""

    def __init__(self, mv, proj, view, bbox_min, bbox_max):
        self.size = tuple(int(v) for v in view)
        self.mv, self.proj = mat(mv), mat(proj)
        self.v2w = vol_to_world(bbox_min, bbox_max)
        self.mvv = self.mv @ self.v2w                                      # volume -> eye
        self.clip = self.proj @ self.mvv                                   # volume -> clip
        self.unclip = np.linalg.inv(self.clip)
        self.cam = np.linalg.solve(self.mvv, np.array([0.0, 0.0, 0.0, 1.0]))[:3]        # CameraPos
        self.normal = np.linalg.inv(self.mvv).T                            # NormalMatrix

    def window_to_vol(self, x, y, z):
        """screenToVol, tsdf_raymarch.fs:376-382: window -> NDC -> volume"""
        w, h = self.size
        ndc = np.stack([x / w * 2 - 1, y / h * 2 - 1, z * 2 - 1, np.ones_like(x)], -1)
        p = ndc @ self.unclip.T
        return p[..., :3] / p[..., 3:4]

    def ray_directions(self):
        """normalize(pass_Position - CameraPos) for every pixel centre: pass_Position is the point of the cube's surface under the pixel,
        any other point of the pixel's line of sight gives the same direction"""
        x, y = pixel_centres(self.size)
        d = self.window_to_vol(x, y, np.ones_like(x)) - self.cam
        return d / np.linalg.norm(d, axis=-1, keepdims=True)

    def in_clip(self, p):
        c = _xf(self.clip, p)
        return (c[..., 2] >= -c[..., 3]) & (c[..., 2] <= c[..., 3])

    def frag_depth(self, p):
        """tsdf_raymarch.fs:123,133"""
        vz = _xf(self.mvv, p)[..., 2]
        with np.errstate(invalid="ignore", divide="ignore"):
            return (self.proj[2, 2] * vz + self.proj[2, 3]) / -vz * 0.5 + 0.5


def _integer_distance(x):
    with np.errstate(invalid="ignore"):
        d = np.abs(x - np.rint(x))
    return np.where(np.isnan(d), 0.0, d)


def box_interval(V, step):
    """:75-86 -> (covered, start position, max_num_samples as float, ceil margin).  A fragment exists where the unit cube's surface under
    the pixel is inside the clip volume: its entry or its exit point lies between the near and the far plane."""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / step
        tbot, ttop = inv * (0.0 - V.cam), inv * (1.0 - V.cam)
    t0 = np.minimum(ttop, tbot).max(-1)
    t1 = np.maximum(ttop, tbot).min(-1)
    hit = t0 <= t1
    entry, leave = V.cam + step * t0[..., None], V.cam + step * t1[..., None]
    with np.errstate(invalid="ignore"):
        covered = hit & (((t0 > 0) & V.in_clip(entry)) | ((t1 > 0) & V.in_clip(leave)))
    t_near = np.where(t0 < 0, 0.0, t0)
    length = np.abs(t1 - t_near)
    margin = np.where(covered, _integer_distance(length), np.abs(t1 - t0))
    return covered, V.cam + step * t_near[..., None], np.where(covered, np.ceil(length), 0.0), margin


def start_pos(V, peels):
    """getStartPos, :384-393 -> (pos_front, distance(pos_front, pos_back)); peels [h][w][>=3] as texelFetch reads them"""
    x, y = pixel_centres(V.size)
    pe = np.asarray(peels, np.float64)
    r, g, b = pe[..., 0], pe[..., 1], pe[..., 2]
    r = np.where(r >= b, 0.0, r)                                           # gl_DepthRange.near
    front = V.window_to_vol(x, y, r)
    back = V.window_to_vol(x, y, -g)
    back = np.where((r >= 1.0)[..., None], front, back)
    return front, np.linalg.norm(front - back, axis=-1)


def march(volume, peels, mv, proj, view, limit, bbox_min, bbox_max):
    """tsdf_raymarch.fs:62-114 for every pixel centre -> dict: n (samples taken), hit, pos (the refined hit position, volume space),
    depth (gl_FragDepth), covered (a fragment exists), margin.  peels None: skipSpace off.  The margin is the smallest |density - IsoValue|
    over the samples taken up to and including the hit, and the distance of the ceil()'s argument (:73, :85) to an integer; for a pixel
    outside the cube's silhouette, t0 - t1 of intersectBox."""
    limit = float(np.float32(limit))
    sd = limit * 0.5                                                       # sampleDistance :34
    V = View(mv, proj, view, bbox_min, bbox_max)
    step = V.ray_directions() * sd                                         # :64
    covered, pos, max_n, margin = box_interval(V, step)
    if peels is not None:                                                  # :69-74
        pos, length = start_pos(V, peels)
        max_n = np.where(covered, np.ceil(length / sd), 0.0)
        margin = np.where(covered, _integer_distance(length / sd), margin)
    vol = np.asarray(volume, np.float64)
    h, w = V.size[1], V.size[0]
    n = np.zeros((h, w))
    hit = np.zeros((h, w), bool)
    prev = np.full((h, w), -limit)                                         # :89
    pos = pos.copy()
    active = n < max_n
    while active.any():                                                    # :92-110
        n[active] += 1
        p, s = pos[active], step[active]
        dens = tex3d(vol, p)
        with np.errstate(invalid="ignore", divide="ignore"):
            margin[active] = np.fmin(margin[active], np.where(np.isnan(dens), INF, np.abs(dens)))
            inside = dens > 0.0                                            # :98
            refined = (p - s) - s * (prev[active] / (dens - prev[active]))[..., None]                # :100
        pos[active] = np.where(inside[..., None], refined, p + s)
        pa = prev[active]
        prev[active] = np.where(inside, pa, dens)
        hit[active] = inside
        active = active & ~hit & (n < max_n)
    with np.errstate(invalid="ignore"):
        depth = np.where(hit, V.frag_depth(pos), 1.0)
    margin = np.where(hit & np.isnan(depth), 0.0, margin)                  # a NaN gl_FragDepth: what GL does with it is undefined
    return dict(n=n, hit=hit, pos=pos, depth=depth, covered=covered, margin=margin, view=V)


# ---------------------------------------------------------------------------------------------------------------- shade
CAMERA_COLORS = np.array([(228, 26, 28), (55, 126, 184), (77, 175, 74), (152, 78, 163), (255, 127, 0)], np.float64) / 255.0    # shading.glsl:24-30


def gradient_normal(volume, pos, limit):
    """get_gradient, :140-149 (volume space, unit length, pointing to smaller density)"""
    sd = float(np.float32(limit)) * 0.5
    vol = np.asarray(volume, np.float64)
    g = np.stack([tex3d(vol, pos + o) - tex3d(vol, pos - o) for o in np.eye(3) * sd], -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return -g / np.linalg.norm(g, axis=-1, keepdims=True)


def shade(scene, volume, pos, V, limit, mode):
    """submitFragment :116-131 at the positions pos [n][3] -> dict: rgba [n][4] (out_Color), normal [n][3] (view_normal), margin [n]:
    the smallest |dist - limit| over the streams (:159, :311) and total_weight against 0 (:321, :359)."""
    assert mode in (0, 2, 3)
    limit = float(np.float32(limit))
    pos = np.asarray(pos, np.float64)
    vn = gradient_normal(volume, pos, limit) @ V.normal[:3, :3].T                                     # :119
    with np.errstate(invalid="ignore", divide="ignore"):
        vn = vn / np.linalg.norm(vn, axis=-1, keepdims=True)
    k = len(pos)
    margin = np.full(k, INF)
    tc, tc2, cam = np.zeros((k, 3)), np.zeros((k, 3)), np.zeros((k, 3))
    tw, tw2, wsum = np.zeros(k), np.zeros(k), np.zeros(k)
    for i in range(int(scene["n"])):
        pc = tex3d(_lut(scene, "cv_xyz_inv", i, "inv_res", 4), pos)                                   # :303
        uv = tex3d(_lut(scene, "cv_uv", i, "lut_res", 2), pc[..., :3])                                # :304
        col = tex2d_linear(np.asarray(scene["color"][i], np.float64) / 255.0, uv[..., 0], uv[..., 1])   # :305, RGB8 unorm
        depth = tex2d_nearest(np.asarray(scene["depth"][i])[..., 0], pc[..., 0], pc[..., 1])          # :307
        dist = np.abs(depth - pc[..., 2])
        margin = np.minimum(margin, np.abs(dist - limit))
        q = np.where(dist < limit, tex2d_linear(scene["quality"][i], pc[..., 0], pc[..., 1]), 0.0)   # :311-313
        with np.errstate(invalid="ignore", divide="ignore"):
            tc += col * (q / (dist + 0.01))[..., None]                                                # :315-316
            tw += q / (dist + 0.01)
            tc2 += col / dist[..., None]                                                              # :318-319
            tw2 += 1.0 / dist
        cam += CAMERA_COLORS[i % len(CAMERA_COLORS)] * q[..., None]                                   # :352-355, weights of getWeights :151-166
        wsum += q
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode == 3:
            margin = np.minimum(margin, np.where(wsum > 0, wsum, INF))
            rgb = np.where((wsum <= 0)[..., None], 1.0, cam / wsum[..., None])                       # :358-359
            alpha = np.ones(k)
        else:
            margin = np.minimum(margin, np.where(tw > 0, tw, INF))
            good = tw > 0                                                                             # :321-329
            rgb = np.where(good[..., None], tc / tw[..., None], tc2 / tw2[..., None])
            alpha = np.where(good, 1.0, -1.0)
            if mode == 2:
                rgb = vn @ V.mv[:3, :3]                                                               # shading.glsl:66: inverse(gl_NormalMatrix) = transpose(MV)
    return dict(rgba=np.concatenate([rgb, alpha[:, None]], -1), normal=vn, margin=np.where(np.isnan(margin), 0.0, margin))

