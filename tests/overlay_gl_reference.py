"""float64 numpy reference of the client's overlay draws.  HIP-free, and written from the reference's host code and shaders and the OpenGL 4.4
specification alone -- not from include/rgbd_recon_hip.h, not from the kernels and not from the four fp32 twins (overlay_reference,
client_overlay_reference, brick_overlay_reference, sensor_view_reference), whose formulation of a line (a half-open column / row walk) it
does not share:

* order            source/kinect_client.cpp:672-707: ReconCalibs::draw, drawFrustums, drawOccupiedBricks, g_bbox.draw, TextureBlitter::blit; the
                   texture windows of :483-515 come last, with the GUI
* draw_calibvis    recon_calibs.cpp:20,38-61 (limit 0.01f, vol_to_world = translate(min) * scale(max - min)), volume_sampler.cpp:14-23,71-73 (one
                   GL_POINT per cell of the inverse volume's grid, x fastest; (x + 0.5f) * stepX is a float product: the buffer is data),
                   calib_vis.vs:25-38, calib_vis.fs:17-30
* draw_frustums    CalibVolumes.cpp:98-113 (the eight corner texels), frustum.cpp:45-95 (12 GL_LINES in green, then glPointSize(3) and one red
                   GL_POINT at getCameraPos()), frustum.cpp:21-33,97-111 (camera_position below, float64)
* draw_bbox        BoundingBox.cpp:298-318 (colour (1, 1, 1, 0.75), glLineWidth(2.0), inside a pushed attribute set: no other draw inherits the
                   width), gloostRenderGoodies.h:251-304 (six GL_LINE_LOOPs of four vertices: 24 segments, each loop closed by its last segment)
* draw_bricks      recon_integration.cpp:447-454, bricks.vs:16-20 with inc_bricks.glsl:22-24,30-38 (to_world, index_3d), solid.fs ((Color, 1)),
                   unit_cube.cpp:20-29,74-83 (vertex table, the 12 GL_LINES of drawWireInstanced, instances in list order)
* blit             kinect_client.cpp:704-707, view_lod.cpp:29 (resolution_full = uvec2(width * 1.5f, height)), texture_blitter.cpp:34-39,50-66
                   (glViewport(0, 0, resolution), depth test off), screen_quad.cpp:11-15,32-35 (one triangle (-1,-1) (3,-1) (-1,3) with
                   texture coordinates (0,0) (2,0) (0,2)), texture_passthrough.vs:7-12 (noperspective), texture_passthrough.fs:46-47
* sensor_window    kinect_client.cpp:499-509, imgui_impl_glfw_glb.cpp:68-74 (blend SRC_ALPHA / ONE_MINUS_SRC_ALPHA on all four channels, no depth
                   test, scissor), :78-85 (orthographic: window x = p.x, window y = height - p.y), :111-124 (array mode, glScissor's (int)
                   casts), :260-285 (the quarter turn), NetKinectArray.cpp:159-188 (formats, and NEAREST for the depth arrays alone)

Lines (OpenGL 4.4, 14.5.1), literally.  Pixel f with centre (x_f, y_f) owns the diamond R_f = {|x - x_f| + |y - y_f| < 1/2}.  The segment
p_a -> p_b produces a fragment for f iff the segment p_a - (e, e^2) -> p_b - (e, e^2) intersects R_f and p_b - (e, e^2) is not in R_f; e is
the spec's "tiny amount" (2^-20 here), which settles a segment through a diamond's corner or along its edge.  Evaluated per pixel of the
segment's bounding box: the L1 distance of a point of the segment to the centre is convex and piecewise linear along the segment, so its
minimum is at an end or where the segment crosses the centre's column or row.  No major axis, no walk.  A fragment's depth is eq. 14.5 / 14.6:
t = (p_r - p_a) . (p_b - p_a) / |p_b - p_a|^2 with p_r the fragment's CENTRE, z = (1 - t) z_a + t z_b.
Wide lines (14.5.2.2), literally: w = the width rounded; the segment moved by -(w - 1) / 2 in its minor direction (y for |dx| >= |dy|) is
rasterised as above and each fragment is the lowest of a column (row) of w fragments.
Clipping: in clip space against the near and the far plane (every point left has w >= 0).  x and y are not clipped -- a rasteriser with a guard
band does not, GL allows both, and the two differ only where the line leaves the viewport: that pixel gets margin 0 (`open`).
Points: clipped by the centre, the square c - s/2 <= p < c + s/2 over pixel centres p, the size not rounded (tests/backend_reference.py).
Depth test: GL_LESS in draw order -- per pixel the first of the fragments of smallest z among those with z < the depth before the overlay.

What GL leaves open, and how it is treated here:
* 14.5.1 binds no implementation to the diamond rule at a segment's two ends (conditions 1-4 allow one fragment more or less, one pixel off):
  the pixel that holds an end point of a (clipped, shifted) segment has margin 0 for that segment (`open`), and so have the other pixels of a
  wide line's column there.  Every other pixel is held to the literal rule.
* which fragment's data a wide line's replicated fragments carry: here the lowest one's (eq. 14.5 at its centre, on the moved segment).
* kinect_client.cpp:258 enables GL_PROGRAM_POINT_SIZE and calib_vis.vs writes no gl_PointSize (calib_sample.vs has it commented out): the size
  of ReconCalibs' points is undefined.  1 is taken, as glPointSize's initial value; Frustum::draw's glPointSize(3) is never undone, so a
  driver that falls back to the fixed-function size would draw them 3 pixels wide from the second frame on.  The camera points themselves are
  drawn without a program: size 3.
* the top-left rule of the texture windows' two triangles at a pixel centre exactly on the quad's outline: edge margin 0.
* ViewLod's colour texture wraps MIRRORED_REPEAT (view_lod.cpp:52-53), not CLAMP_TO_EDGE; the blit's coordinates (x + .5) / vw never bring a
  LINEAR tap outside the image (asserted), so the wrap mode is never reached.

Every draw returns (rgba [h][w][4], depth [h][w], margin [h][w][4], touched [h][w]) -- the framebuffer after the overlay in float64, row 0 =
gl_FragCoord.y 0.5.  touched: a fragment was produced there (kept, or failed the depth test), or one was missed by less than NEAR_MISS, or the
pixel is `open`.  The margin says how close the float64 arithmetic came to deciding a pixel otherwise, per TERMS, each in its own unit; it is
the smallest value over all fragments that touch the pixel, kept or discarded:

  edge   pixels: |L1 distance of the line to the pixel centre - 1/2|; of a point's square or a window quad's edge to the pixel centre; for a
         wide line also ||dx| - |dy||, the choice of the minor direction
  test   the operand's own unit: d to -0.01, 0 and 0.01 of calib_vis.fs (TSDF units; a sample whose eight taps are equal is data and compares
         exactly in every precision: no margin), a point's clip coordinates to +-w (NDC), window z to the depth before the overlay, a NEAREST
         texel coordinate to a texel boundary (texels)
  zgap   window z: the winning fragment's distance to the nearest passing fragment of another colour
  open   0 at the pixels GL leaves open (above), infinite elsewhere
"""
import numpy as np

import main_path_reference as R
from main_path_reference import mat, tex2d_linear, tex2d_nearest, tex3d

INF = np.inf
TERMS = ("edge", "test", "zgap", "open")
EDGE, TEST, ZGAP, OPEN = range(4)
NEAR_MISS = 1e-3                                       # pixels: a fragment missed by less than this still marks its pixel touched
TIE = 2.0 ** -20                                       # the spec's perturbation (e, e^2) of a line's end points
CALIB_LIMIT = float(np.float32(0.01))                  # recon_calibs.cpp:20
LINE_GREEN, POINT_RED = (0.0, 1.0, 0.0, 1.0), (1.0, 0.0, 0.0, 1.0)       # frustum.cpp:47,92 (glColor3f: alpha 1)
BBOX_WHITE = (1.0, 1.0, 1.0, float(np.float32(0.75)))                    # BoundingBox.cpp:304
WIRE_RED = (1.0, 0.0, 0.0, 1.0)                                          # recon_integration.cpp:449, solid.fs
FRUSTUM_LINES = ((0, 4), (1, 5), (2, 6), (3, 7), (0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4))   # frustum.cpp:48-84
CUBE_WIRE = ((0, 1), (0, 2), (0, 4), (5, 1), (5, 4), (5, 6), (3, 1), (3, 6), (3, 2), (7, 2), (7, 4), (7, 6))        # unit_cube.cpp:76-81
ROT = np.float32(90.0) * np.float32(0.017453292519943295)                # radians(90.0): the float 1.5707964
ROT_COS = float(np.float32(np.cos(np.float64(ROT))))                     # cos(rot) as a float: -4.3711388e-08, not 0
ROT_SIN = float(np.float32(np.sin(np.float64(ROT))))                     # sin(rot) as a float: 1
NEAREST_TYPES = (1, 5)                                                   # NetKinectArray.cpp:180-188


# ---------------------------------------------------------------------------------------------------------------- fragments
class Frags:
    """the fragments of a draw in draw order, and the margins / touched mask they leave behind"""

    def __init__(self, view):
        self.view = (int(view[0]), int(view[1]))
        self.margin = np.full((self.view[1], self.view[0], 4), INF)
        self.touched = np.zeros((self.view[1], self.view[0]), bool)
        self.prim, self.pix, self.z, self.col = [], [], [], []
        self.n_prim = 0

    def add(self, px, py, z, colour):
        """fragments of the next primitive; colour (4,) or [n][4]"""
        px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
        if px.size:
            self.prim.append(np.full(px.size, self.n_prim))
            self.pix.append(py * self.view[0] + px)
            self.z.append(np.clip(np.asarray(z, np.float64), 0.0, 1.0))
            self.col.append(np.broadcast_to(np.asarray(colour, np.float64), (px.size, 4)))
            self.touched[py, px] = True
        self.n_prim += 1

    def lower(self, term, px, py, value):
        np.minimum.at(self.margin[..., term], (np.asarray(py, np.int64), np.asarray(px, np.int64)), value)

    def resolve(self, fb_c, fb_d):
        """the in-order GL_LESS loop -> (rgba, depth, margin, touched)"""
        vw, vh = self.view
        c, d = np.array(fb_c, np.float64).reshape(vh * vw, 4), np.array(fb_d, np.float64).reshape(vh * vw)
        margin = self.margin.copy().reshape(vh * vw, 4)
        if self.pix:
            prim, pix, z, col = np.concatenate(self.prim), np.concatenate(self.pix), np.concatenate(self.z), np.concatenate(self.col)
            before = d[pix]
            with np.errstate(invalid="ignore"):
                np.minimum.at(margin[:, TEST], pix, np.nan_to_num(np.abs(z - before), nan=0.0))
                ok = z < before                                          # GL_LESS against the depth before the overlay ...
            prim, pix, z, col = prim[ok], pix[ok], z[ok], col[ok]
            order = np.lexsort((prim, z, pix))                           # ... and among the passing ones the first of smallest z stays
            prim, pix, z, col = prim[order], pix[order], z[order], col[order]
            head = np.ones(pix.size, bool)
            head[1:] = pix[1:] != pix[:-1]
            best, wincol = np.full(vh * vw, INF), np.zeros((vh * vw, 4))
            best[pix[head]], wincol[pix[head]] = z[head], col[head]
            other = (col != wincol[pix]).any(-1)
            second = np.full(vh * vw, INF)
            np.minimum.at(second, pix[other], z[other])
            hit = np.isfinite(best)
            margin[hit, ZGAP] = np.minimum(margin[hit, ZGAP], second[hit] - best[hit])
            d[hit], c[hit] = best[hit], wincol[hit]
        touched = self.touched | (self.margin[..., EDGE] < NEAR_MISS) | (self.margin[..., OPEN] == 0.0)
        return c.reshape(vh, vw, 4), d.reshape(vh, vw), margin.reshape(vh, vw, 4), touched


def clip_near_far(a, b):
    """clip-space a -> b against z >= -w and z <= w -> (a', b') or None"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    t0, t1 = 0.0, 1.0
    for da, db in ((a[2] + a[3], b[2] + b[3]), (a[3] - a[2], b[3] - b[2])):
        if not (da >= 0.0) and not (db >= 0.0):
            return None
        if not (da >= 0.0):
            t0 = max(t0, da / (da - db))
        elif not (db >= 0.0):
            t1 = min(t1, da / (da - db))
    if not t0 <= t1:
        return None
    return a + (b - a) * t0, a + (b - a) * t1


def to_window(p, view):
    return np.array([(p[0] / p[3] * 0.5 + 0.5) * view[0], (p[1] / p[3] * 0.5 + 0.5) * view[1], p[2] / p[3] * 0.5 + 0.5])


def _l1_min(ax, ay, bx, by, cx, cy):
    """smallest L1 distance of the segment a -> b to the centres (cx, cy)"""
    dx, dy = bx - ax, by - ay
    ts = [np.zeros_like(cx), np.ones_like(cx)]
    if dx != 0.0:
        ts.append(np.clip((cx - ax) / dx, 0.0, 1.0))
    if dy != 0.0:
        ts.append(np.clip((cy - ay) / dy, 0.0, 1.0))
    return np.minimum.reduce([np.abs(ax + t * dx - cx) + np.abs(ay + t * dy - cy) for t in ts])


def window_line(fr, wa, wb, colour, width=1.0):
    """rasterise the window segment wa -> wb (x, y, z) as one primitive of fr"""
    vw, vh = fr.view
    w = max(int(np.floor(width + 0.5)), 1)
    ax, ay, az = [float(v) for v in wa]
    bx, by, bz = [float(v) for v in wb]
    if not np.isfinite([ax, ay, bx, by, az, bz]).all():
        fr.add([], [], [], colour)
        return
    xmajor = abs(bx - ax) >= abs(by - ay)
    if w > 1:
        if xmajor:
            ay, by = ay - (w - 1) / 2.0, by - (w - 1) / 2.0
        else:
            ax, bx = ax - (w - 1) / 2.0, bx - (w - 1) / 2.0
    lo_x, lo_y = (0, -(w - 1)) if xmajor else (-(w - 1), 0)                       # a base fragment below the view still reaches into it
    x0, x1 = max(int(np.floor(min(ax, bx))) - 1, lo_x), min(int(np.floor(max(ax, bx))) + 1, vw - 1)
    y0, y1 = max(int(np.floor(min(ay, by))) - 1, lo_y), min(int(np.floor(max(ay, by))) + 1, vh - 1)
    rep = np.arange(w)

    def column(px, py):
        """the w pixels of the columns (rows) above the base pixels, those inside the view -> (px, py, index of the base)"""
        k = np.repeat(np.arange(px.size), w)
        qx, qy = (px[k], py[k] + np.tile(rep, px.size)) if xmajor else (px[k] + np.tile(rep, px.size), py[k])
        ok = (qx >= 0) & (qx < vw) & (qy >= 0) & (qy < vh)
        return qx[ok], qy[ok], k[ok]

    # ---- what GL leaves open: the pixels of the two ends, and those where the segment leaves the viewport
    ends = [(ax, ay), (bx, by)]
    dx, dy = bx - ax, by - ay
    for bound, d, a0, o0, do, extent, is_x in ((0.0, dx, ax, ay, dy, vh, True), (float(vw), dx, ax, ay, dy, vh, True),
                                               (0.0, dy, ay, ax, dx, vw, False), (float(vh), dy, ay, ax, dx, vw, False)):
        if d != 0.0:
            t = (bound - a0) / d
            o = o0 + t * do
            if 0.0 < t < 1.0 and -w <= o <= extent + w:
                ends.append((bound, o) if is_x else (o, bound))
    ex = np.array([min(max(int(np.floor(e[0])), lo_x), vw - 1) for e in ends], np.int64)
    ey = np.array([min(max(int(np.floor(e[1])), lo_y), vh - 1) for e in ends], np.int64)
    inside = np.array([(-1.0 <= e[0] <= vw + 1.0) and (-1.0 - w <= e[1] <= vh + 1.0 + w) for e in ends])
    qx, qy, _ = column(ex[inside], ey[inside])
    fr.lower(OPEN, qx, qy, 0.0)
    if x0 > x1 or y0 > y1:
        fr.add([], [], [], colour)
        return
    py, px = [g.ravel() for g in np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")]
    cx, cy = px + 0.5, py + 0.5
    # ---- the diamond-exit rule on the perturbed segment; the margin from the given one
    pax, pay, pbx, pby = ax - TIE, ay - TIE * TIE, bx - TIE, by - TIE * TIE
    hit = _l1_min(pax, pay, pbx, pby, cx, cy) < 0.5
    end_in = (np.abs(pbx - cx) + np.abs(pby - cy)) < 0.5
    frag = hit & ~end_in
    dist = _l1_min(ax, ay, bx, by, cx, cy)
    edge = np.abs(dist - 0.5)
    edge = np.where(dist < 0.5, np.minimum(edge, np.abs(np.abs(bx - cx) + np.abs(by - cy) - 0.5)), edge)
    if w > 1:
        edge = np.where(frag | (edge < NEAR_MISS), np.minimum(edge, abs(abs(dx) - abs(dy))), edge)
    qx, qy, k = column(px, py)
    fr.lower(EDGE, qx, qy, edge[k])
    # ---- eq. 14.5 / 14.6 at the fragment's centre
    len2 = dx * dx + dy * dy
    t = ((cx - ax) * dx + (cy - ay) * dy) / len2 if len2 > 0.0 else np.zeros_like(cx)
    z = az + t * (bz - az)
    fx, fy, k = column(px[frag], py[frag])
    fr.add(fx, fy, z[frag][k], colour)


def clip_line(fr, ca, cb, colour, width=1.0):
    """one GL_LINES segment between clip-space points"""
    r = clip_near_far(ca, cb)
    if r is None or not (r[0][3] > 0.0) or not (r[1][3] > 0.0):
        fr.add([], [], [], colour)
        return
    with np.errstate(over="ignore", invalid="ignore"):
        window_line(fr, to_window(r[0], fr.view), to_window(r[1], fr.view), colour, width)


def clip_points(fr, clip, size, colour, test=None, kept=None, near_test=0.0):
    """GL_POINTS at clip [n][4] in buffer order, one primitive each; colour (4,) or [n][4]; test [n]: a margin of the whole point in its own
    unit (the shader's discard); kept [n]: False = the shader discards every fragment of the point (such a point leaves margins behind only
    if its test margin is below near_test)"""
    vw, vh = fr.view
    clip = np.asarray(clip, np.float64).reshape(-1, 4)
    n = len(clip)
    colour = np.broadcast_to(np.asarray(colour, np.float64), (n, 4))
    kept = np.ones(n, bool) if kept is None else kept
    test = np.full(n, INF) if test is None else test
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ndc = clip[:, :3] / clip[:, 3:4]
        in_clip = (clip[:, 3] > 0.0) & (np.abs(ndc) <= 1.0).all(-1)                      # clipped by its centre
        d_clip = np.nan_to_num(np.abs(1.0 - np.abs(ndc)).min(-1), nan=0.0)
        xw, yw, zw = (ndc[:, 0] * 0.5 + 0.5) * vw, (ndc[:, 1] * 0.5 + 0.5) * vh, ndc[:, 2] * 0.5 + 0.5
    near = (clip[:, 3] > 0.0) & np.isfinite(xw) & np.isfinite(yw) & (in_clip | (d_clip < NEAR_MISS)) & (kept | (test < near_test))
    test = np.minimum(test, d_clip)
    idx = np.flatnonzero(near)
    span = int(np.ceil(size)) + 2                                                         # the square's box and one pixel more on every side
    bx, by = np.ceil(xw[idx] - size * 0.5 - 0.5) - 1.0, np.ceil(yw[idx] - size * 0.5 - 0.5) - 1.0
    half = size * 0.5
    all_px, all_py, all_z, all_col, all_prim = [], [], [], [], []
    for oy in range(span):
        for ox in range(span):
            px, py = (bx + ox).astype(np.int64), (by + oy).astype(np.int64)
            ok = (px >= 0) & (px < vw) & (py >= 0) & (py < vh)
            dx, dy = px + 0.5 - xw[idx], py + 0.5 - yw[idx]
            inx, iny = (dx >= -half) & (dx < half), (dy >= -half) & (dy < half)
            ex, ey = np.minimum(np.abs(dx + half), np.abs(dx - half)), np.minimum(np.abs(dy + half), np.abs(dy - half))
            edge = np.minimum(np.where(iny | (ey < 1.0), ex, INF), np.where(inx | (ex < 1.0), ey, INF))
            fr.lower(EDGE, px[ok], py[ok], edge[ok])
            cover = ok & inx & iny
            fr.lower(TEST, px[cover], py[cover], test[idx][cover])
            fr.touched[py[cover], px[cover]] = True                                       # also of a point that a test rejects by less than its near-miss bound
            drawn = cover & in_clip[idx] & kept[idx]
            all_px.append(px[drawn]); all_py.append(py[drawn]); all_z.append(zw[idx][drawn]); all_col.append(colour[idx][drawn]); all_prim.append(idx[drawn])
    px, py, z, col, prim = [np.concatenate(a) for a in (all_px, all_py, all_z, all_col, all_prim)]
    if px.size:
        fr.prim.append(fr.n_prim + prim)
        fr.pix.append(py * vw + px)
        fr.z.append(np.clip(z, 0.0, 1.0))
        fr.col.append(col)
        fr.touched[py, px] = True
    fr.n_prim += n


def transform(mv, pr, p):
    """gl_ProjectionMatrix * (gl_ModelViewMatrix * (p, 1)) for p [..., 3]"""
    return R._xf(mat(pr) @ mat(mv), np.asarray(p, np.float64))


# ---------------------------------------------------------------------------------------------------------------- "Draw TSDF"
def grid_axis(n):
    """(x + 0.5f) * stepX with float stepX = 1.0f / n (volume_sampler.cpp:14-20): a float product, stored as float"""
    step = np.float32(1.0) / np.float32(n)
    return ((np.arange(n, dtype=np.float32) + np.float32(0.5)) * step).astype(np.float64)


def calib_colour(d):
    """calib_vis.fs:17-30 -> (rgba [n][4], kept [n]); limit is the float 0.01f"""
    inv = np.abs(d) / CALIB_LIMIT
    zero, one = np.zeros_like(d), np.ones_like(d)
    col = np.where((d > 0.0)[:, None], np.stack([1.0 - inv, zero, zero, one], -1), np.stack([zero, 1.0 - inv, zero, one], -1))   # :19-24
    col = np.where((d >= CALIB_LIMIT)[:, None], np.array([0.0, 0.0, 1.0, 1.0]), col)                                            # :26-28
    return col, ~(d <= -CALIB_LIMIT)                                                                                             # :30


def calibvis_samples(volume, gres):
    """calib_vis.vs:25,37 at every grid point, x fastest -> (positions [n][3], d [n], data [n]: the eight taps are equal)"""
    vol = np.asarray(volume, np.float64)
    gz, gy, gx = np.meshgrid(grid_axis(gres[2]), grid_axis(gres[1]), grid_axis(gres[0]), indexing="ij")
    p = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], -1)
    nz, ny, nx = vol.shape
    x0, x1, _ = R._axis(p[:, 0], nx)
    y0, y1, _ = R._axis(p[:, 1], ny)
    z0, z1, _ = R._axis(p[:, 2], nz)
    taps = np.stack([vol[zi, yi, xi] for zi in (z0, z1) for yi in (y0, y1) for xi in (x0, x1)], -1)
    data = (taps == taps[:, :1]).all(-1)
    d = np.where(data, taps[:, 0], tex3d(vol, p))                          # equal taps: the weights sum to one, the sample is the texel
    return p, d, data


def draw_calibvis(volume, gres, bbox_min, bbox_max, mv, pr, view, fb_c, fb_d):
    p, d, data = calibvis_samples(volume, gres)
    world = R._xf(R.vol_to_world(bbox_min, bbox_max), p)[:, :3]            # calib_vis.vs:29
    eye = R._xf(mat(mv), world)[:, :3]                                     # :33
    clip = R._xf(mat(pr), eye)                                             # :38
    col, kept = calib_colour(d)
    with np.errstate(invalid="ignore"):
        test = np.minimum.reduce([np.abs(d + CALIB_LIMIT), np.abs(d), np.abs(d - CALIB_LIMIT)])
    test = np.where(data, INF, np.nan_to_num(test, nan=0.0))
    fr = Frags(view)
    clip_points(fr, clip, 1.0, col, test=test, kept=kept, near_test=NEAR_MISS * CALIB_LIMIT)
    return fr.resolve(fb_c, fb_d)


# ---------------------------------------------------------------------------------------------------------------- "Draw frustums"
def frustum_corners(cv_xyz, res):
    """getCornerPoints (CalibVolumes.cpp:98-113) of a forward volume, texels x fastest: (0,0) (0,ey) (ex,ey) (ex,0) at z = 0, then at ez"""
    v = np.asarray(cv_xyz, np.float64).reshape(int(res[2]), int(res[1]), int(res[0]), 3)
    ez, ey, ex = v.shape[0] - 1, v.shape[1] - 1, v.shape[2] - 1
    ring = ((0, 0), (0, ey), (ex, ey), (ex, 0))
    return np.array([v[0, y, x] for x, y in ring] + [v[ez, y, x] for x, y in ring])


def _closest_point(p, u, q, v):
    """frustum.cpp:97-111: the middle between the closest points of the lines p + s u and q + t v"""
    w0 = p - q
    a, b, c, d, e = u @ u, u @ v, v @ v, u @ w0, v @ w0
    sc, tc = (b * e - c * d) / (a * c - b * b), (a * e - b * d) / (a * c - b * b)
    return ((p + u * sc) + (q + v * tc)) * 0.5


def camera_position(c):
    """Frustum::getCameraPos (frustum.cpp:21-33) of the corners c [8][3]"""
    near, far = c[:4].sum(0) / 4.0, c[4:].sum(0) / 4.0
    return sum(_closest_point(c[i], c[i] - c[i + 4], near, far - near) for i in range(4)) / 4.0


def draw_frustums(corners, mv, pr, view, fb_c, fb_d):
    """corners [n][8][3]: frustum after frustum, its 12 lines and then its camera point (frustum.cpp:45-95)"""
    fr = Frags(view)
    for c in np.asarray(corners, np.float64):
        clip = transform(mv, pr, c)
        for i, j in FRUSTUM_LINES:
            clip_line(fr, clip[i], clip[j], LINE_GREEN)
        clip_points(fr, transform(mv, pr, camera_position(c))[None], 3.0, POINT_RED)
    return fr.resolve(fb_c, fb_d)


# ---------------------------------------------------------------------------------------------------------------- the bounding box
def bbox_segments(bmin, bmax):
    """drawWiredBox (gloostRenderGoodies.h:251-304): front, right, back, left, top, bottom, each a closed loop of four vertices"""
    (x0, y0, z0), (x1, y1, z1) = [[float(np.float32(v)) for v in b] for b in (bmin, bmax)]
    loops = [[(x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)], [(x1, y0, z1), (x1, y0, z0), (x1, y1, z0), (x1, y1, z1)],
             [(x1, y0, z0), (x0, y0, z0), (x0, y1, z0), (x1, y1, z0)], [(x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)],
             [(x0, y1, z1), (x1, y1, z1), (x1, y1, z0), (x0, y1, z0)], [(x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)]]
    return [(lp[k], lp[(k + 1) % 4]) for lp in loops for k in range(4)]


def draw_bbox(bmin, bmax, mv, pr, view, fb_c, fb_d):
    fr = Frags(view)
    for p, q in bbox_segments(bmin, bmax):
        clip_line(fr, transform(mv, pr, p), transform(mv, pr, q), BBOX_WHITE, width=2.0)           # BoundingBox.cpp:310
    return fr.resolve(fb_c, fb_d)


# ---------------------------------------------------------------------------------------------------------------- occupied bricks
def draw_bricks(ids, res_bricks, brick_size, bbox_min, mv, pr, view, fb_c, fb_d):
    """ids: the occupied list in its own order (ascending in the reference, recon_integration.cpp:430-441); brick_size per axis, fp32 data"""
    rx, ry = int(res_bricks[0]), int(res_bricks[1])
    bs = np.array([float(np.float32(v)) for v in brick_size])
    lo = np.array([float(np.float32(v)) for v in bbox_min])
    fr = Frags(view)
    for i in np.asarray(ids, np.int64).reshape(-1):
        z, rem = divmod(int(i), rx * ry)                                                           # inc_bricks.glsl:30-38
        y, x = divmod(rem, rx)
        world = np.array([x, y, z]) * bs + lo + R.CUBE * bs                                        # :22-24
        clip = transform(mv, pr, world)
        for a, b in CUBE_WIRE:
            clip_line(fr, clip[a], clip[b], WIRE_RED)
    return fr.resolve(fb_c, fb_d)


# ---------------------------------------------------------------------------------------------------------------- the texture view
def blit_viewport(w, h):
    """uvec2(fvec2(resolution_full) / 2.0f), resolution_full = uvec2(w * 1.5f, h) (kinect_client.cpp:706, view_lod.cpp:29)"""
    full_x = int(np.float32(w) * np.float32(1.5))
    return int(np.float32(full_x) / np.float32(2.0)), int(np.float32(h) / np.float32(2.0))


def blit(src, view, fb_c, fb_d):
    """TextureBlitter::blit(unit, resolution): the triangle covers every pixel of the viewport (0, 0, vw, vh); noperspective texture
    coordinates are ((x + .5) / vw, (y + .5) / vh); LINEAR (Texture::createDefault); (rgb, 1); no depth test, no depth write"""
    src = np.asarray(src, np.float64)
    sh, sw = src.shape[:2]
    vw, vh = blit_viewport(*view)
    y, x = np.meshgrid(np.arange(vh) + 0.5, np.arange(vw) + 0.5, indexing="ij")
    ndc_x, ndc_y = x / vw * 2.0 - 1.0, y / vh * 2.0 - 1.0                                     # the window transform of the blit's viewport, inverted
    u, v = (ndc_x + 1.0) / 4.0 * 2.0, (ndc_y + 1.0) / 4.0 * 2.0                               # barycentric weight (ndc + 1) / 4 of the vertex with coordinate 2
    assert (u * sw - 0.5 >= 0.0).all() and (u * sw - 0.5 <= sw - 1).all() and (v * sh - 0.5 >= 0.0).all() and (v * sh - 0.5 <= sh - 1).all(), "a tap reaches the wrap mode"
    rgba = np.array(fb_c, np.float64)
    rgba[:vh, :vw, :3] = tex2d_linear(src, u, v)[..., :3]
    rgba[:vh, :vw, 3] = 1.0
    margin = np.full(rgba.shape[:2] + (4,), INF)
    touched = np.zeros(rgba.shape[:2], bool)
    touched[:vh, :vw] = True
    return rgba, np.array(fb_d, np.float64), margin, touched


# ---------------------------------------------------------------------------------------------------------------- the sensor windows
def texel_rgba(type, layer):
    """one layer of NetKinectArray's arrays as texture() returns it: 0 RGB8 / decoded RGBA8 -> (rgb / 255, 1) / rgba / 255; 1 RG32F -> (r, g, 0, 1)
    (or the frame slot's r alone); 2, 5 LUMINANCE32F -> (L, L, L, 1); 3, 6 RGB32F -> (rgb, 1); 4 R32F -> (r, 0, 0, 1)"""
    a = np.asarray(layer)
    out = np.zeros(a.shape[:2] + (4,))
    out[..., 3] = 1.0
    if type == 0:
        out[..., :a.shape[2]] = a.astype(np.float64) / 255.0
    elif type == 1:
        out[..., :2 if a.ndim == 3 else 1] = a[..., :2] if a.ndim == 3 else a[..., None]
    elif type in (2, 5):
        out[..., :3] = a[..., None]
    elif type in (3, 6):
        out[..., :3] = a[..., :3]
    elif type == 4:
        out[..., 0] = a
    else:
        raise ValueError(type)
    return out


def scissor(clip, view):
    """glScissor of imgui_impl_glfw_glb.cpp:123: float arithmetic on the host, (int) casts -> (x, y, w, h); None: the whole view"""
    if clip is None:
        return 0, 0, view[0], view[1]
    x, y, z, w = [np.float32(v) for v in clip]
    return int(x), int(np.float32(view[1]) - w), int(z - x), int(w - y)


def sensor_window(type, layer, rect, clip, fb_c, fb_d):
    """ImGui::Image(p_min, p_max, uv (0,0)-(1,1), white) in array mode: rect = (p_min.x, p_min.y, p_max.x, p_max.y) in ImGui's coordinates"""
    rgba, depth = np.array(fb_c, np.float64), np.array(fb_d, np.float64)
    vh, vw = depth.shape
    x0, y0, x1, y1 = [float(np.float32(v)) for v in rect]
    j, i = np.meshgrid(np.arange(vh), np.arange(vw), indexing="ij")
    wx, py = i + 0.5, vh - (j + 0.5)                                       # imgui_impl_glfw_glb.cpp:79-85: window y = height - p.y
    cover = (wx > x0) & (wx < x1) & (py > y0) & (py < y1)
    edge = np.minimum.reduce([np.abs(wx - x0), np.abs(wx - x1), np.abs(py - y0), np.abs(py - y1)])
    near = (wx > x0 - 1) & (wx < x1 + 1) & (py > y0 - 1) & (py < y1 + 1)
    sx, sy, sw, sh = scissor(clip, (vw, vh))
    box = (i >= sx) & (i < sx + max(sw, 0)) & (j >= sy) & (j < sy + max(sh, 0))
    margin = np.full((vh, vw, 4), INF)
    margin[..., EDGE] = np.where(near & box, edge, INF)
    cover &= box
    u, v = (wx - x0) / (x1 - x0) - 0.5, (py - y0) / (y1 - y0) - 0.5        # Frag_UV, uv -= .5
    ru, rv = ROT_COS * u + ROT_SIN * v + 0.5, -ROT_SIN * u + ROT_COS * v + 0.5   # mat2(c, -s, s, c) * uv: columns (c, -s) and (s, c); uv += .5
    tex = texel_rgba(type, layer)
    th, tw = tex.shape[:2]
    if type in NEAREST_TYPES:
        s = tex2d_nearest(tex, ru, rv)
        margin[..., TEST] = np.where(cover, np.minimum(R.texel_boundary_distance(ru, tw), R.texel_boundary_distance(rv, th)), INF)
    else:
        s = tex2d_linear(tex, ru, rv)
    a = s[..., 3:4]
    with np.errstate(invalid="ignore", over="ignore"):
        mixed = s * a + rgba * (1.0 - a)                                   # SRC_ALPHA, ONE_MINUS_SRC_ALPHA on rgb and alpha alike
    rgba[cover] = mixed[cover]
    return rgba, depth, margin, cover | (margin[..., EDGE] < NEAR_MISS)
