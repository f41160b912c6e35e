"""float64 numpy reference of the three rasterising back-ends: the triangle grid, the points and the draw half of MVT.  HIP-free, and
written from the reference's host code and shaders alone -- not from oracle/tsdf_oracle.cpp, not from the kernels and not from the
rasteriser of tests/mvt_reference.py, whose formulation (edge functions over the window triangle, l_i / w_i weights, whole-triangle
rejection) it does not share:

* vertex buffers  framework/reconstruction/recon_trigrid.cpp:48-61 and recon_mvt.cpp:50-63 (two triangles per cell, cells x < height,
                  y < width: the loop bounds are swapped, and kept), recon_points.cpp:47-54 (one point per depth pixel).  (x + .5) * stepX
                  is a double product with a float stepX, stored as float: the buffer is data.
* trigrid         glsl/trigrid_accum.vs:21-34, trigrid_accum.gs:26-37,40-72, trigrid_accum.fs:39-76 under ReconTrigrid::draw
                  (recon_trigrid.cpp:82-148: pass 0 to the depth buffer with GL_LESS, pass 1 blended ONE / ONE without a depth test,
                  img_to_eye_curr of :84-95 in float64), trigrid_normalize.fs:11-28
* MVT             the same draw (recon_mvt.cpp:84-150) with glsl/mvt_accum.vs:100-115 behind a given bilateral filter result,
                  validSurface of mvt_accum.gs:29-41 and the fragment quality of mvt_accum.fs:53
* points          glsl/points.vs:22-35, points.gs:35-61, points.fs:36-75 under ReconPoints::draw (recon_points.cpp:71-111: GL_LESS, layers
                  in order)
* shared          shading.glsl:5-12,24-30,32-69 (mode 1, Phong, is written here; the camera colours are those of main_path_reference),
                  inc_bbox_test.glsl:11-21

Triangles are rasterised as GL does it: the clip-space triangle is clipped against the near and the far plane (every point with
-w <= z <= w has w >= 0, so this is the clip against w > 0 as well), the remaining polygon goes through the window transform and covers the
pixel centres inside it (edge functions with the top-left rule, main_path_reference._covered).  Window z and the perspective-correct
barycentrics of a pixel come from the UNCLIPPED triangle in homogeneous form: with the columns (x_i, y_i, w_i) of the three clip positions
as a matrix M, b = M^-1 (x_ndc, y_ndc, 1) are the weights of the clip-space point of w = 1 under the pixel; z_ndc = sum b_i z_i (the
triangle's plane) and a smooth varying is sum b_i a_i / sum b_i.  Nothing here divides by a vertex's w: a triangle with vertices behind the
eye needs no special case.

Sampler state as in SURVEY.md Appendix A: depth NEAREST; quality, normals, colours and the LUTs LINEAR; CLAMP_TO_EDGE.

Definitions GL leaves to the implementation are the ones the oracle's header lists, because a reference cannot know better: a point is
clipped by its centre, its size is clamped to [1, 2047] and not rounded (GL_POINT_SPRITE), it covers the pixel centres p with
c - s/2 <= p < c + s/2 per axis, window z is not quantised, gl_NormalMatrix is inverseTranspose(MV).  pow() of a negative base is undefined in
GLSL: such a pixel gets margin 0.

One definition stays open, and is NOT taken from the oracle: whose a pixel centre exactly on the common edge of two triangles is.  GL asks only
that exactly one of them produces the fragment (OpenGL 4.4, 14.6.1).  _covered gives it to a left or a top edge (y up); the oracle and the
kernels to a right or a top edge.  Inside a mesh both produce the pixel once; on the mesh's outline they differ, legitimately, and the edge
margin there is exactly 0 (tests/backend_cases.exact_case compares what GL does fix).

Every draw returns (rgba [h][w][4], depth [h][w], margin [h][w][4]); row 0 is gl_FragCoord.y 0.5; an uncovered pixel is (0, 0, 0, 0) and
depth 1.  The margin says how close the float64 arithmetic came to deciding a pixel otherwise, per TERMS, each in its own unit because the
fp32 error of the operations behind them differs by orders of magnitude:

  edge   pixels: distance of the pixel centre to an edge of a projected (clipped) triangle, or to the boundary of a sprite's square
  test   the operand's own unit: distance to a discard's threshold -- a bbox face (m), 0.01 / 0.99 (texture coordinate), the back-face dot
         product to 0, window z to 0 and 1, an edge length to validSurface's l (LUT units), a point's clip coordinates to +-w (NDC), the
         accumulated alpha to 0
  eps    metres: | |position_curr_es - pos_es| - epsilon | of pass 1
  zgap   window z: the winning point's distance to the runner-up from another point

It is the smallest value over all fragments that touch the pixel, kept or discarded.  Depths are data (NEAREST texels, or MVT's given filter
result): `depth < 0`, `depth <= 0` and `depth < 0.5` compare them exactly in every precision and have no margin; the vertex buffers' coordinates
are texel centres, half a texel from any boundary of the nearest fetch.
"""
import numpy as np

import main_path_reference as R
from main_path_reference import tex2d_linear, tex2d_nearest, tex3d

INF = np.inf
TERMS = ("edge", "test", "eps", "zgap")
EDGE, TEST, EPS, ZGAP = range(4)
EPSILON = float(np.float32(0.075))                      # recon_trigrid.cpp:35, recon_mvt.cpp:37
CV_MIN_D, CV_MAX_D = 0.5, 4.5                           # recon_mvt.cpp:35-36
LIGHT_POSITION = np.array([1.5, 1.0, 1.0])              # shading.glsl:5-8,11-12,22
LIGHT_DIFFUSE = np.array([float(np.float32(v)) for v in (1.0, 0.9, 0.7)])
LIGHT_AMBIENT = LIGHT_DIFFUSE * float(np.float32(0.2))
LIGHT_SPECULAR, KS, SHININESS, SOLID_DIFFUSE = 1.0, 0.5, 20.0, 0.5
NEAR_MISS = 1e-3                                        # a triangle / point rejected by less than this still marks the pixels it would cover


# ---------------------------------------------------------------------------------------------------------------- pieces
def buffer_coords(cells, n):
    """the coordinates (i + 0.5) * step, i = 0 .. cells, of a vertex buffer: float step = 1.0f / n, double product, stored as float"""
    step = np.float32(1.0) / np.float32(n)
    return ((np.arange(cells + 1) + 0.5) * np.float64(step)).astype(np.float32).astype(np.float64)


def _volume(scene, key, l, nc):
    r = [int(v) for v in scene["lut_res"]]
    return np.asarray(scene[key][l], np.float64).reshape(r[2], r[1], r[0], nc)


def _unit(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)


def image_to_eye(proj, view):
    """recon_trigrid.cpp:84-95: inverse(scale(w/2, h/2, 1/2) * translate(1, 1, 1) * projection)"""
    s, t = np.diag([view[0] * 0.5, view[1] * 0.5, 0.5, 1.0]), np.eye(4)
    t[:3, 3] = 1.0
    return np.linalg.inv(s @ t @ R.mat(proj))


def bbox_distance(scene, p):
    """(in_bbox of inc_bbox_test.glsl:11-21, distance to the nearest face)"""
    lo, hi = np.asarray(scene["bbox_min"], np.float64), np.asarray(scene["bbox_max"], np.float64)
    return ((p >= lo) & (p <= hi)).all(-1), np.minimum(np.abs(p - lo), np.abs(p - hi)).min(-1)


def border_distance(tc):
    """(the 0.01 / 0.99 discard of trigrid_accum.fs:46-49 / points.fs:38-41, distance to the nearest of the four thresholds); the literals are
    double constants of the shader rounded to float"""
    lo, hi = float(np.float32(0.01)), float(np.float32(0.99))
    return ((tc > hi) | (tc < lo)).any(-1), np.minimum(np.abs(tc - lo), np.abs(tc - hi)).min(-1)


def phong(pos, normal):
    """shade() in mode 1, shading.glsl:32-52,58-63 -> (rgb, defined): pow() of a negative base is undefined"""
    to_light = _unit(LIGHT_POSITION - pos)                                                           # :33
    angle = (normal * to_light).sum(-1)                                                              # :34
    lit = ~(angle <= 0.0)                                                                            # :36
    half = _unit(to_light + _unit(-pos))                                                             # :42-43
    refl = (half * normal).sum(-1)                                                                   # :44
    with np.errstate(invalid="ignore"):
        spec = np.power(np.where(refl > 0, refl, 0.0), SHININESS)                                    # :45
    a = (1.0 - angle) * (1.0 - angle)                                                                # :48
    spec = np.where(lit, spec * (1.0 - a * a * a), 0.0)                                              # :49
    diff = np.where(lit, np.maximum(angle, 0.0), 0.0)                                                # :40
    rgb = LIGHT_AMBIENT * SOLID_DIFFUSE + LIGHT_DIFFUSE * SOLID_DIFFUSE * diff[..., None] + (LIGHT_SPECULAR * KS * spec)[..., None]
    return rgb, ~(lit & (refl < 0))


def shade(mode, pos_es, normal, colour, mv):
    """shading.glsl:54-69 -> (rgb, defined)"""
    if mode == 0:
        return colour, np.ones(len(colour), bool)
    if mode == 1:
        return phong(pos_es, normal)
    assert mode == 2
    nm = np.linalg.inv(R.mat(mv)).T                                                                  # gl_NormalMatrix as a mat4
    return (np.linalg.inv(nm)[:3, :3] @ normal.T).T, np.ones(len(colour), bool)                      # :66


def rasterise(clip3, view, pad=1):
    """One triangle, clip coordinates [3][4] -> None (nothing near the view) or dict: rows, cols (slices of the view: the window polygon's
    pixel box, padded), covered [..] (pixel centres the clipped triangle owns), edge [..] (distance to the polygon's outline, pixels),
    lam [..][3] (perspective-correct barycentrics in the unclipped triangle, sum 1), z [..] (window z), clipped (the polygon is not the
    triangle)."""
    clip3 = np.asarray(clip3, np.float64)
    poly = R._clip(clip3)
    if len(poly) < 3 or not np.isfinite(poly).all():
        return None
    with np.errstate(invalid="ignore", divide="ignore"):
        win = R._window(poly, view)
    if not np.isfinite(win).all():
        return None
    x0, x1 = max(int(np.floor(win[:, 0].min())) - pad, 0), min(int(np.ceil(win[:, 0].max())) + pad, view[0])
    y0, y1 = max(int(np.floor(win[:, 1].min())) - pad, 0), min(int(np.ceil(win[:, 1].max())) + pad, view[1])
    if x0 >= x1 or y0 >= y1:
        return None
    y, x = np.meshgrid(np.arange(y0, y1) + 0.5, np.arange(x0, x1) + 0.5, indexing="ij")
    covered, _ = R._covered(win, x, y)
    edge = np.full(x.shape, INF)
    for k in range(len(win)):
        edge = np.minimum(edge, R._segment_distance(win[k], win[(k + 1) % len(win)], x, y))
    try:
        minv = np.linalg.inv(clip3[:, [0, 1, 3]].T)
    except np.linalg.LinAlgError:                                   # no area in any projection
        return None
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        b = np.stack([x / view[0] * 2.0 - 1.0, y / view[1] * 2.0 - 1.0, np.ones_like(x)], -1) @ minv.T
        z = (b @ clip3[:, 2]) * 0.5 + 0.5
        lam = b / b.sum(-1, keepdims=True)
    return dict(rows=slice(y0, y1), cols=slice(x0, x1), x0=x0, y0=y0, covered=covered, edge=edge, lam=lam, z=z, clipped=len(poly) != 3 or not (poly == clip3).all())


def accumulate(n_pixels, pix, rgb, q):
    """the ONE / ONE blend of pass 1: sum of (rgb * q, q) per pixel (trigrid_accum.fs:71,74)"""
    acc = np.zeros((n_pixels, 4))
    np.add.at(acc, pix, np.concatenate([rgb * q[:, None], q[:, None]], -1))
    return acc


def normalise(acc, zbuf):
    """trigrid_normalize.fs:11-28: col / col.a and pass 0's depth where col.a > 0, nothing elsewhere"""
    hit = acc[:, 3] > 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        rgba = np.where(hit[:, None], acc / acc[:, 3:4], 0.0)
    return rgba, np.where(hit, zbuf, 1.0)


# ---------------------------------------------------------------------------------------------------------------- triangle grids
def trigrid_vertices(scene, l):
    """trigrid_accum.vs:21-34 at every vertex of the buffer -> dict of [gy][gx] arrays, gx = 0 .. height, gy = 0 .. width"""
    w, h = int(scene["width"]), int(scene["height"])
    u, v = np.meshgrid(buffer_coords(h, w), buffer_coords(w, h))                                      # recon_trigrid.cpp:49-59
    depth = tex2d_nearest(np.asarray(scene["depth"][l])[..., 0], u, v)                                # :24
    at = np.stack([u, v, depth], -1)
    return dict(depth=depth, weight=tex2d_linear(scene["quality"][l], u, v),                          # :31
                pos_cs=tex3d(_volume(scene, "cv_xyz", l, 3), at), tc=tex3d(_volume(scene, "cv_uv", l, 2), at))   # :27,29


def mvt_vertices(scene, vtx, l):
    """mvt_accum.vs:100-115 behind the given bilateral_filter() result vtx [n][width + 1][height + 1][2] = (filtered depth, lateral quality)"""
    w, h = int(scene["width"]), int(scene["height"])
    u, v = np.meshgrid(buffer_coords(h, w), buffer_coords(w, h))                                      # recon_mvt.cpp:51-61
    depth = np.asarray(vtx[l][..., 0], np.float64)
    at = np.stack([u, v, (depth - CV_MIN_D) / (CV_MAX_D - CV_MIN_D)], -1)                             # :106
    return dict(depth=depth, weight=np.asarray(vtx[l][..., 1], np.float64),
                pos_cs=tex3d(_volume(scene, "cv_xyz", l, 3), at), tc=tex3d(_volume(scene, "cv_uv", l, 2), at))


def trigrid_surface(min_length):
    """validSurface of trigrid_accum.gs:26-37 -> (no invalid depth, l)"""
    ml = float(np.float32(min_length))
    return lambda d: (~(d < 0.0).any(-1), ml * (d.sum(-1) / 3.0) * 4.0)


def mvt_surface(min_length):
    """validSurface of mvt_accum.gs:29-41"""
    ml = float(np.float32(min_length))
    return lambda d: (~(d < 0.5).any(-1), ml * (d.sum(-1) / 3.0) + float(np.float32(0.005)))


class GridDraw:
    """Passes 0 of a triangle-grid draw, and everything of pass 1 that does not depend on the shade mode.  resolve(mode) finishes it.
    stats: depth_valid (triangles of three positive depths), accepted (of those, validSurface true), behind (accepted triangles with one or
    two vertices at w <= 0 of which a fragment survives pass 0), fragments."""

    def __init__(self, scene, vertices, surface, mvt, mv, proj, view):
        self.scene, self.view, self.mv, self.mvt = scene, (int(view[0]), int(view[1])), mv, mvt
        vw, vh = self.view
        w, h = int(scene["width"]), int(scene["height"])
        mvm = R.mat(mv)
        pmv = R.mat(proj) @ mvm
        margin = np.full((vh, vw, 4), INF)
        gy, gx = [a.ravel() for a in np.meshgrid(np.arange(w), np.arange(h), indexing="ij")]          # for y < width, for x < height
        corners = [((gy, gx), (gy, gx + 1), (gy + 1, gx)), ((gy, gx + 1), (gy + 1, gx + 1), (gy + 1, gx))]   # recon_trigrid.cpp:53-59
        frag = {k: [] for k in ("pix", "lam", "z", "layer", "tri", "len_margin")}
        tris = {k: [] for k in ("pos_cs", "pos_es", "tc", "weight", "depth", "normal")}
        stats = dict(depth_valid=0, accepted=0, behind=0)
        behind_tris, base = [], 0
        for l in range(int(scene["n"])):
            V = vertices(l)
            T = {k: np.concatenate([np.stack([V[k][c] for c in tri], 1) for tri in corners]) for k in ("depth", "weight", "pos_cs", "tc")}
            T["pos_es"] = R._xf(mvm, T["pos_cs"])[..., :3]
            clip = R._xf(pmv, T["pos_cs"])
            p = T["pos_cs"]
            defined, lim = surface(T["depth"])
            lens = np.stack([np.linalg.norm(p[:, 1] - p[:, 0], axis=-1), np.linalg.norm(p[:, 2] - p[:, 0], axis=-1),
                             np.linalg.norm(p[:, 2] - p[:, 1], axis=-1)], -1)                          # trigrid_accum.gs:46-48
            accepted = defined & (lens < lim[:, None]).all(-1)                                         # :36
            len_margin = np.abs(lens - lim[:, None]).min(-1)
            e = T["pos_es"]
            T["normal"] = _unit(np.cross(e[:, 1] - e[:, 0], e[:, 2] - e[:, 0]))                        # :53-57
            real = (T["depth"] > 0.0).all(-1)
            stats["depth_valid"] += int(real.sum())
            stats["accepted"] += int((real & accepted).sum())
            lo, hi = np.asarray(scene["bbox_min"], np.float64), np.asarray(scene["bbox_max"], np.float64)
            off = ((p < lo - NEAR_MISS).all(1) | (p > hi + NEAR_MISS).all(1)).any(-1)                  # beyond one bbox face: every fragment fails in_bbox
            for a in range(3):                                                                         # beyond one clip plane: no fragment
                off |= (clip[..., a] > clip[..., 3]).all(-1) | (clip[..., a] < -clip[..., 3]).all(-1)
            live = defined & ~off & (accepted | (len_margin < NEAR_MISS))
            for t in np.flatnonzero(live):
                r = rasterise(clip[t], self.view)
                if r is None:
                    continue
                m = margin[r["rows"], r["cols"]]
                m[..., EDGE] = np.minimum(m[..., EDGE], r["edge"])
                ys, xs = np.nonzero(r["covered"])
                if not accepted[t]:
                    m[ys, xs, TEST] = np.minimum(m[ys, xs, TEST], len_margin[t])
                    continue
                if len(ys) == 0:
                    continue
                frag["pix"].append((ys + r["y0"]) * vw + xs + r["x0"])
                frag["lam"].append(r["lam"][ys, xs])
                frag["z"].append(r["z"][ys, xs])
                frag["layer"].append(np.full(len(ys), l))
                frag["tri"].append(np.full(len(ys), base + t))
                frag["len_margin"].append(np.full(len(ys), len_margin[t]))
                if r["clipped"] and (clip[t, :, 3] <= 0).any():
                    behind_tris.append(base + t)
            for k in tris:
                tris[k].append(T[k])
            base += len(lens)
        self.stats = stats
        F = {k: (np.concatenate(v) if v else np.zeros((0, 3) if k == "lam" else 0, np.float64 if k in ("lam", "z", "len_margin") else np.int64)) for k, v in frag.items()}
        TA = {k: np.concatenate(v) for k, v in tris.items()}
        lam, tri = F["lam"], F["tri"]
        ip = lambda k: (TA[k][tri] * (lam[..., None] if TA[k].ndim == 3 else lam)).sum(1)             # smooth varyings
        self.pix, self.layer, self.z = F["pix"], F["layer"], F["z"]
        self.pos_es, self.tc = ip("pos_es"), ip("tc")
        pos_cs = ip("pos_cs")
        with np.errstate(invalid="ignore", divide="ignore"):
            self.weight = ip("weight") / ip("depth") if mvt else ip("weight")                         # mvt_accum.fs:53 / trigrid_accum.fs:56
        inside, d_box = bbox_distance(scene, pos_cs)                                                  # trigrid_accum.fs:41-43
        border, d_border = border_distance(self.tc)                                                   # :46-49
        self.normal = -_unit(TA["normal"][tri])                                                       # :51
        facing = (self.normal * _unit(self.pos_es)).sum(-1)                                           # :53
        kept = inside & ~border & ~(facing > 0.0)
        test = np.minimum.reduce([d_box, d_border, np.abs(facing), self.z, 1.0 - self.z, F["len_margin"]]) if len(tri) else np.zeros(0)
        test = np.where(np.isnan(test), 0.0, test)
        flat = margin.reshape(-1, 4)
        np.minimum.at(flat[:, TEST], self.pix, test)
        zbuf = np.ones(vw * vh)
        np.minimum.at(zbuf, self.pix[kept], self.z[kept])                                             # pass 0: GL_LESS over the cleared 1
        x, y = (self.pix % vw) + 0.5, (self.pix // vw) + 0.5
        cur = np.stack([x + 0.5, y + 0.5, zbuf[self.pix], np.ones(len(x))], -1) @ image_to_eye(proj, self.view).T   # :59-62, the + 0.5 is the shader's
        with np.errstate(invalid="ignore", divide="ignore"):
            dist = np.linalg.norm(cur[:, :3] / cur[:, 3:4] - self.pos_es, axis=-1)
        np.minimum.at(flat[:, EPS], self.pix[kept], np.nan_to_num(np.abs(dist - EPSILON)[kept], nan=0.0))
        self.kept = kept & ~(EPSILON < dist)                                                          # :64
        self.zbuf, self.margin = zbuf, margin
        seen = set(tri[self.kept & np.isin(tri, behind_tris)].tolist()) if behind_tris else set()
        stats["behind"] = len(seen)
        stats["fragments"] = int(self.kept.sum())

    def resolve(self, mode):
        k = self.kept
        vw, vh = self.view
        margin = self.margin.copy()
        if mode == 3:
            rgb = R.CAMERA_COLORS[self.layer[k]]                                                      # trigrid_accum.fs:70-71
        else:
            colour = np.zeros((int(k.sum()), 3))
            for l in np.unique(self.layer[k]):
                s = self.layer[k] == l
                colour[s] = tex2d_linear(np.asarray(self.scene["color"][l], np.float64) / 255.0, self.tc[k][s, 0], self.tc[k][s, 1])   # :69
            rgb, defined = shade(mode, self.pos_es[k], self.normal[k], colour, self.mv)               # :74
            np.minimum.at(margin.reshape(-1, 4)[:, TEST], self.pix[k][~defined], 0.0)
        acc = accumulate(vw * vh, self.pix[k], rgb, self.weight[k])
        rgba, depth = normalise(acc, self.zbuf)
        touched = np.zeros(vw * vh, bool)
        touched[self.pix[k]] = True
        m = margin.reshape(-1, 4)
        m[:, TEST] = np.where(touched, np.minimum(m[:, TEST], np.nan_to_num(np.abs(acc[:, 3]), nan=0.0)), m[:, TEST])   # col.a > 0.0
        return rgba.reshape(vh, vw, 4), depth.reshape(vh, vw), margin


def trigrid(scene, mv, proj, view, min_length):
    return GridDraw(scene, lambda l: trigrid_vertices(scene, l), trigrid_surface(min_length), False, mv, proj, view)


def draw_trigrid(scene, mv, proj, view, min_length, mode):
    """ReconTrigrid::draw -> (rgba, depth, margin); modes 0, 1, 3"""
    return trigrid(scene, mv, proj, view, min_length).resolve(mode)


def mvt_raster(scene, vtx, mv, proj, view, min_length):
    return GridDraw(scene, lambda l: mvt_vertices(scene, vtx, l), mvt_surface(min_length), True, mv, proj, view)


def draw_mvt_raster(scene, vtx, mv, proj, view, min_length, mode):
    """ReconMVT::draw behind its vertex stage's bilateral filter (vtx: its result per vertex) -> (rgba, depth, margin)"""
    return mvt_raster(scene, vtx, mv, proj, view, min_length).resolve(mode)


# ---------------------------------------------------------------------------------------------------------------- points
def sprite_pixels(xw, yw, size, view):
    """the pixel box [x0, x1) x [y0, y1) of the centres p with c - s/2 <= p < c + s/2, cut to the view"""
    lo = lambda c: int(np.ceil(c - size * 0.5 - 0.5))                      # the first i with i + 0.5 >= c - s/2
    x0, x1, y0, y1 = lo(xw), lo(xw + size), lo(yw), lo(yw + size)          # the first i with i + 0.5 >= c + s/2 ends the run
    return max(x0, 0), min(x1, view[0]), max(y0, 0), min(y1, view[1])


def draw_points(scene, normals, mv, proj, view, mode, stats=None):
    """ReconPoints::draw -> (rgba, depth, margin); modes 0 to 3.  stats (a dict, filled): drawn, largest (sprite size, pixels), centre_dropped
    (points clipped by their centre in x or y whose square would have reached into the view)."""
    vw, vh = int(view[0]), int(view[1])
    w, h = int(scene["width"]), int(scene["height"])
    mvm = R.mat(mv)
    pmv = R.mat(proj) @ mvm
    margin = np.full((vh, vw, 4), INF)
    best = np.ones((vh, vw))                                               # the depth buffer, cleared to 1
    second = np.full((vh, vw), INF)                                        # the nearest loser from another point
    owner = np.full((vh, vw), -1, np.int64)
    max_size = 4.0 if mode == 3 else 10.0                                  # points.gs:53-57
    u, v = np.meshgrid(buffer_coords(w - 1, w), buffer_coords(h - 1, h))   # recon_points.cpp:50-54
    P = {k: [] for k in ("pos_es", "tc", "layer", "uv")}
    st = dict(drawn=0, largest=0.0, centre_dropped=0)
    n_pts = 0
    for l in range(int(scene["n"])):                                       # recon_points.cpp:105-109
        depth = tex2d_nearest(np.asarray(scene["depth"][l])[..., 0], u, v)                            # points.vs:25
        at = np.stack([u, v, depth], -1)
        pos_cs = tex3d(_volume(scene, "cv_xyz", l, 3), at)                                            # :28
        tc = tex3d(_volume(scene, "cv_uv", l, 2), at)                                                 # :30
        pos_es = R._xf(mvm, pos_cs)[..., :3]
        clip = R._xf(pmv, pos_cs)
        inside, d_box = bbox_distance(scene, pos_cs)                                                  # points.gs:37
        border, d_border = border_distance(tc)                                                        # points.fs:38-41: flat, so the whole point
        with np.errstate(invalid="ignore", divide="ignore"):
            ndc = clip[..., :3] / clip[..., 3:4]
            in_clip = (clip[..., 3:4] > 0).all(-1) & (np.abs(ndc) <= 1.0).all(-1)                     # clipped by its centre
            d_clip = np.abs(1.0 - np.abs(ndc)).min(-1)
            xw, yw, zw = (ndc[..., 0] * 0.5 + 0.5) * vw, (ndc[..., 1] * 0.5 + 0.5) * vh, ndc[..., 2] * 0.5 + 0.5
            size = np.clip(max_size / np.linalg.norm(pos_es, axis=-1), 1.0, 2047.0)                   # points.gs:51,58 and the point size range
        emitted = inside & ~(depth <= 0.0) & ~border                                                  # points.gs:37
        test = np.nan_to_num(np.minimum.reduce([d_box, d_border, d_clip, np.abs(1.0 - zw)]), nan=0.0)
        drawn = emitted & in_clip & (zw < 1.0)                                                        # GL_LESS against the cleared 1
        ahead = emitted & ~in_clip & (clip[..., 3] > 0) & (np.abs(ndc[..., 2]) <= 1.0)
        for y, x in zip(*np.nonzero(ahead)):
            x0, x1, y0, y1 = sprite_pixels(xw[y, x], yw[y, x], size[y, x], (vw, vh))
            st["centre_dropped"] += int(x0 < x1 and y0 < y1)
        for y, x in zip(*np.nonzero(emitted & (drawn | (test < NEAR_MISS)))):                         # row-major: the buffer's order
            cx, cy, s = xw[y, x], yw[y, x], size[y, x]
            if not (np.isfinite(cx) and np.isfinite(cy)):
                continue
            x0, x1, y0, y1 = sprite_pixels(cx - 1.0, cy - 1.0, s + 2.0, (vw, vh))                     # one pixel more on every side for the margin
            if x0 >= x1 or y0 >= y1:
                continue
            px, py = np.arange(x0, x1) + 0.5, np.arange(y0, y1) + 0.5
            dx, dy = px - cx, py - cy
            inx, iny = (dx >= -s * 0.5) & (dx < s * 0.5), (dy >= -s * 0.5) & (dy < s * 0.5)
            cover = iny[:, None] & inx[None, :]
            m = margin[y0:y1, x0:x1]
            ex, ey = np.minimum(np.abs(dx + s * 0.5), np.abs(dx - s * 0.5)), np.minimum(np.abs(dy + s * 0.5), np.abs(dy - s * 0.5))
            near_x, near_y = np.where(iny[:, None] | (ey[:, None] < 1.0), ex[None, :], INF), np.where(inx[None, :] | (ex[None, :] < 1.0), ey[:, None], INF)
            m[..., EDGE] = np.minimum(m[..., EDGE], np.minimum(near_x, near_y))
            m[..., TEST] = np.where(cover, np.minimum(m[..., TEST], test[y, x]), m[..., TEST])
            if not drawn[y, x]:
                continue
            st["drawn"] += 1
            st["largest"] = max(st["largest"], float(s))
            z = zw[y, x]
            b, s2, o = best[y0:y1, x0:x1], second[y0:y1, x0:x1], owner[y0:y1, x0:x1]
            wins = cover & (z < b)                                                                    # GL_LESS: the earlier of two equal points stays
            s2[...] = np.where(wins, np.where(o >= 0, b, INF), np.where(cover & (z < s2), z, s2))
            b[...] = np.where(wins, z, b)
            o[...] = np.where(wins, n_pts + y * w + x, o)
        for k, val in (("pos_es", pos_es), ("tc", tc), ("layer", np.full(u.shape, l)), ("uv", np.stack([u, v], -1))):
            P[k].append(val.reshape(w * h, -1))
        n_pts += w * h
    if stats is not None:
        stats.update(st)
    P = {k: np.concatenate(val) for k, val in P.items()}
    hit = owner >= 0
    ids = owner[hit]
    margin[..., ZGAP] = np.where(hit, second - best, INF)
    layer = P["layer"][ids, 0].astype(np.int64)
    if mode == 3:
        rgb = R.CAMERA_COLORS[layer]                                                                  # points.fs:70-71
    else:
        colour, normal = np.zeros((len(ids), 3)), np.zeros((len(ids), 3))
        for l in np.unique(layer):
            s = layer == l
            colour[s] = tex2d_linear(np.asarray(scene["color"][l], np.float64) / 255.0, P["tc"][ids[s], 0], P["tc"][ids[s], 1])      # :66
            normal[s] = tex2d_linear(np.asarray(normals[l], np.float64), P["uv"][ids[s], 0], P["uv"][ids[s], 1])                     # :67
        view_normal = normal @ np.linalg.inv(mvm)[:3, :3]                                             # :68: inverseTranspose(MV) * (normal, 0)
        rgb, defined = shade(mode, P["pos_es"][ids], view_normal, colour, mv)                         # :74
        t = margin[..., TEST]
        t[hit] = np.where(defined, t[hit], 0.0)
    rgba = np.zeros((vh, vw, 4))
    rgba[hit] = np.concatenate([rgb, np.ones((len(ids), 1))], -1)
    return rgba, np.where(hit, best, 1.0), margin
