"""float64 numpy reference of the pre-processing passes (NetKinectArray::processTextures).  HIP-free, and written from the reference's
shaders and driver alone -- not from oracle/tsdf_oracle.cpp and not from the kernels, whose tiling, tap order and helpers it does not share:

* morph      glsl/pre_morph.fs:73-112 (dilate; in_bbox of :44-50 returns true before it looks at the box) under processDepth,
             framework/NetKinectArray.cpp:249-288: mode 0 reads the raw array, mode 1 only copies (:130-135)
* filter     glsl/pre_depth.fs:51-154 with inc_bbox_test.glsl:11-21; it reads depth2 when processed_depth is set and the raw array
             otherwise (NetKinectArray.cpp:285-287,317-318), per stream cv_min_ds / cv_max_ds and the compression uniforms of :337-349
* rgb_to_lab glsl/inc_color.glsl:8-47, with the colour fetch of pre_depth.fs:81-84,136
* boundary   glsl/pre_boundary.fs:27-55,86-117 over the filter's two outputs (NetKinectArray.cpp:364, :459)
* normal     glsl/pre_normal.fs:22-56 over depth_b (NetKinectArray.cpp:377) with mark_brick, glsl/inc_bricks.glsl:22-28,40-58
* quality    glsl/pre_quality.fs:39-48,65-119 over depth_b and the normals (NetKinectArray.cpp:377,443-444)

Sampler state (NetKinectArray.cpp:180-188 and the globjects default): NEAREST for the raw array, depth2, depth (RG) and depth_b; LINEAR for
the Lab image, the normals, the colours and the LUTs; CLAMP_TO_EDGE everywhere.  pass_TexCoord is the pixel centre (x + .5) / w, so a
LINEAR fetch at a pixel centre or a whole number of texels off it is a texel up to the last bit; it is evaluated as a LINEAR fetch all the
same (main_path_reference.tex2d_linear), and a tap past the border is the clamped border texel on either filter.

One function per pass and stream.  Each takes that pass's fp32 inputs as they are and returns the product plus a per-pixel *decision
margin*: how close the pixel came to deciding otherwise.  GLSL literals are fp32 constants (F below): where an fp32 input is compared
against one the decision is exact and has no margin; everything computed is float64.

What GLSL leaves open gets margin 0, so no implementation is held to a choice: normalize() of a zero vector (pre_normal.fs:55), pow() of a
negative base (pre_quality.fs:114), a division by a zero weight sum (pre_depth.fs:124), uvec3() of a negative float (inc_bricks.glsl:41),
a NaN that reaches a comparison and a NaN texel next to a LINEAR fetch at a pixel centre (weight 0).

The reference's Bricks buffer holds one float brick_size (inc_bricks.glsl:11); this project lets it differ per axis, so `brick_size * 0.1`
of inc_bricks.glsl:52, which is compared with d_abs.x, is read as the x size.
"""
import numpy as np

from main_path_reference import tex3d, tex2d_linear, nearest_index, texel_boundary_distance, INF


def F(x):
    """a GLSL literal: the fp32 constant, as a float64"""
    return float(np.float32(x))


def tex_coords(h, w):
    """pass_TexCoord of the full-screen pass and texSizeInv (an fp32 uniform, NetKinectArray.cpp:195): v [h], u [w], (tx, ty)"""
    return (np.arange(h) + 0.5) / h, (np.arange(w) + 0.5) / w, (float(np.float32(1.0) / np.float32(w)), float(np.float32(1.0) / np.float32(h)))


class Taps:
    """NEAREST + CLAMP_TO_EDGE fetches at pass_TexCoord + (dx, dy) * texSizeInv of an [h][w(, c)] image"""

    def __init__(self, h, w):
        self.h, self.w = h, w
        self.v, self.u, (self.tx, self.ty) = tex_coords(h, w)

    def __call__(self, img, dx, dy):
        yi = nearest_index(self.v + dy * self.ty, self.h)
        xi = nearest_index(self.u + dx * self.tx, self.w)
        return img[yi[:, None], xi[None, :]]

    def boundary(self, reach):
        """[h][w]: the smallest distance, in texels, of any fetch within `reach` taps to the texel boundary at which it would pick another texel"""
        by = np.min([texel_boundary_distance(self.v + d * self.ty, self.h) for d in range(-reach, reach + 1)], 0)
        bx = np.min([texel_boundary_distance(self.u + d * self.tx, self.w) for d in range(-reach, reach + 1)], 0)
        return np.minimum(by[:, None], bx[None, :])


def lut(volume, res, nc):
    """a LUT of scene['cv_xyz'][i] / ['cv_uv'][i] as [z][y][x][c] float64"""
    r = [int(x) for x in res]
    return np.asarray(volume, np.float64).reshape(r[2], r[1], r[0], nc)


def grid_uv(h, w):
    v, u, _ = tex_coords(h, w)
    return np.broadcast_to(u[None, :], (h, w)), np.broadcast_to(v[:, None], (h, w))


# ---------------------------------------------------------------------------------------------------------------- morph
def morph(raw):
    """raw [h][w] fp32 -> (depth2 [h][w], margin).  pre_morph.fs:73-112 with kernel_size 1; is_valid :36-39 is exact on fp32 inputs."""
    raw32 = np.asarray(raw, np.float32)
    h, w = raw32.shape
    t = Taps(h, w)
    with np.errstate(invalid="ignore"):
        ok32 = (raw32 > np.float32(0.5)) & (raw32 < np.float32(4.5))                        # :38
    d = np.where(ok32, raw32.astype(np.float64), 0.0)
    offs = [(x, y) for y in (-1, 0, 1) for x in (-1, 0, 1)]
    tap = np.stack([t(d, x, y) for x, y in offs])                                           # invalid taps read 0 here and are masked by ...
    val = np.stack([t(ok32, x, y) for x, y in offs])                                        # ... is_valid of the tap
    n1 = val.sum(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        avg = np.where(val, tap, 0.0).sum(0) / n1                                           # :81-93
        dist = np.abs(avg[None] - tap)
        near = val & (dist < F(0.2))                                                        # :102, max_dist :54
        n2 = near.sum(0)
        new = np.where(near, tap, 0.0).sum(0) / n2                                          # :104-111
    out = np.where(n1 == 0, 0.0, np.where(n2 == 0, 0.0, new))                               # :92, :110
    out = np.where(ok32, raw32.astype(np.float64), out)                                     # :75-77
    with np.errstate(invalid="ignore"):
        m = np.where(val, np.abs(dist - F(0.2)), INF).min(0)
    margin = np.where(ok32 | (n1 == 0), INF, np.minimum(m, t.boundary(1)))
    return out, margin


# ---------------------------------------------------------------------------------------------------------------- colour
def pivot_rgb(n):
    """inc_color.glsl:8-10"""
    n = np.asarray(n, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(n > F(0.04045), np.power(np.maximum((n + F(0.055)) / F(1.055), 0.0), F(2.4)), n / F(12.92)) * 100.0


def pivot_xyz(n):
    """inc_color.glsl:27-29"""
    n = np.asarray(n, np.float64)
    return np.where(n > F(0.008856), np.power(np.maximum(n, 0.0), F(1.0) / F(3.0)), (F(903.3) * n + 16.0) / 116.0)


def rgb_to_lab(rgb):
    """rgb [..., 3]: what texture() returned, 8-bit colours already in [0, 1]; the shader divides by 255 once more (inc_color.glsl:14-16)"""
    rgb = np.asarray(rgb, np.float64)
    r, g, b = (pivot_rgb(rgb[..., k] / 255.0) for k in range(3))
    x = r * F(0.4124) + g * F(0.3576) + b * F(0.1805)                                       # :20-22
    y = r * F(0.2126) + g * F(0.7152) + b * F(0.0722)
    z = r * F(0.0193) + g * F(0.1192) + b * F(0.9505)
    x, y, z = pivot_xyz(x / F(95.047)), pivot_xyz(y / F(100.0)), pivot_xyz(z / F(108.883))  # :4, :32-34
    return np.stack([np.maximum(0.0, 116.0 * y - 16.0), 500.0 * (x - y), 200.0 * (y - z)], -1)   # :38-40


def lab_decisions(rgb):
    """distance of the two pivots' arguments to their thresholds, [...]: how close rgb_to_lab came to its other branch"""
    rgb = np.asarray(rgb, np.float64)
    n = rgb / 255.0
    lin = pivot_rgb(n)
    xyz = np.stack([lin @ np.array([F(0.4124), F(0.3576), F(0.1805)]) / F(95.047), lin @ np.array([F(0.2126), F(0.7152), F(0.0722)]) / F(100.0),
                    lin @ np.array([F(0.0193), F(0.1192), F(0.9505)]) / F(108.883)], -1)
    return np.minimum(np.abs(n - F(0.04045)).min(-1), np.abs(xyz - F(0.008856)).min(-1))


# ---------------------------------------------------------------------------------------------------------------- filter
def uncompress(code, near, far):
    """pre_depth.fs:51-61 with the uniforms of NetKinectArray.cpp:344-349 (fp32 arithmetic of the driver).  -> (metres, margin of `d_c < scaled_near`:
    exact on an fp32 input, so INF)"""
    near32, far32 = np.float32(near), np.float32(far)
    scale = np.float32(far32 - near32)
    scaled_near = np.float32(scale / np.float32(255.0))
    c32 = np.asarray(code, np.float32)
    c = c32.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(c32 < scaled_near, 0.0, (c * c + F(0.15) * float(scaled_near)) * float(scale) + float(near32))


def filter_pass(depth_in, colour, cv_xyz, cv_uv, bbox_min, bbox_max, limits, filter_textures=True, compression=None):
    """depth_in [h][w] fp32: depth2 or the raw array; colour [ch][cw][3] uint8; cv_xyz / cv_uv from lut(); limits = (cv_min_ds, cv_max_ds);
    compression = (near, far) of a compressed stream or None.  -> (depth_rg [h][w][2], lab [h][w][3], margins {"depth_rg", "lab"})."""
    d32 = np.asarray(depth_in, np.float32)
    h, w = d32.shape
    t = Taps(h, w)
    lo, hi = float(np.float32(limits[0])), float(np.float32(limits[1]))
    with np.errstate(invalid="ignore"):
        d = d32.astype(np.float64) if compression is None else uncompress(d32, *compression)   # sample(), :63-72
    u, v = grid_uv(h, w)
    dn = (d - lo) / (hi - lo)                                                               # :78-80, :132
    world = tex3d(cv_xyz, np.stack([u, v, dn], -1))                                         # :133
    bmin, bmax = np.asarray(bbox_min, np.float32).astype(np.float64), np.asarray(bbox_max, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        inbox = ((world >= bmin) & (world <= bmax)).all(-1)                                 # inc_bbox_test.glsl:11-21
        face = np.minimum(np.abs(world - bmin), np.abs(world - bmax)).min(-1)
        sl = np.where((dn <= 0.0) | (dn >= 1.0), 1.0, dn)                                   # :136
    cc = tex3d(cv_uv, np.stack([u, v, sl], -1))                                             # get_color, :81-84
    rgb = tex2d_linear(np.asarray(colour, np.float64) / 255.0, cc[..., 0], cc[..., 1])      # GL_RGB8, LINEAR
    lab = rgb_to_lab(rgb)
    m_lab = np.minimum(np.minimum(np.abs(dn), np.abs(dn - 1.0)), lab_decisions(rgb))
    m_lab = np.where(np.isnan(dn), 0.0, m_lab)
    tb = t.boundary(6) if filter_textures else t.boundary(0)
    out = np.zeros((h, w, 2))
    margin = np.minimum(face, tb)
    if not filter_textures:
        out[..., 0], out[..., 1] = dn, 1.0                                                  # :148-150
    else:
        drm = F(0.35) * (d / F(4.5))                                                        # :89-92
        with np.errstate(invalid="ignore", divide="ignore"):
            inv = 1.0 / drm
        bf = np.zeros((h, w)); wsum = np.zeros((h, w)); wr = np.zeros((h, w)); mt = np.full((h, w), INF)
        for y in range(-6, 7):
            for x in range(-6, 7):
                ds = t(d, x, y)
                with np.errstate(invalid="ignore"):
                    rng = np.abs(ds - d)                                                    # :109
                    outside = (ds < lo) | (ds > hi)                                         # is_outside, :74-76
                    border = outside | (rng > drm)                                          # :110
                    mt = np.minimum(mt, np.where(outside, INF, np.abs(rng - drm)))
                    if compression is not None:                                             # a computed depth against cv_min_ds / cv_max_ds (metres)
                        mt = np.minimum(mt, np.minimum(np.abs(ds - lo), np.abs(ds - hi)))
                    gs = 1.0 - np.hypot(x, y) * (1.0 / 6.0)                                 # computeGaussSpace, :37-41
                    gr = 1.0 - np.minimum(rng, drm) * inv                                   # computeGaussRange, :45-48
                    ws = np.where(border, 0.0, gs * gr)
                    bf += np.where(border, 0.0, ws * ds)
                    wsum += ws
                    wr += np.where(border, 0.0, gr)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[..., 0] = (bf / wsum - lo) / (hi - lo)                                      # :124-126
        out[..., 1] = wr / 169.0
        margin = np.minimum(margin, mt)
        margin = np.where(inbox & (np.abs(wsum) < 1e-12), 0.0, margin)                      # x / 0
    out[~inbox] = 0.0                                                                       # :143-146
    margin = np.where(np.isnan(world).any(-1) | np.isnan(d), 0.0, margin)
    return out, lab, dict(depth_rg=margin, lab=m_lab)


# ---------------------------------------------------------------------------------------------------------------- boundary
def boundary(depth_rg, lab, refine=True):
    """depth_rg [h][w][2] fp32 (the filter's product), lab [h][w][3] -> (depth_b [h][w][2], silhouette [h][w], margin, info).
    pre_boundary.fs:86-117; `> 0.0f`, `> min_range` (:27-30) and the count against total_samples * 0.5 = 8 (:23, :53) are exact.
    info: {"candidates", "counted" [h][w] number of valid taps, "colour_dist" [h][w]}"""
    rg = np.asarray(depth_rg, np.float32)
    h, w = rg.shape[:2]
    t = Taps(h, w)
    x32, y32 = rg[..., 0], rg[..., 1]
    with np.errstate(invalid="ignore"):
        outside = x32 <= np.float32(0.0)                                                    # :90
        good = y32 > np.float32(0.65)                                                       # valid_range, :27-30
        tapok = (x32 > np.float32(0.0)) & good                                              # :45
    cand = ~outside & ~good                                                                 # :102
    lab = np.asarray(lab, np.float64)
    dist = np.zeros((h, w)); num = np.zeros((h, w))
    ys, xs = np.nonzero(cand)
    if ys.size:
        v, u = t.v[ys], t.u[xs]
        centre = tex2d_linear(lab, u, v)                                                    # :38
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                us, vs = u + dx * t.tx, v + dy * t.ty                                       # :43
                ok = tapok[nearest_index(vs, h), nearest_index(us, w)]                      # :44-45
                cs = tex2d_linear(lab, us, vs)                                              # :47
                dd = np.sqrt(((centre - cs) ** 2).sum(-1))
                dist[ys, xs] += np.where(ok, dd, 0.0)
                num[ys, xs] += ok
    with np.errstate(invalid="ignore", divide="ignore"):
        cdist = np.where(num < 8.0, 1.0, dist / num)                                        # :53-54
    reject = cand & ((cdist > F(0.5)) | (not refine))                                       # :105
    out = np.zeros((h, w, 2))
    out[..., 0] = np.where(reject, -1.0, x32.astype(np.float64))
    out[..., 1] = np.where(outside, 0.0, np.where(cand, np.where(reject, F(0.1), 1.0), 0.0))     # :97, :107, :111, :115
    sil = np.where(~outside & good, 1.0, 0.0)                                               # :88, :98, :103, :108
    margin = np.full((h, w), INF)
    if refine:
        margin = np.where(cand & (num >= 8.0), np.abs(cdist - F(0.5)), margin)
    margin = np.where(cand, np.minimum(margin, t.boundary(2)), margin)
    margin = np.where(np.isnan(rg).any(-1), 0.0, margin)
    return out, sil, margin, dict(candidates=cand, counted=num, colour_dist=np.where(cand, cdist, 0.0))


# ---------------------------------------------------------------------------------------------------------------- normal + mark_brick
def mark_brick(pos, bbox_min, brick_size, res_bricks):
    """pos [n][3] -> (main id [n], neighbour id [n], neighbour increment [n] in {0, 1}, margin [n]).  inc_bricks.glsl:40-58.
    margin: distance to the next brick face (world units), to the 0.1 * brick_size test of :52 and between the two largest |difference|."""
    bs = np.asarray(brick_size, np.float32).astype(np.float64)
    lo = np.asarray(bbox_min, np.float32).astype(np.float64)
    res = np.asarray(res_bricks, np.int64)
    rel = (pos - lo) / bs
    fl = np.floor(rel)                                                                      # :41
    bad = np.isnan(rel).any(-1) | (fl < 0).any(-1) | (fl >= res).any(-1)                    # uvec3() of a negative float; an id past the buffer
    idx = np.clip(np.nan_to_num(fl), 0, res - 1).astype(np.int64)
    centre = idx * bs + lo + 0.5 * bs                                                       # to_world(vec3(0.5), index), :22-24, :42
    diff = pos - centre
    dabs = np.abs(diff)
    mx = dabs.max(-1)                                                                       # :45 (named min_v)
    mc = ~(dabs < mx[:, None])                                                              # :46-49
    off = np.sign(diff * mc).astype(np.int64)                                               # :50
    nb = np.clip(idx + off, 0, res - 1)                                                     # :52
    gid = lambda i: (i[:, 2] * res[1] + i[:, 1]) * res[0] + i[:, 0]                         # :26-28
    inc = (dabs[:, 0] > bs[0] * F(0.1)).astype(np.int64)
    srt = np.sort(dabs, -1)
    face = (np.minimum(rel - fl, fl + 1.0 - rel) * bs).min(-1)
    margin = np.minimum(np.minimum(face, np.abs(dabs[:, 0] - bs[0] * F(0.1))), srt[:, 2] - srt[:, 1])
    return gid(idx), gid(nb), inc, np.where(bad, 0.0, margin)


def normal_pass(depth_b, cv_xyz, bbox_min, brick_size, res_bricks):
    """depth_b [h][w][2] fp32 -> (normals [h][w][3], margin [h][w], marks).  pre_normal.fs:26-56; is_outside :22-24 is exact on fp32 inputs.
    marks: {"pixel" [n] flat pixel index, "main", "neighbour", "add", "margin"} of the pixels that call mark_brick"""
    d32 = np.asarray(depth_b, np.float32)[..., 0]
    h, w = d32.shape
    t = Taps(h, w)
    with np.errstate(invalid="ignore"):
        out32 = ~((d32 > np.float32(0.0)) & (d32 < np.float32(1.0)))                        # :22-24 (a NaN counts as outside here and gets margin 0)
    d = d32.astype(np.float64)
    u, v = grid_uv(h, w)
    world = tex3d(cv_xyz, np.stack([u, v, d], -1))                                          # :32
    ws = {}
    for k, (dx, dy) in dict(t=(0, 1), b=(0, -1), l=(-1, 0), r=(1, 0)).items():              # :35-38
        dk = np.where(t(out32, dx, dy), d, t(d, dx, dy))                                    # :40-48
        ws[k] = tex3d(cv_xyz, np.stack([u + dx * t.tx, v + dy * t.ty, dk], -1))             # :50-53
    c = np.cross(ws["b"] - ws["t"], ws["l"] - ws["r"])                                      # :55
    ln = np.sqrt((c * c).sum(-1))
    with np.errstate(invalid="ignore", divide="ignore"):
        n = c / ln[..., None]
    n = np.where(out32[..., None], 0.0, n)                                                  # :28-30
    margin = np.where(out32, INF, np.minimum(ln, t.boundary(1)))                            # |cross|: how far from normalize(0)
    margin = np.where(np.isnan(d32), 0.0, margin)
    px = np.flatnonzero(~out32)
    main, nb, inc, mm = mark_brick(world.reshape(-1, 3)[px], bbox_min, brick_size, res_bricks)
    return n, margin, dict(pixel=px, main=main, neighbour=nb, add=inc, margin=mm)


def brick_counts(marks, n_bricks, sure=None):
    """the counters mark_brick leaves, from the marks of all streams; sure: a mask over the marks"""
    keep = np.ones(marks["main"].shape, bool) if sure is None else sure
    c = np.bincount(marks["main"][keep], minlength=n_bricks)
    return c + np.bincount(marks["neighbour"][keep], weights=marks["add"][keep], minlength=n_bricks).astype(np.int64)


def brick_slack(marks, unsure, res_bricks):
    """per brick: the number of marking pixels whose margin is below the bound and which may touch that brick one way or the other -- the
    bricks of the 3 x 3 x 3 neighbourhood of the pixel's own brick"""
    res = np.asarray(res_bricks, np.int64)
    m = marks["main"][unsure]
    idx = np.stack([m % res[0], m // res[0] % res[1], m // (res[0] * res[1])], -1)
    out = np.zeros(int(res.prod()), np.int64)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                j = idx + (dx, dy, dz)
                ok = ((j >= 0) & (j < res)).all(-1)
                np.add.at(out, ((j[ok, 2] * res[1] + j[ok, 1]) * res[0] + j[ok, 0]), 1)
    return out


# ---------------------------------------------------------------------------------------------------------------- quality
def quality_pass(depth_b, normals, cv_xyz, camera_position):
    """depth_b [h][w][2] fp32, normals [h][w][3] fp32 -> (quality [h][w], margin).  pre_quality.fs:65-119; is_outside :39-41 exact."""
    d32 = np.asarray(depth_b, np.float32)[..., 0]
    h, w = d32.shape
    t = Taps(h, w)
    with np.errstate(invalid="ignore"):
        out32 = ~((d32 > np.float32(0.0)) & (d32 < np.float32(1.0)))
    d = d32.astype(np.float64)
    drm = F(0.35) * d                                                                       # :72-74
    with np.errstate(invalid="ignore", divide="ignore"):
        inv = 1.0 / drm
    border = np.zeros((h, w)); wr = np.zeros((h, w)); mt = np.full((h, w), INF)
    for y in range(-6, 7):
        for x in range(-6, 7):
            ds, so = t(d, x, y), t(out32, x, y)
            with np.errstate(invalid="ignore"):
                rng = np.abs(ds - d)                                                        # :92
                b = so | (rng > drm)                                                        # :93
                mt = np.minimum(mt, np.where(so, INF, np.abs(rng - drm)))
                border += b
                wr += np.where(b, 0.0, 1.0 - np.minimum(rng, drm) * inv)                    # :99, :103
    u, v = grid_uv(h, w)
    nrm = tex2d_linear(np.asarray(normals, np.float64), u, v)                               # :44
    wp = tex3d(cv_xyz, np.stack([u, v, d], -1))                                             # :45
    to_cam = np.asarray(camera_position, np.float32).astype(np.float64) - wp
    with np.errstate(invalid="ignore", divide="ignore"):
        to_cam = to_cam / np.sqrt((to_cam ** 2).sum(-1))[..., None]
        angle = (to_cam * nrm).sum(-1)                                                      # :46
        q = (1.0 - border / 169.0) ** 6 * (wr / 169.0) ** 6 / (d * F(6.5)) * angle ** 2     # :107-114
    q = np.where(out32, 0.0, q)                                                             # :68-70
    with np.errstate(invalid="ignore"):
        margin = np.where(out32, INF, np.where(angle < 0, 0.0, np.minimum(mt, t.boundary(6))))
    nn = np.isnan(np.asarray(normals, np.float64)).any(-1)                                  # a NaN texel under a LINEAR fetch's footprint: its weight
    foot = np.any([t(nn, x, y) for y in (-1, 0, 1) for x in (-1, 0, 1)], 0)                 # is 0 at a pixel centre, and 0 * NaN is whoever's choice
    margin = np.where(np.isnan(q) | np.isnan(d32) | foot, 0.0, margin)
    return q, margin
