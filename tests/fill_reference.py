"""float64 numpy reference of hole filling, fillColors(): the literal two-atlas sequence.  HIP-free, and written from the reference's
shaders and host code alone -- not from oracle/tsdf_oracle.cpp and not from k_inpaint.hip, whose composed squeeze mapping, tap classes
and fp32 operation order it does not share:

* lod_tables     framework/rendering/view_lod.cpp:24-50 (ViewLod::setResolution): num_lods, resolutions, offsets, the atlas size
* transfer       ViewLod::enable(0) (view_lod.cpp:62-82: viewport of level 0, the WHOLE attachment cleared to colour (0, 1, 0, 0) and depth 1)
                 and glsl/framebuffer_transfer.fs:13-17 over ScreenQuad::draw with glsl/texture_passthrough.vs:9-12
* inpaint_level  glsl/tsdf_inpaint.fs:30-89 over the viewport of level lod + 1 (ViewLod::enable(i, false, false): nothing cleared)
* colorfill      glsl/tsdf_colorfill.fs:20-55 into the default framebuffer under GL_LESS and glColorMask (recon_integration.cpp:313-334)
* fill_colors    recon_integration.cpp:279-338 with the uniforms of :491-499: which atlas each pass binds after each std::swap

Sampler state: the colour atlas is RGBA32F with GL_MIRRORED_REPEAT on both axes and globjects' default LINEAR filter (view_lod.cpp:52-53),
the depth atlas NEAREST (:54-55); only tsdf_colorfill.fs:43-46 filters at all (texture()), every other read is a texelFetch.  A linear
fetch is the weighted sum of its four taps.  An out-of-range texelFetch returns 0 in every channel, as SURVEY.md Appendix A fixes it (GL
leaves it undefined without robust buffer access).  The depth attachment is GL_DEPTH_COMPONENT32, fixed point; the project holds it as
float and so does this module.  gl_FragCoord is the integer pixel (pixel_center_integer), pass_TexCoord the pixel centre over the
viewport size.

Everything is float64.  An atlas is a pair (colour [h][W][4], depth [h][W]) with W = int(1.5f * w), row 0 = gl_FragCoord.y 0.

Every position that ends in an ivec2() truncation is evaluated twice: in exact rational arithmetic (fractions.Fraction; GLSL literals such
as 2.0 / 3.0 enter as the fp32 constants they are) and in numpy float32 in the shader's own operation order.  The exact value is used;
where the two truncate differently the element gets margin 0, because GL leaves the rounding of a division open.

Every function also returns a *decision margin* per output pixel:
* truncation   distance of the exact coordinate to the integer boundary it could cross (1 for an exactly integral value: there the fp32
               evaluation decides), and 0 where fp32 and exact disagree; colorfill() evaluates the whole shader under both sets of
               truncations and gives margin 0 where the two write different values (two candidate texels of equal content have one answer)
* mean depth   the smallest |d_i - depth_av| over the valid samples of tsdf_inpaint.fs:77; a tie that is exact in every precision (one
               valid sample, or 2 or 4 equal ones: sequential sums of 2 and 4 equal values are exact) has none (inf)
* undefined    0 where the shader is: to_lod_pos2 at a level >= num_lods (zero uniform slots, clamp with min > max)
The alpha and depth < 1 tests compare stored values and the bilinear fetch is continuous: neither has a margin -- but for a NaN or
infinite texel under a vanishing weight (texture_linear_mirrored), which counts as undefined.  The margin returned is the
smallest of these; `trunc_ok` says which pixels' truncations are safe, so a caller can tell the causes apart.
"""
import functools
from fractions import Fraction

import numpy as np

INF = np.inf
f32 = np.float32
CLEAR_COLOR, CLEAR_DEPTH = (0.0, 1.0, 0.0, 0.0), 1.0              # view_lod.cpp:75-81
TWO_THIRDS = f32(2.0) / f32(3.0)                                  # the literal of tsdf_inpaint.fs:38, an fp32 constant


# ---------------------------------------------------------------------------------------------------------------- ViewLod
def lod_tables(w, h):
    """ViewLod::setResolution -> dict(num_lods, res [n][2], off [n][2], full (W, h)); (x, y) order"""
    n = 1 + int(np.floor(np.log2(f32(min(w, h)))))                # :25, glm::log2(float)
    assert n == min(w, h).bit_length()
    full = (int(f32(w) * f32(1.5)), h)                            # :29, uvec2{width * 1.5f, height}
    res, off = np.zeros((n, 2), np.int64), np.zeros((n, 2), np.int64)
    ox, oy = w, h                                                 # :37
    for i in range(n):
        p = f32(2.0) ** f32(i)
        res[i] = int(np.floor(f32(w) / p)), int(np.floor(f32(h) / p))       # :39
        if i > 0:                                                 # :42-45
            oy -= res[i][1]
            off[i] = ox, oy
    return dict(num_lods=n, res=res, off=off, full=full, view=(w, h))


def cleared_atlas(t):
    W, h = t["full"]
    c = np.empty((h, W, 4))
    c[:] = CLEAR_COLOR
    return c, np.full((h, W), CLEAR_DEPTH)


def place_level(atlas, t, lod, rgba, depth):
    (ox, oy), (rx, ry) = t["off"][lod], t["res"][lod]
    atlas[0][oy:oy + ry, ox:ox + rx] = rgba
    atlas[1][oy:oy + ry, ox:ox + rx] = depth


def level_of(atlas, t, lod):
    (ox, oy), (rx, ry) = t["off"][lod], t["res"][lod]
    return atlas[0][oy:oy + ry, ox:ox + rx], atlas[1][oy:oy + ry, ox:ox + rx]


# ---------------------------------------------------------------------------------------------------------------- truncations
def _trunc(exact, single):
    """exact: Fractions, single: the same positions in float32 -> (int64 of the exact ones, margin)"""
    i = np.array([int(e) for e in exact], np.int64)               # ivec2(): towards zero; every position here is >= 0
    fr = [e - int(e) for e in exact]
    m = np.array([1.0 if f == 0 else float(min(f, 1 - f)) for f in fr])
    m[np.asarray(single).astype(np.int64) != i] = 0.0
    return i, m


def _fetch(atlas, x, y):
    """texelFetch of colour and depth at integer (x, y) arrays; out of range -> 0"""
    h, W = atlas[1].shape
    ok = (x >= 0) & (y >= 0) & (x < W) & (y < h)
    xc, yc = np.clip(x, 0, W - 1), np.clip(y, 0, h - 1)
    return np.where(ok[..., None], atlas[0][yc, xc], 0.0), np.where(ok, atlas[1][yc, xc], 0.0)


# ---------------------------------------------------------------------------------------------------------------- transfer
def transfer_columns(t):
    """squeezed column x -> atlas column ivec2(pass_TexCoord * resolution_tex).x, and rows likewise: (cols, rows, col margin, row margin)"""
    return _transfer_columns(t["view"])


@functools.lru_cache(maxsize=None)
def _transfer_columns(view):
    t = lod_tables(*view)
    (w, h), (W, _) = t["view"], t["full"]
    xs, ys = np.arange(w), np.arange(h)
    cx, mx = _trunc([Fraction(2 * x + 1, 2 * w) * W for x in xs], (xs.astype(f32) + f32(0.5)) / f32(w) * f32(W))
    cy, my = _trunc([Fraction(2 * y + 1, 2 * h) * h for y in ys], (ys.astype(f32) + f32(0.5)) / f32(h) * f32(h))
    return cx, cy, mx, my


def transfer(atlas, t):
    """ViewLod::enable(0) of the other atlas, then framebuffer_transfer.fs over the viewport (0, 0, w, h) under GL_ALWAYS ->
    (squeezed atlas, margin [h][W]: inf over the cleared rest)"""
    w, h = t["view"]
    cx, cy, mx, my = transfer_columns(t)
    out = cleared_atlas(t)
    c, d = _fetch(atlas, cx[None, :] + 0 * cy[:, None], cy[:, None] + 0 * cx[None, :])
    out[0][:h, :w], out[1][:h, :w] = c, d
    margin = np.full(out[1].shape, INF)
    margin[:h, :w] = np.minimum(mx[None, :], my[:, None])
    return out, margin


# ---------------------------------------------------------------------------------------------------------------- inpaint
def inpaint_positions(t, lod):
    """pos_int of tsdf_inpaint.fs:37-38 per column and row of level lod + 1: (px [rx], py [ry], margin x, margin y)"""
    return _inpaint_positions(t["view"], lod)


@functools.lru_cache(maxsize=None)
def _inpaint_positions(view, lod):
    t = lod_tables(*view)
    out = []
    for k in (0, 1):
        r1, r0, o0 = int(t["res"][lod + 1][k]), int(t["res"][lod][k]), int(t["off"][lod][k])
        p = np.arange(r1)
        tc = p.astype(f32) / f32(r1)                              # (gl_FragCoord - offsets[lod + 1]) / resolutions[lod + 1]; the difference is exact
        l, m1 = _trunc([o0 + Fraction(r0 * int(i), r1) for i in p], f32(o0) + f32(r0) * tc)            # to_lod_pos :30-32
        scale = TWO_THIRDS if k == 0 else f32(1.0)
        q, m2 = _trunc([Fraction(int(i)) * Fraction(float(scale)) for i in l], l.astype(f32) * scale)     # :38
        out += [q, np.minimum(m1, m2)]
    return out[0], out[2], out[1], out[3]


def inpaint_level(S, t, lod, squeeze_margin=None):
    """tsdf_inpaint.fs over the viewport of level lod + 1, reading the squeezed copy S -> dict(rgba [ry][rx][4], depth, margin, trunc_ok,
    mean_margin, n: the valid samples).  squeeze_margin: transfer()'s, so that a tap read through an unsafe truncation taints the pixel."""
    px, py, mx, my = inpaint_positions(t, lod)
    X, Y = px[None, :] + 0 * py[:, None], py[:, None] + 0 * px[None, :]
    trunc = np.minimum(mx[None, :], my[:, None])
    n = np.zeros(X.shape, np.int64)
    depth_av = np.zeros(X.shape)
    smp = []
    for x in range(4):                                            # :43-57, the shader's own loop order
        for y in range(4):
            tx, ty = X + (x - 1), Y + (y - 1)                     # ivec2(x - kernel_size * 0.5 + 1, ...)
            c, d = _fetch(S, tx, ty)
            with np.errstate(invalid="ignore"):
                valid = ~(c[..., 3] <= 0.0)
            depth_av = depth_av + np.where(valid, d, 0.0)
            n += valid
            smp.append((x + y * 4, valid, c[..., :3], d))
            if squeeze_margin is not None:
                h, W = squeeze_margin.shape
                ok = (tx >= 0) & (ty >= 0) & (tx < W) & (ty < h)
                trunc = np.minimum(trunc, np.where(ok, squeeze_margin[np.clip(ty, 0, h - 1), np.clip(tx, 0, W - 1)], INF))
    smp.sort(key=lambda s: s[0])                                  # samples[x + y * kernel_size]
    some = n > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        depth_av = depth_av / np.where(some, n, 1)                # :71
        dmin = np.full(X.shape, INF)
        dmax = np.full(X.shape, -INF)
        mean_margin = np.full(X.shape, INF)
        for _, valid, _, d in smp:
            dmin = np.where(valid, np.minimum(dmin, d), dmin)
            dmax = np.where(valid, np.maximum(dmax, d), dmax)
            mean_margin = np.where(valid, np.minimum(mean_margin, np.abs(d - depth_av)), mean_margin)
        exact_tie = some & (dmin == dmax) & np.isin(n, (1, 2, 4))
        mean_margin[some & (dmin == dmax)] = 0.0                  # equal depths: (d + .. + d) / n against d is a matter of rounding ...
        mean_margin[exact_tie] = INF                              # ... unless the sum is exact
        tc, td, tw = np.zeros(X.shape + (3,)), np.zeros(X.shape), np.zeros(X.shape)
        for _, valid, c, d in smp:                                # :76-88
            keep = valid & (c[..., 0] >= 0.0) & ((d >= depth_av) | exact_tie)
            tc = tc + np.where(keep[..., None], c, 0.0)
            td = td + np.where(keep, d, 0.0)
            tw = tw + keep
        rgba = np.concatenate([tc / tw[..., None], np.ones(X.shape + (1,))], -1)
        depth = td / tw
    cc, cd = _fetch(S, X, Y)                                      # :59-68
    none = ~some
    depth = np.where(none, cd, depth)
    rgba[none & (cd < 1.0)] = (0.0, 0.0, 0.0, -1.0)
    rgba[none & ~(cd < 1.0)] = (0.0, 1.0, 0.0, 0.0)
    mean_margin[none] = INF
    trunc_ok = trunc > 0
    return dict(rgba=rgba, depth=depth, margin=np.where(trunc_ok, mean_margin, 0.0), trunc_ok=trunc_ok, trunc=trunc, mean_margin=mean_margin, n=n)


# ---------------------------------------------------------------------------------------------------------------- colour fill
def _mirror(i, n):
    """GL_MIRRORED_REPEAT: mirror(a) = a if a >= 0 else -(1 + a), over periods of 2 n"""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


SUBTEXEL = 2.0 ** -8                                              # GL asks for no more than 8 fractional bits of a linear filter's weights


def texture_linear_mirrored(color, u, v):
    """texture() on the colour atlas: LINEAR, MIRRORED_REPEAT, the weighted sum of four taps -> (value, fragile).  fragile: a tap that is
    not finite carries a weight below SUBTEXEL -- whether 0 * NaN reaches the result then hangs on the last bits of the coordinate, the
    one place where the otherwise continuous fetch is not"""
    h, W = color.shape[:2]
    fx, fy = u * W - 0.5, v * h - 0.5
    x0, y0 = np.floor(fx), np.floor(fy)
    ax, ay = (fx - x0)[..., None], (fy - y0)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    xa, xb, ya, yb = _mirror(x0, W), _mirror(x0 + 1, W), _mirror(y0, h), _mirror(y0 + 1, h)
    out, fragile = 0.0, np.zeros(u.shape, bool)
    with np.errstate(invalid="ignore"):
        for tap, wt in ((color[ya, xa], (1 - ax) * (1 - ay)), (color[ya, xb], ax * (1 - ay)), (color[yb, xa], (1 - ax) * ay), (color[yb, xb], ax * ay)):
            out = out + tap * wt
            fragile |= ~np.isfinite(tap).all(-1) & (wt[..., 0] < SUBTEXEL)
    return out, fragile


def colorfill_positions(t, lod):
    """to_lod_pos(gl_FragCoord / resolutions[0], lod) per column and row of the framebuffer:
    (cx [w], cy [h], margin x, margin y, the float32 evaluation's cx, cy)"""
    return _colorfill_positions(t["view"], lod)


@functools.lru_cache(maxsize=None)
def _colorfill_positions(view, lod):
    t = lod_tables(*view)
    out = []
    for k in (0, 1):
        r0, rl, ol = int(t["res"][0][k]), int(t["res"][lod][k]), int(t["off"][lod][k])
        p = np.arange(t["view"][k])
        single = f32(ol) + f32(rl) * (p.astype(f32) / f32(r0))
        out += list(_trunc([ol + Fraction(rl * int(i), r0) for i in p], single)) + [single.astype(np.int64)]
    return out[0], out[3], out[1], out[4], out[2], out[5]


def _lod_pos2(t, ptc, lod, k):
    """to_lod_pos2 along axis k; a slot >= num_lods holds zeros, and clamp(x, .5, -.5) is undefined: min(max()) is one possible outcome"""
    o, r = (float(t["off"][lod][k]), float(t["res"][lod][k])) if lod < t["num_lods"] else (0.0, 0.0)
    return np.minimum(np.maximum(o + r * ptc, o + 0.5), o + r - 0.5)


def _colorfill(T, t, mask, base, single):
    """the shader with every truncation as exact arithmetic gives it, or (single) as float32 in the shader's operation order does"""
    w, h = t["view"]
    n = t["num_lods"]
    level = np.full((h, w), n, np.int64)
    out = np.zeros((h, w, 4))
    searching = np.ones((h, w), bool)
    for l in range(n):                                            # :36-40
        cx, cy = colorfill_positions(t, l)[4 if single else 0:][:2]
        c, d = _fetch(T, cx[None, :] + 0 * cy[:, None], cy[:, None] + 0 * cx[None, :])
        if l == 0:
            depth0 = d                                            # :54 fetches the same position again
        out[searching] = c[searching]
        with np.errstate(invalid="ignore"):
            found = searching & (c[..., 3] > 0.0)
        level[found] = l
        searching &= ~found
    ptx, pty = (np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h             # pass_TexCoord
    W, _ = t["full"]
    rix, riy = float(f32(1.0) / f32(W)), float(f32(1.0) / f32(h))              # resolution_inv, recon_integration.cpp:497
    w1 = np.sqrt(ptx[None, :] ** 2 + pty[:, None] ** 2)                        # distance(tc, floor(tc)), tc in (0, 1)
    w2 = 1.0 - w1
    undefined = np.zeros((h, w), bool)
    for lv in range(1, n + 1):                                    # :42-51
        at = level == lv
        if not at.any():
            continue
        ys, xs = np.nonzero(at)                                   # only the pixels whose search ended at lv
        c = []
        for l in (lv + 1, lv + 2):
            u, v = _lod_pos2(t, ptx, l, 0) * rix, _lod_pos2(t, pty, l, 1) * riy
            val, fragile = texture_linear_mirrored(T[0], u[xs], v[ys])
            c.append(val)
            undefined[ys, xs] |= fragile
        with np.errstate(invalid="ignore"):
            out[ys, xs] = (c[0] * w1[ys, xs, None] + c[1] * w2[ys, xs, None]) / (w1 + w2)[ys, xs, None]
        if lv + 2 >= n:
            undefined |= at
    written = depth0 < 1.0                                        # GL_LESS against the cleared depth
    kept = np.zeros((h, w, 4)) if base is None else np.asarray(base, np.float64)
    chan = {0: [True] * 4, 1: [True, False, False, False], 2: [False, True, True, False]}[mask]           # :321-326
    rgba = np.where(written[..., None] & np.array(chan), out, kept)
    return dict(rgba=rgba, depth=np.where(written, depth0, 1.0), level=level, written=written, undefined=undefined & written)


def colorfill(T, t, mask=0, base=None):
    """tsdf_colorfill.fs over the framebuffer's w x h pixels, reading the finished atlas T, with the depth buffer cleared to 1 (GL_LESS) and
    the colour buffer cleared to 0 (base None) or kept (base [h][w][4]); mask: m_color_mask_mode 0 / 1 (red) / 2 (green and blue)
    -> dict(rgba, depth, margin, trunc_ok, level: where the search ended, written, undefined).
    Truncation margin: the shader is evaluated with the exact truncations and with the float32 ones; a pixel is safe where both write the
    same colour and depth -- a pixel whose two candidate texels hold the same value does not depend on how the division rounds."""
    r = _colorfill(T, t, mask, base, False)
    unsafe = any((m == 0).any() for l in range(t["num_lods"]) for m in colorfill_positions(t, l)[2:4])
    trunc_ok = np.ones(r["written"].shape, bool)
    if unsafe:
        s = _colorfill(T, t, mask, base, True)
        with np.errstate(invalid="ignore"):
            same = ((r["rgba"] == s["rgba"]) | (np.isnan(r["rgba"]) & np.isnan(s["rgba"]))).all(-1) & (r["depth"] == s["depth"])
        trunc_ok = same & (r["undefined"] == s["undefined"])
    r["trunc_ok"] = trunc_ok
    r["margin"] = np.where(trunc_ok & ~r["undefined"], INF, 0.0)
    return r


# ---------------------------------------------------------------------------------------------------------------- fillColors()
def fill_colors(level0_rgba, level0_depth, mask=0, base=None):
    """recon_integration.cpp:279-338 on the atlas the draw left: ViewLod::enable(0) cleared all of it and the march wrote level 0.
    -> dict(atlas, squeezed: the other atlas as it ends, framebuffer: colorfill()'s dict, levels: inpaint_level()'s dicts, tables).
    The margins are each step's own; they are not carried down the chain."""
    h, w = np.asarray(level0_depth).shape
    t = lod_tables(w, h)
    view_inpaint = cleared_atlas(t)
    place_level(view_inpaint, t, 0, np.asarray(level0_rgba, np.float64), np.asarray(level0_depth, np.float64))
    view_inpaint2 = None                                          # whatever it held: enable(0) clears it
    view_inpaint2, _ = transfer(view_inpaint, t)                  # :282-288 binds m_view_inpaint, draws into m_view_inpaint2
    view_inpaint, view_inpaint2 = view_inpaint2, view_inpaint     # :289
    levels = []
    for i in range(1, t["num_lods"]):                             # :291
        lv = inpaint_level(view_inpaint, t, i - 1)                # :292-299 binds m_view_inpaint (squeezed), draws level i of m_view_inpaint2
        place_level(view_inpaint2, t, i, lv["rgba"], lv["depth"])
        levels.append(lv)
        view_inpaint, view_inpaint2 = view_inpaint2, view_inpaint             # :301
        view_inpaint2, _ = transfer(view_inpaint, t)              # :303-310
        view_inpaint, view_inpaint2 = view_inpaint2, view_inpaint             # :311
    fb = colorfill(view_inpaint2, t, mask, base)                  # :315 binds m_view_inpaint2: the atlas with every level
    return dict(atlas=view_inpaint2, squeezed=view_inpaint, framebuffer=fb, levels=levels, tables=t)
