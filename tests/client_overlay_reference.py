"""CPU reference of the client's last two mono draws (source/kinect_client.cpp:685-707), as defined in include/rgbd_recon_hip.h.  numpy, fp32
throughout, every operation in the order the header states it.

* draw_bbox(...): the bounding-box wireframe, gloost::BoundingBox::draw() -> drawWiredBox: 24 segments of width 2.  The near / far clip and
  the in-order GL_LESS loop are tests/overlay_reference.py's; the wide-line walk is its width-1 walk with the -0.5 minor shift and the
  2-fragment replication (wide_window_line_fragments(..., width=1) is checked against overlay_reference.window_line_fragments).
* blit(...): TextureBlitter::blit(unit, resolution_full / 2): bilinear, CLAMP_TO_EDGE, (rgb, 1) into the viewport (0, 0, vw, vh).
"""
import numpy as np

import overlay_reference as O

F = np.float32
BBOX_COLOR = np.array([1, 1, 1, 0.75], np.float32)
# drawWiredBox (gloostRenderGoodies.h:251-304): front, right, back, left, top, bottom; corner = x | y << 1 | z << 2 (0 = min, 1 = max)
BBOX_LOOPS = [(4, 5, 7, 6), (5, 1, 3, 7), (1, 0, 2, 3), (0, 4, 6, 2), (6, 7, 3, 2), (0, 1, 5, 4)]


def bbox_corner(bmin, bmax, k):
    return [F(bmax[a]) if (k >> a) & 1 else F(bmin[a]) for a in range(3)]


def bbox_segments(bmin, bmax):
    """the 24 segments in draw order: index 4 * loop + k runs from corner k of the loop to corner (k + 1) % 4"""
    return [(bbox_corner(bmin, bmax, lp[k]), bbox_corner(bmin, bmax, lp[(k + 1) % 4])) for lp in BBOX_LOOPS for k in range(4)]


def to_window(a, b, view):
    """near then far clip of clip-space a -> b, then window coordinates (None: nothing left)"""
    a, b = [F(x) for x in a], [F(x) for x in b]
    r = O.clip_plane(a, b, a[2] + a[3], b[2] + b[3])
    if r is None:
        return None
    a, b = r
    r = O.clip_plane(a, b, a[3] - a[2], b[3] - b[2])
    if r is None:
        return None
    a, b = r
    if not (a[3] > 0) or not (b[3] > 0):
        return None
    W, H = F(view[0]), F(view[1])
    wa = ((a[0] / a[3] * F(0.5) + F(0.5)) * W, (a[1] / a[3] * F(0.5) + F(0.5)) * H, a[2] / a[3] * F(0.5) + F(0.5))
    wb = ((b[0] / b[3] * F(0.5) + F(0.5)) * W, (b[1] / b[3] * F(0.5) + F(0.5)) * H, b[2] / b[3] * F(0.5) + F(0.5))
    return wa, wb


def wide_window_line_fragments(a, b, view, width=2):
    """GL 4.4 section 14.5.2.2 (aliased) between window points a -> b: shift by -(width - 1) / 2 in the minor direction, walk with the
    width-1 diamond-exit rule, replicate each fragment `width` times upwards in the minor direction, each dropped on its own outside the
    view; fragments (px, py, z) in walk order"""
    ax, ay, az = [F(x) for x in a]
    bx, by, bz = [F(x) for x in b]
    xmajor = abs(F(bx - ax)) >= abs(F(by - ay))
    s0, s1, o0, o1 = (ax, bx, ay, by) if xmajor else (ay, by, ax, bx)
    if width > 1:
        shift = F(0.5) * F(width - 1)
        o0, o1 = F(o0 - shift), F(o1 - shift)
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
        z = F(az + F(F(bz - az) * tz))
        if z != z:
            continue
        z = z if z > 0 else F(0)
        z = z if z < 1 else F(1)
        for r in range(width):
            mr = F(m + F(r))
            if not (mr >= 0 and mr < n_minor):
                continue
            out.append((i, int(mr), z) if xmajor else (int(mr), i, z))
    return out


def wide_line_fragments(a, b, view, width=2):
    w = to_window(a, b, view)
    return [] if w is None else wide_window_line_fragments(w[0], w[1], view, width)


def bbox_fragments(bmin, bmax, mv, pr, view):
    """(segment index, px, py, z) in draw order"""
    out = []
    for s, (p, q) in enumerate(bbox_segments(bmin, bmax)):
        for px, py, z in wide_line_fragments(O.frustum_clip(mv, pr, p), O.frustum_clip(mv, pr, q), view):
            out.append((s, px, py, z))
    return out


def draw_bbox(bmin, bmax, mv, pr, view, fb_c, fb_d):
    return O.gl_less(((px, py, z, BBOX_COLOR) for _, px, py, z in bbox_fragments(bmin, bmax, mv, pr, view)), fb_c, fb_d)


def bbox_winners(bmin, bmax, mv, pr, view, fb_d):
    """per pixel the segment index whose fragment the in-order GL_LESS keeps (-1: none passed)"""
    d = np.array(fb_d, np.float32, copy=True)
    win = np.full(d.shape, -1, np.int64)
    for s, px, py, z in bbox_fragments(bmin, bmax, mv, pr, view):
        if F(z) < d[py, px]:
            d[py, px] = F(z)
            win[py, px] = s
    return win


# ---------------------------------------------------------------------- the texture view
def blit_viewport(w, h):
    """uvec2(fvec2(resolution_full) / 2) with resolution_full = uvec2(1.5f * w, h) (view_lod.cpp:29, kinect_client.cpp:706)"""
    rfx = int(F(1.5) * F(w))
    return int(F(rfx) / F(2)), int(F(h) / F(2))


def blit(src, view, fb_c):
    """src [sh][sw][4]: texture(src, ((x + .5) / vw, (y + .5) / vh)).rgb, 1 into rows y < vh, columns x < vw of a copy of fb_c"""
    src = np.asarray(src, np.float32)
    sh, sw = src.shape[:2]
    vw, vh = blit_viewport(*view)
    u = (np.arange(vw, dtype=np.float32) + F(0.5)) / F(vw)
    v = (np.arange(vh, dtype=np.float32) + F(0.5)) / F(vh)
    x0, x1, ax = O.axis_linear(u, sw)
    y0, y1, ay = O.axis_linear(v, sh)
    t00, t10 = src[y0[:, None], x0[None, :]], src[y0[:, None], x1[None, :]]
    t01, t11 = src[y1[:, None], x0[None, :]], src[y1[:, None], x1[None, :]]
    axx, ayy = ax[None, :, None], ay[:, None, None]
    rgb = O.lerp(O.lerp(t00, t10, axx), O.lerp(t01, t11, axx), ayy)
    out = np.array(fb_c, np.float32, copy=True)
    out[:vh, :vw, :3] = rgb[..., :3]
    out[:vh, :vw, 3] = F(1)
    return out
