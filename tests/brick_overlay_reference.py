"""CPU reference of the occupied-brick wireframes (tsdf_draw_bricks; ReconIntegration::drawOccupiedBricks, recon_integration.cpp:447-454 =
glsl/bricks.vs + glsl/solid.fs over UnitCube::drawWireInstanced), as defined in include/rgbd_recon_hip.h.  numpy, fp32 throughout, every
operation in the order the header states it.

* draw_bricks_literal(...): the definition, on top of tests/overlay_reference.py: mat_mul for the vertices, line_fragments for each of a
  brick's 12 segments, the in-order GL_LESS loop gl_less over (brick in ascending id, segment).  Slow; pins the other one.
* draw_bricks(...): the same result vectorised over segments (the clip, the window transform and the diamond-exit walk of
  overlay_reference.line_fragments restated on arrays), the depth test as "the smallest (z, primitive index) among the fragments that pass
  z < fb_d", primitive index 12 * id + segment -- what the in-order loop keeps.  tests/test_brick_overlay_reference.py checks the two
  against each other.
"""
import numpy as np

import overlay_reference as O

F = np.float32
WIRE_COLOR = np.array([1, 0, 0, 1], np.float32)                       # uniform Color (1, 0, 0), solid.fs: (Color, 1)
# the unit cube's vertex table and the 12 GL_LINES of drawWireInstanced, start -> end (unit_cube.cpp:20-29,74-83)
CUBE_VERTS = np.array([(1, 1, 1), (0, 1, 1), (1, 1, 0), (0, 1, 0), (1, 0, 1), (0, 0, 1), (0, 0, 0), (1, 0, 0)], np.float32)
CUBE_WIRE = [(0, 1), (0, 2), (0, 4), (5, 1), (5, 4), (5, 6), (3, 1), (3, 6), (3, 2), (7, 2), (7, 4), (7, 6)]


def brick_ids(flags_or_ids, n_bricks):
    """ascending brick ids from a per-brick flag array (length n_bricks, as tsdf_download_bricks returns it) or from a list of ids in any
    order: the reference's list ascends in brick id, and GL draws the instances in list order"""
    a = np.asarray(flags_or_ids)
    if a.dtype == np.uint8 or a.dtype == np.bool_:
        assert a.size == n_bricks
        return np.flatnonzero(a).astype(np.int64)
    return np.sort(a.astype(np.int64).reshape(-1))


def index_3d(ids, res_bricks):
    """inc_bricks.glsl:30-38"""
    ids = np.asarray(ids, np.int64)
    rx, ry = int(res_bricks[0]), int(res_bricks[1])
    z = ids // (rx * ry)
    rem = ids % (rx * ry)
    return rem % rx, rem // rx, z


def vertex_clip(ids, res_bricks, brick_size, bbox_min, mv, pr):
    """clip-space position of the 8 cube vertices of every brick: 4 arrays [n][8].  to_world(position, index) = float(index) * brick_size +
    bbox_min + position * brick_size per axis (bricks.vs:16-20, inc_bricks.glsl:22-24), then P . (MV . (world, 1))"""
    idx = index_3d(ids, res_bricks)
    p = []
    for a in range(3):
        base = idx[a].astype(np.float32)[:, None] * F(brick_size[a]) + F(bbox_min[a])
        p.append((base + CUBE_VERTS[None, :, a] * F(brick_size[a])).astype(np.float32))
    e = O.mat_mul(mv, p[0], p[1], p[2], F(1))
    return O.mat_mul(pr, e[0], e[1], e[2], e[3])


# ---------------------------------------------------------------------- the definition
def brick_fragments_literal(ids, res_bricks, brick_size, bbox_min, mv, pr, view):
    """(primitive index, px, py, z) in draw order"""
    ids = np.sort(np.asarray(ids, np.int64).reshape(-1))
    clip = vertex_clip(ids, res_bricks, brick_size, bbox_min, mv, pr)
    out = []
    for n, i in enumerate(ids):
        v = [[clip[k][n, c] for k in range(4)] for c in range(8)]
        for s, (a, b) in enumerate(CUBE_WIRE):
            for px, py, z in O.line_fragments(v[a], v[b], view):
                out.append((12 * int(i) + s, px, py, z))
    return out


def draw_bricks_literal(flags_or_ids, res_bricks, brick_size, bbox_min, mv, pr, view, fb_c, fb_d):
    ids = brick_ids(flags_or_ids, int(np.prod(res_bricks)))
    frags = brick_fragments_literal(ids, res_bricks, brick_size, bbox_min, mv, pr, view)
    return O.gl_less(((px, py, z, WIRE_COLOR) for _, px, py, z in frags), fb_c, fb_d)


# ---------------------------------------------------------------------- vectorised over segments
def _clip_plane(a, b, da, db, alive):
    """overlay_reference.clip_plane on arrays: a, b lists of 4 arrays; returns the moved end points and the updated alive mask"""
    a_in, b_in = da >= 0, db >= 0
    alive = alive & (a_in | b_in)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ta = (da / (da - db)).astype(np.float32)
        tb = (db / (db - da)).astype(np.float32)
        move_a, move_b = ~a_in, a_in & ~b_in
        na = [np.where(move_a, (a[k] + (b[k] - a[k]) * ta).astype(np.float32), a[k]) for k in range(4)]
        nb = [np.where(move_b, (b[k] + (a[k] - b[k]) * tb).astype(np.float32), b[k]) for k in range(4)]
    return na, nb, alive


def brick_fragments(ids, res_bricks, brick_size, bbox_min, mv, pr, view):
    """arrays (primitive index, px, py, z) of every fragment inside the view (order: by segment, then along the walk)"""
    ids = np.sort(np.asarray(ids, np.int64).reshape(-1))
    empty = (np.zeros(0, np.int64),) * 3 + (np.zeros(0, np.float32),)
    if ids.size == 0:
        return empty
    clip = vertex_clip(ids, res_bricks, brick_size, bbox_min, mv, pr)
    va, vb = [w[0] for w in CUBE_WIRE], [w[1] for w in CUBE_WIRE]
    a = [clip[k][:, va].reshape(-1) for k in range(4)]                  # [n * 12], segment fastest
    b = [clip[k][:, vb].reshape(-1) for k in range(4)]
    prim = (12 * ids[:, None] + np.arange(12)[None, :]).reshape(-1)
    alive = np.ones(prim.size, bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        a, b, alive = _clip_plane(a, b, a[2] + a[3], b[2] + b[3], alive)  # near
        a, b, alive = _clip_plane(a, b, a[3] - a[2], b[3] - b[2], alive)  # far
        alive &= (a[3] > 0) & (b[3] > 0)
        W, H = F(view[0]), F(view[1])
        ax, ay, az = (a[0] / a[3] * F(0.5) + F(0.5)) * W, (a[1] / a[3] * F(0.5) + F(0.5)) * H, a[2] / a[3] * F(0.5) + F(0.5)
        bx, by, bz = (b[0] / b[3] * F(0.5) + F(0.5)) * W, (b[1] / b[3] * F(0.5) + F(0.5)) * H, b[2] / b[3] * F(0.5) + F(0.5)
        xmajor = np.abs(bx - ax) >= np.abs(by - ay)
        s0, s1 = np.where(xmajor, ax, ay), np.where(xmajor, bx, by)
        o0, o1 = np.where(xmajor, ay, ax), np.where(xmajor, by, bx)
        n_major = np.where(xmajor, view[0], view[1]).astype(np.int64)
        n_minor = np.where(xmajor, view[1], view[0]).astype(np.int64)
        # candidate pixel columns / rows: a superset of those whose centre lies on the segment (every i in [0, n_major) where a bound is NaN)
        lo = np.fmax(np.floor(np.fmin(s0, s1)) - F(1), F(0))
        hi = np.fmin(np.ceil(np.fmax(s0, s1)) + F(1), (n_major - 1).astype(np.float32))
        lo = np.where(np.isnan(lo), F(0), lo)
        hi = np.where(np.isnan(hi), (n_major - 1).astype(np.float32), hi)
    cnt = np.where(alive & (lo <= hi), hi.astype(np.int64) - lo.astype(np.int64) + 1, 0)
    total = int(cnt.sum())
    if total == 0:
        return empty
    seg = np.repeat(np.arange(prim.size), cnt)
    first = np.cumsum(cnt) - cnt
    i = lo.astype(np.int64)[seg] + (np.arange(total) - first[seg])
    S0, S1, O0, O1, AZ, BZ, XM = s0[seg], s1[seg], o0[seg], o1[seg], az[seg], bz[seg], xmajor[seg]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c = i.astype(np.float32) + F(0.5)
        on = np.where(S1 > S0, (c >= S0) & (c < S1), (c <= S0) & (c > S1))
        DS, DM = (S1 - S0).astype(np.float32), (O1 - O0).astype(np.float32)
        t = ((c - S0) / DS).astype(np.float32)
        m = np.floor((O0 + (DM * t).astype(np.float32)).astype(np.float32))
        tz = ((((c - S0) * DS).astype(np.float32) + (((m + F(0.5)) - O0).astype(np.float32) * DM).astype(np.float32)).astype(np.float32)
              / ((DS * DS).astype(np.float32) + (DM * DM).astype(np.float32)).astype(np.float32)).astype(np.float32)   # eq. 14.5, as overlay_reference
        z = (AZ + ((BZ - AZ) * tz).astype(np.float32)).astype(np.float32)
        on &= (m >= 0) & (m < n_minor[seg]) & ~np.isnan(z)
        z = np.where(z > 0, z, F(0)).astype(np.float32)
        z = np.where(z < 1, z, F(1)).astype(np.float32)
    i, m, z, XM, seg = i[on], m[on].astype(np.int64), z[on], XM[on], seg[on]
    return prim[seg], np.where(XM, i, m), np.where(XM, m, i), z


def brick_winners(ids, res_bricks, brick_size, bbox_min, mv, pr, view, fb_d):
    """per pixel the primitive index whose fragment the in-order GL_LESS keeps (-1: none passed) and the depth after the overlay;
    also (fragments inside the view, fragments that failed the strict test, pixels where the winner's depth was shared by another primitive)"""
    prim, px, py, z = brick_fragments(ids, res_bricks, brick_size, bbox_min, mv, pr, view)
    d = np.array(fb_d, np.float32, copy=True)
    win = np.full(d.shape, -1, np.int64)
    stats = dict(fragments=int(prim.size), failed=0, tie_pixels=0)
    if prim.size == 0:
        return win, d, stats
    ok = z < d[py, px]
    stats["failed"] = int((~ok).sum())
    prim, px, py, z = prim[ok], px[ok], py[ok], z[ok]
    pix = py * d.shape[1] + px
    order = np.lexsort((prim, z, pix))                                  # by pixel, then depth, then primitive index
    pix, prim, z = pix[order], prim[order], z[order]
    head = np.ones(pix.size, bool)
    head[1:] = pix[1:] != pix[:-1]
    h = np.flatnonzero(head)
    if pix.size > 1:
        nxt = h + 1
        nxt = nxt[nxt < pix.size]
        stats["tie_pixels"] = int(((pix[nxt] == pix[nxt - 1]) & (z[nxt] == z[nxt - 1])).sum())
    win.reshape(-1)[pix[h]] = prim[h]
    d.reshape(-1)[pix[h]] = z[h]
    return win, d, stats


def draw_bricks(flags_or_ids, res_bricks, brick_size, bbox_min, mv, pr, view, fb_c, fb_d, stats=None):
    """the framebuffer (colour [h][w][4], depth [h][w]) after the overlay; stats: a dict that receives brick_winners' counts and `bricks`"""
    ids = brick_ids(flags_or_ids, int(np.prod(res_bricks)))
    win, d, st = brick_winners(ids, res_bricks, brick_size, bbox_min, mv, pr, view, fb_d)
    c = np.array(fb_c, np.float32, copy=True)
    c[win >= 0] = WIRE_COLOR
    if stats is not None:
        stats.update(st, bricks=int(ids.size), changed=int((win >= 0).sum()))
    return c, d
