"""Inputs, float64 references and the acceptance rule of the overlay tests, shared by tests/test_overlay_gl_reference.py (the fp32 twins against
tests/overlay_gl_reference.py, no GPU) and tests/test_gpu_overlay_gl_reference.py (kernels and twins against it).  HIP-free.

The acceptance rule is main_path_cases.compare.  The compared set is the reference's `touched`.  An untouched pixel must equal the framebuffer
before the overlay bit for bit, colour and depth, with no margin; the two texture draws must leave every depth alone.  A touched pixel is
excluded only where one term of the reference's own margin (overlay_gl_reference.TERMS) is below its bound; on every other touched pixel
coverage (did the overlay write it) and the winner's colour agree exactly for the uniform-colour line draws, depth and the computed colours
(calibvis, blit, sensor windows) within a tolerance.  The margin handed to compare() is the smallest term / bound ratio, so its bound is 1.

Every input is made on the CPU -- the oracle's drawF framebuffer, fused volume, counters, atlas and depth-limit image, or a random framebuffer --
and a kernel is handed the same arrays (set_framebuffer, set_tsdf, set_counters), so a reference is computed once per input
(functools.lru_cache) and never modified.  The sensor windows alone read what their side holds (the pre-processing products of the oracle or
of the library, which tests/test_gpu_preprocess.py pins to each other); their reference is cheap and computed per call.

Changes to the cases as first listed, and why:
* the bricks shorter than a pixel are seen through a 140 degree lens from inside the box, among bricks that are many pixels long: with sub-pixel
  bricks alone every drawn pixel holds a segment's end point, all of them are `open`, and the case could not stay under its cap.
* the fused frame's NaN voxels (no stream saw them) are set to the cleared -limit before calibvis samples it: a NaN sample passes all three
  comparisons of calib_vis.fs as false and is drawn with a NaN colour, which GLSL leaves undefined (margin 0) -- a fifth of the touched pixels.
* the crafted calibvis volume keeps its blocks at exactly -0.01, 0 and 0.01: a sample whose eight taps are equal is data (the filter weights sum
  to one), so the reference gives it no margin and the case stays under its cap with a third of its points on a threshold.
"""
import functools

import numpy as np

import brick_overlay_reference as TB
import client_overlay_reference as TC
import main_path_cases as MC
import overlay_gl_reference as G
import overlay_reference as TO
import rgbd_recon_amd as rr
import sensor_view_reference as TS
from helpers import same
from main_path_cases import Mismatch, close_abs, compare
from oracle.oracle import OracleRecon, frustum

S = rr.scene

# Measured on the CPU (print_measurements()), twin against reference, over the cases of all_cpu_cases():
#   dev       largest deviation on non-excluded touched pixels                             -> tol = 4 x dev, rounded up
#   need      per term of the margin, the largest value at which the twin decides a pixel's coverage or winner differently (a mismatch belongs
#             to the term that is smallest in units of PRIOR)                              -> bound = 4 x need, rounded up; a term without any
#             mismatch gets 4 x PRIOR, the fp32 error of the operation behind it
#   excluded  largest share of a case's touched pixels that those bounds exclude (cap: what the share may never pass)
# draw       depth dev   colour dev   coverage / winner decided differently at      excluded   cap
# calibvis   6.83e-8     1.13e-7      test 6.21e-8 (the crafted depth ties)            3.16 %     5 %
# frustums   1.55e-7     exact        edge 9.42e-7, and at `open` pixels               8.48 %    10 %    (front eye: a frustum edge along a pixel row boundary)
# bbox       7.96e-8     exact        at `open` pixels only                            5.16 %    10 %
# bricks     1.96e-6     exact        at `open` pixels only                            7.16 %    10 %    (both figures: the 140 degree lens, near plane 0.05)
# blit       -           8.67e-6      (no decision)                                    0.00 %     0 %
# sensor     -           7.61e-6      none                                             3.81 %     5 %    (quad edges on pixel centres: RECT's y 2.5)
# No mismatch lies above 4 x PRIOR, so every bound is 4 x PRIOR.  The twins stand in for the kernels, which the bit-for-bit tests hold equal to them.
PRIOR = dict(edge=2e-5,     # pixels: window coordinates up to 173 carry ulps of 1.5e-5; end points of clipped lines lie further out
             test=2.5e-7,   # window z just below 1 against an fp32 depth: 2 ulp each side; NDC at +-1 alike; d of 0.01 carries far less
             zgap=2.5e-7,   # window z just below 1: 2 ulp each side
             open=1.0)      # (0 or infinite)
# (the sensor windows' test term is a NEAREST texel coordinate of up to 160 texels: 4 x 2.5e-6)
TABLE = {
    "calibvis": dict(depth=2.8e-7, colour=4.6e-7, bounds=dict(edge=8e-5, test=1e-6, zgap=1e-6, open=1.0), cap=0.05, uniform=False),
    "frustums": dict(depth=6.2e-7, colour=0.0, bounds=dict(edge=8e-5, test=1e-6, zgap=1e-6, open=1.0), cap=0.10, uniform=True),
    "bbox":     dict(depth=3.2e-7, colour=0.0, bounds=dict(edge=8e-5, test=1e-6, zgap=1e-6, open=1.0), cap=0.10, uniform=True),
    "bricks":   dict(depth=7.9e-6, colour=0.0, bounds=dict(edge=8e-5, test=1e-6, zgap=1e-6, open=1.0), cap=0.10, uniform=True),
    "blit":     dict(depth=0.0, colour=3.5e-5, bounds=dict(edge=8e-5, test=1e-6, zgap=1e-6, open=1.0), cap=0.0, uniform=False),
    "sensor":   dict(depth=0.0, colour=3.1e-5, bounds=dict(edge=8e-5, test=1e-5, zgap=1e-6, open=1.0), cap=0.05, uniform=False),
}
MIN_PIXELS = 300           # touched pixels compared per line and point draw: a condition, not a measurement

VIEW = (173, 99)           # no multiple of 8, 16 or 64; wider than two 64-lane strides of the line walker
KW = dict(res=(64, 64, 64), brick_size=[2.0 / 4, 2.2 / 4, 2.0 / 4], limit=0.04, view=VIEW)         # 4 bricks per axis
KW_TINY = dict(KW, brick_size=[2.0 / 16, 2.2 / 16, 2.0 / 16])
CENTRE = (0.0, 1.1, 0.0)
# name -> (eye, at, field of view, near, far)
EYES = {
    "front":   ((0.0, 1.1, 3.0), CENTRE, 50.0, 0.1, 200.0),              # the three eyes of tests/test_gpu_overlays.py
    "oblique": ((1.6, 1.4, 2.4), CENTRE, 50.0, 0.1, 200.0),
    "behind":  ((-2.2, 2.6, -1.5), CENTRE, 50.0, 0.1, 200.0),
    "inside":  ((0.78, 1.93, 0.78), (-0.51, 1.32, -0.13), 70.0, 0.3, 200.0),  # inside the box and inside frusta (a random search): segments cross the near plane
    "far_cut": ((0.3, 1.3, 3.0), CENTRE, 50.0, 0.1, 3.2),                # the far plane cuts the box
    "sides":   ((-0.12, 2.05, 0.72), (0.69, 0.86, -0.01), 70.0, 0.1, 200.0),   # under the box's top (found by a random search over eyes inside it): segments of
                                                                           # every line draw leave through each of the four sides, others lie wholly outside or end at w <= 0
    "tiny":    ((-0.9, 0.1, 0.9), (0.6, 1.9, -0.8), 140.0, 0.05, 200.0), # from a corner of the box through a wide lens: far bricks under a pixel
}


def matrices(eye):
    e, at, fov, near, far = EYES[eye]
    return S.gl_flat(S.look_at(e, at)), S.gl_flat(S.perspective(fov, VIEW[0] / float(VIEW[1]), near, far))


@functools.lru_cache(maxsize=None)
def scene(kind="small"):
    """'small': the suite's small_scene (volume 64^3 under KW, LUT 32^3, inverse grid 32^3, streams 160 x 120); 'grid16': two streams and an
    inverse grid of 16^3; 'colour': colour images of 200 x 88 beside depth of 160 x 120"""
    if kind == "small":
        return MC.small_scene()
    if kind == "grid16":
        return S.make_scene(n_streams=2, width=160, height=120, lut_res=32, inv_res=16)
    return S.make_scene(n_streams=2, width=160, height=120, lut_res=24, inv_res=24, color_width=200, color_height=88)


def kw_of(kind):
    """the context's parameters: under 'grid16' the limit is 0.005, so the cleared -0.005 lies above calib_vis.fs's -0.01 and every empty cell is drawn"""
    return dict(KW, limit=0.005) if kind == "grid16" else KW


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def oracle_frame(kind, eye):
    """the oracle's frame of scene(kind) seen from `eye`: dict(fb=(rgba, depth), volume, counters, occupied, atlas, peels)"""
    o = OracleRecon(scene(kind), **kw_of(kind))
    mv, pr = matrices(eye)
    o.clearOccupiedBricks(); o.markBricks(); o.updateOccupiedBricks(); o.integrate(); o.drawF(mv, pr)
    out = dict(fb=_frozen(*o.framebuffer()), volume=_frozen(o.tsdf())[0], counters=_frozen(o.counters())[0],
               occupied=_frozen(np.sort(o.occupied().astype(np.int64)))[0], atlas=_frozen(o.atlas()[0])[0], peels=_frozen(o.view_images()[3])[0],
               res_bricks=tuple(int(v) for v in o.res_bricks), brick_size=[float(v) for v in np.asarray(o.brick_size).reshape(-1)])
    assert (out["fb"][1] < 1).sum() > 300, "the frame shows nothing"
    return out


@functools.lru_cache(maxsize=None)
def framebuffer(kind, eye):
    """'drawF': the oracle's; 'random': colours in (0, 1), depth in (0.5, 1); 'clear': black, depth 1"""
    if kind == "drawF":
        return oracle_frame("small", eye)["fb"]
    if kind == "clear":
        return _frozen(np.zeros((VIEW[1], VIEW[0], 4), np.float32), np.ones((VIEW[1], VIEW[0]), np.float32))
    rng = np.random.default_rng(sum(map(ord, eye)))
    return _frozen(rng.uniform(0, 1, (VIEW[1], VIEW[0], 4)).astype(np.float32), rng.uniform(0.5, 1.0, (VIEW[1], VIEW[0])).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- the acceptance rule
NEED = None                # print_measurements() sets a dict: per draw and term, the largest margin of a coverage / winner mismatch
STATS = None               # ... and a dict: per draw the compared pixels, excluded share and deviations of every case
SEEN = {}                  # (draw, side) -> [largest depth deviation, largest colour deviation] on compared pixels so far: what a test may print


def check(kind, what, ref, before, sides, depth_free=False):
    """ref: (rgba, depth, margin, touched) of overlay_gl_reference; before: the framebuffer (rgba, depth) the overlay was drawn over;
    sides: {"kernel": (rgba, depth), "twin": ...}.  Returns (touched pixels compared, excluded share)."""
    rgba, depth, margin, touched = ref
    fb_c, fb_d = before
    t = TABLE[kind]
    bounds = np.array([t["bounds"][k] for k in G.TERMS])
    ex = (margin < bounds).any(-1)
    ratio = (margin / bounds).min(-1)
    for k, (c, d) in sides.items():                                          # untouched: bit for bit, no margin
        keep = np.ones_like(touched) if depth_free else ~touched
        bad_d, bad_c = keep & ~same(d, fb_d), ~touched & ~same(c, fb_c).all(-1)
        if bad_d.any() or bad_c.any():
            at = tuple(np.argwhere(bad_d | bad_c)[0])
            raise Mismatch(f"{kind}: {what}: the {k} changes {int(bad_d.sum())} depths and {int(bad_c.sum())} colours the reference leaves alone, e.g. at (row, column) {at}")
    got_c = {k: np.asarray(v[0], np.float64) for k, v in sides.items()}
    got_d = {k: np.asarray(v[1], np.float64) for k, v in sides.items()}
    minimum = 0 if MC.MEASURE is not None or depth_free else MIN_PIXELS
    kw = dict(excluded=ex, count=touched)
    if not depth_free:
        covered = depth != np.asarray(fb_d, np.float64)                      # GL_LESS: a written pixel's depth went down
        got_cov = {k: d != np.asarray(fb_d, np.float64) for k, d in got_d.items()}
        if NEED is not None:
            _record_need(kind, margin, [(g != covered) | ((g & covered) & (got_c[k] != rgba).any(-1) & t["uniform"]) for k, g in got_cov.items()])
        compare(f"{kind} coverage: {what}", covered, ratio, 1.0, t["cap"], got_cov, lambda a, b: a == b, minimum=minimum, **kw)
        compare(f"{kind} depth: {what}", depth, ratio, 1.0, t["cap"], got_d, close_abs(t["depth"]), **kw)
    agree = (lambda a, b: a == b) if t["uniform"] else close_abs(t["colour"])
    _, n = compare(f"{kind} colour: {what}", rgba, ratio, 1.0, t["cap"], got_c, agree, **kw)
    share = float((ex & touched).sum()) / max(int(touched.sum()), 1)
    keep = touched & ~ex
    for k in sides:
        s = SEEN.setdefault((kind, k), [0.0, 0.0])
        s[0], s[1] = max(s[0], MC.deviation(got_d[k], depth, keep)), max(s[1], MC.deviation(got_c[k], rgba, keep))
    if STATS is not None:
        STATS.setdefault(kind, []).append(dict(what=what, compared=n, excluded=share,
                                               depth=max(MC.deviation(d, depth, keep) for d in got_d.values()),
                                               colour=max(MC.deviation(c, rgba, keep) for c in got_c.values())))
    return n, share


def _record_need(kind, margin, mismatches):
    prior = np.array([PRIOR[k] for k in G.TERMS])
    for bad in mismatches:
        if bad.any():
            m = margin[bad]
            term = (m / prior).argmin(-1)
            for i, k in enumerate(G.TERMS):
                if (term == i).any():
                    NEED.setdefault(kind, {}).setdefault(k, 0.0)
                    NEED[kind][k] = max(NEED[kind][k], float(m[term == i, i].max()))


# ---------------------------------------------------------------------------------------------------------------- the sides
class Twins:
    """the four fp32 twins behind one interface: each method returns the framebuffer (rgba, depth) after the overlay"""

    def calibvis(self, sc, volume, mv, pr, fb):
        return TO.draw_calibvis(volume, sc["inv_res"], sc["bbox_min"], sc["bbox_max"], mv, pr, VIEW, *fb)

    def frustums(self, sc, mv, pr, fb):
        r = sc["lut_res"]
        corners = [TO.frustum_corners(sc["cv_xyz"][i], r) for i in range(sc["n"])]
        cams = [frustum(np.asarray(sc["cv_xyz"][i], np.float32).reshape(int(r[2]), int(r[1]), int(r[0]), 3))[1] for i in range(sc["n"])]
        return TO.draw_frustums(corners, cams, mv, pr, VIEW, *fb)

    def bbox(self, sc, mv, pr, fb):
        return TC.draw_bbox(sc["bbox_min"], sc["bbox_max"], mv, pr, VIEW, *fb)

    def bricks(self, sc, ids, res_bricks, brick_size, mv, pr, fb):
        return TB.draw_bricks(np.asarray(ids, np.int64), res_bricks, brick_size, sc["bbox_min"], mv, pr, VIEW, *fb)

    def blit(self, which, src, fb):
        return TC.blit(src, VIEW, fb[0]), np.array(fb[1], np.float32)

    def sensor(self, type, stream, layer, rect, clip, fb):
        return TS.draw(type, layer, rect, clip, fb[0]), np.array(fb[1], np.float32)


class Kernels:
    """the library behind the same interface: one context, handed the same inputs"""

    def __init__(self, hip):
        self.hip = hip

    def _draw(self, fb, call):
        self.hip.set_framebuffer(*fb)
        call()
        return self.hip.framebuffer()

    def calibvis(self, sc, volume, mv, pr, fb):
        self.hip.set_tsdf(volume)
        return self._draw(fb, lambda: self.hip.drawCalibVis(mv, pr))

    def frustums(self, sc, mv, pr, fb):
        return self._draw(fb, lambda: self.hip.drawFrustums(mv, pr))

    def bbox(self, sc, mv, pr, fb):
        return self._draw(fb, lambda: self.hip.drawBBox(mv, pr))

    def bricks(self, sc, ids, res_bricks, brick_size, mv, pr, fb):
        counters = np.zeros(int(np.prod(res_bricks)), np.uint32)
        counters[np.asarray(ids, np.int64)] = 50
        assert tuple(int(v) for v in self.hip.res_bricks) == tuple(res_bricks)
        self.hip.set_counters(counters)
        self.hip.updateOccupiedBricks()
        assert (np.flatnonzero(self.hip.bricks()[1]) == np.sort(np.asarray(ids, np.int64))).all(), "the library's occupied list is not the case's"
        return self._draw(fb, lambda: self.hip.drawOccupiedBricks(mv, pr))

    def blit(self, which, src, fb):
        """(the source is the library's own atlas / depth-limit image of the frame it drew last, which the bit-for-bit tests pin to the oracle's)"""
        return self._draw(fb, lambda: self.hip.drawTextures(which))

    def sensor(self, type, stream, layer, rect, clip, fb):
        return self._draw(fb, lambda: self.hip.drawSensorTexture(type, stream, rect, clip))


def only_twins(*_):
    return {"twin": Twins()}


# ---------------------------------------------------------------------------------------------------------------- line draws
# (eye, framebuffer) per line draw; every draw is seen over drawF's framebuffer and over a random one
LINE_CASES = [("front", "drawF"), ("oblique", "random"), ("behind", "drawF"), ("inside", "random"), ("far_cut", "clear"), ("sides", "random")]
TINY_CASE = ("tiny", "clear")


def census(segments, view=VIEW):
    """of clip-space segments [(a, b)]: how many cross the near plane, are cut by the far plane, lie wholly outside the view volume, have an end at
    w <= 0, and leave the view through its left / right / bottom / top side while drawn inside it"""
    out = dict(near=0, far=0, outside=0, behind=0, left=0, right=0, bottom=0, top=0, short=0)
    for a, b in segments:
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        out["near"] += int((a[2] + a[3] < 0) != (b[2] + b[3] < 0))
        out["far"] += int((a[3] - a[2] < 0) != (b[3] - b[2] < 0))
        out["behind"] += int(a[3] <= 0 or b[3] <= 0)
        r = G.clip_near_far(a, b)
        if r is None or not (r[0][3] > 0 and r[1][3] > 0):
            out["outside"] += 1
            continue
        wa, wb = G.to_window(r[0], view), G.to_window(r[1], view)
        if max(wa[0], wb[0]) < 0 or min(wa[0], wb[0]) > view[0] or max(wa[1], wb[1]) < 0 or min(wa[1], wb[1]) > view[1]:
            out["outside"] += 1
            continue
        out["short"] += int(np.abs(wb[:2] - wa[:2]).max() < 1.0)
        for key, axis, bound in (("left", 0, 0.0), ("right", 0, float(view[0])), ("bottom", 1, 0.0), ("top", 1, float(view[1]))):
            if (wa[axis] - bound) * (wb[axis] - bound) < 0:
                t = (bound - wa[axis]) / (wb[axis] - wa[axis])
                o = wa[1 - axis] + t * (wb[1 - axis] - wa[1 - axis])
                out[key] += int(0 <= o <= view[1 - axis])
    return out


def _expect(kind, eye, c):
    """the situations the eyes were chosen for really occur, on the reference's own geometry"""
    if eye == "inside":
        assert c["near"] >= 2, f"{kind} {eye}: {c}"
    if eye == "far_cut" and kind != "frustums":
        assert c["far"] >= 2, f"{kind} {eye}: {c}"
    if eye == "sides":
        assert min(c["left"], c["right"], c["bottom"], c["top"]) >= 1 and c["outside"] >= 1 and c["behind"] >= 1, f"{kind} {eye}: {c}"
    if eye == "tiny":
        assert c["short"] >= 50, f"{kind} {eye}: {c}"


@functools.lru_cache(maxsize=None)
def frustum_reference(eye, fb):
    sc = scene()
    mv, pr = matrices(eye)
    corners = [G.frustum_corners(sc["cv_xyz"][i], sc["lut_res"]) for i in range(sc["n"])]
    _expect("frustums", eye, census([(G.transform(mv, pr, c[i]), G.transform(mv, pr, c[j])) for c in corners for i, j in G.FRUSTUM_LINES]))
    return _frozen(*G.draw_frustums(corners, mv, pr, VIEW, *framebuffer(fb, eye)))


@functools.lru_cache(maxsize=None)
def bbox_reference(eye, fb):
    sc = scene()
    mv, pr = matrices(eye)
    _expect("bbox", eye, census([(G.transform(mv, pr, p), G.transform(mv, pr, q)) for p, q in G.bbox_segments(sc["bbox_min"], sc["bbox_max"])]))
    return _frozen(*G.draw_bbox(sc["bbox_min"], sc["bbox_max"], mv, pr, VIEW, *framebuffer(fb, eye)))


@functools.lru_cache(maxsize=None)
def brick_inputs(eye):
    """(ids ascending, res_bricks, brick_size): the bricks the oracle marks in small_scene (4 per axis), or for 'tiny' those of a 16-per-axis grid
    within 0.5 m of the eye (tens of pixels long through the 140 degree lens) and one in 80 of those further than 2.4 m (under a pixel)"""
    if eye != "tiny":
        f = oracle_frame("small", "front")
        return f["occupied"], f["res_bricks"], f["brick_size"]
    o = OracleRecon(scene(), **KW_TINY)
    res = tuple(int(v) for v in o.res_bricks)
    rx, ry = res[0], res[1]
    i = np.arange(int(np.prod(res)))
    centre = (np.stack([i % (rx * ry) % rx, i % (rx * ry) // rx, i // (rx * ry)], -1) + 0.5) * np.asarray(o.brick_size, np.float64) + np.asarray(scene()["bbox_min"], np.float64)
    dist = np.linalg.norm(centre - np.asarray(EYES["tiny"][0]), axis=-1)
    ids = np.flatnonzero((dist < 0.5) | ((dist > 2.4) & (np.random.default_rng(16).uniform(size=i.size) < 0.012)))
    return _frozen(ids)[0], res, [float(v) for v in np.asarray(o.brick_size).reshape(-1)]


@functools.lru_cache(maxsize=None)
def brick_reference(eye, fb):
    sc = scene()
    mv, pr = matrices(eye)
    ids, res, bs = brick_inputs(eye)
    assert len(ids) >= 8, "too few occupied bricks"
    segs = []
    for i in ids:
        z, rem = divmod(int(i), res[0] * res[1])
        y, x = divmod(rem, res[0])
        clip = G.transform(mv, pr, (np.array([x, y, z]) + G.R.CUBE) * np.asarray(bs) + np.asarray(sc["bbox_min"], np.float64))
        segs += [(clip[a], clip[b]) for a, b in G.CUBE_WIRE]
    _expect("bricks", eye, census(segs))
    return _frozen(*G.draw_bricks(ids, res, bs, sc["bbox_min"], mv, pr, VIEW, *framebuffer(fb, eye)))


def frustums_case(sides, eye, fb):
    mv, pr = matrices(eye)
    before = framebuffer(fb, eye)
    return check("frustums", f"eye {eye} over {fb}", frustum_reference(eye, fb), before, {k: s.frustums(scene(), mv, pr, before) for k, s in sides.items()})


def bbox_case(sides, eye, fb):
    mv, pr = matrices(eye)
    before = framebuffer(fb, eye)
    return check("bbox", f"eye {eye} over {fb}", bbox_reference(eye, fb), before, {k: s.bbox(scene(), mv, pr, before) for k, s in sides.items()})


def bricks_case(sides, eye, fb):
    mv, pr = matrices(eye)
    before = framebuffer(fb, eye)
    ids, res, bs = brick_inputs(eye)
    return check("bricks", f"eye {eye} over {fb}", brick_reference(eye, fb), before,
                 {k: s.bricks(scene(), ids, res, bs, mv, pr, before) for k, s in sides.items()})


# ---------------------------------------------------------------------------------------------------------------- calibvis
CALIBVIS_CASES = [("small", "real", "front", "drawF"), ("small", "real", "oblique", "random"), ("small", "crafted", "front", "ties"),
                  ("grid16", "real", "front", "clear")]


@functools.lru_cache(maxsize=None)
def calibvis_volume(kind, volume):
    """'real': the oracle's fused frame; 'crafted': the 2^3-block volume of test_calibvis_crafted_volume_and_framebuffer -- every colour
    branch, blocks at exactly -0.01, 0 and 0.01, a fifth of them random"""
    if volume == "real":
        v = oracle_frame(kind, "front")["volume"]
        return _frozen(np.where(np.isnan(v), np.float32(-kw_of(kind)["limit"]), v))[0]      # (see the module's docstring)
    rng = np.random.default_rng(3)
    values = np.array([-0.04, -0.01, -0.005, 0.0, 0.005, 0.01, 0.02], np.float32)
    blocks = rng.choice(values, size=(32, 32, 32)).astype(np.float32)
    mask = rng.random((32, 32, 32)) < 0.2
    blocks[mask] = rng.uniform(-0.03, 0.03, int(mask.sum()))
    return _frozen(np.kron(blocks, np.ones((2, 2, 2), np.float32)))[0]


@functools.lru_cache(maxsize=None)
def calibvis_framebuffer(kind, volume, eye, fb):
    """'ties': a random framebuffer whose depth equals, at every 97th visible point's pixel, that point's own fp32 window depth (GL_LESS fails)"""
    if fb != "ties":
        return framebuffer(fb, eye) if fb != "drawF" else oracle_frame(kind, eye)["fb"]
    sc = scene(kind)
    mv, pr = matrices(eye)
    c, d = [np.array(a) for a in framebuffer("random", eye)]
    ids, dist, ok, xw, yw, zw = TO.calibvis_points(calibvis_volume(kind, volume), sc["inv_res"], sc["bbox_min"], sc["bbox_max"], mv, pr, VIEW)
    n = 0
    for i in np.flatnonzero(ok)[::97]:
        for px, py in TO.point_pixels(xw[i], yw[i], 1, VIEW):
            d[py, px] = zw[i]
            n += 1
    assert n > 10
    return _frozen(c, d)


@functools.lru_cache(maxsize=None)
def calibvis_reference(kind, volume, eye, fb):
    sc = scene(kind)
    mv, pr = matrices(eye)
    vol = calibvis_volume(kind, volume)
    if volume == "crafted":
        _, d, data = G.calibvis_samples(vol, sc["inv_res"])
        lim = G.CALIB_LIMIT
        assert data.all() and all((d == v).any() for v in (-lim, 0.0, lim)) and ((d > 0) & (d < lim)).any() and ((d < 0) & (d > -lim)).any() and (d > lim).any()
    return _frozen(*G.draw_calibvis(vol, sc["inv_res"], sc["bbox_min"], sc["bbox_max"], mv, pr, VIEW, *calibvis_framebuffer(kind, volume, eye, fb)))


def calibvis_case(sides, kind, volume, eye, fb):
    mv, pr = matrices(eye)
    before = calibvis_framebuffer(kind, volume, eye, fb)
    vol = calibvis_volume(kind, volume)
    return check("calibvis", f"{kind} {volume} volume, eye {eye} over {fb}", calibvis_reference(kind, volume, eye, fb), before,
                 {k: s.calibvis(scene(kind), vol, mv, pr, before) for k, s in sides.items()})


# ---------------------------------------------------------------------------------------------------------------- the texture view
BLIT_EYE = "front"


def blit_case(sides, which, fb="random"):
    """unit 15 (which 0, the hole-filling atlas) or 16 (which 1, the depth-limit image) of the frame seen from BLIT_EYE.  A kernel side must
    have drawn that frame itself (drawF from BLIT_EYE) before this is called."""
    f = oracle_frame("small", BLIT_EYE)
    src = f["atlas"] if which == 0 else f["peels"]
    before = framebuffer(fb, BLIT_EYE)
    assert G.blit_viewport(*VIEW) == (129, 49)
    ref = G.blit(src, VIEW, *before)
    assert np.unique(ref[0][:49, :129, :3]).size > 50, "the source shows nothing"
    return check("blit", f"unit {15 + which} over {fb}", ref, before, {k: s.blit(which, src, before) for k, s in sides.items()}, depth_free=True)


# ---------------------------------------------------------------------------------------------------------------- the sensor windows
RECT = (3.25, 2.5, 3.25 + 40.0, 2.5 + 53.375)          # ImGui cursor positions are not integers
# name -> (types, stream, rect, clip)
SENSOR_CASES = {
    "all types":  (range(7), 0, RECT, None),
    "clip rect":  ((4, 5), 1, RECT, (10.0, 8.5, 30.75, 40.25)),
    "top left":   ((3, 0), 1, (-13.5, -20.25, 26.5, 33.0), None),                  # quads that leave the view (LINEAR types: this quad is 40 pixels wide, a
                                                                                   # third of the 120 texel rows, so every NEAREST coordinate would lie ON a texel boundary)
    "bottom right": ((2, 6), 1, (150.25, 70.0, 190.25, 123.375), None),
}


def sensor_check(sides, layers, type, stream, rect, clip, before, what):
    """layers: {side: the layer that side's window shows}; the reference is computed from each side's own layer"""
    n = share = 0
    for k, s in sides.items():
        ref = G.sensor_window(type, layers[k], rect, clip, *before)
        n, share = check("sensor", f"{what}: type {type} stream {stream}", ref, before, {k: s.sensor(type, stream, layers[k], rect, clip, before)}, depth_free=True)
        assert MC.MEASURE is not None or n >= MIN_PIXELS, f"sensor {what} type {type}: only {n} pixels compared"
    return n, share


def oracle_layers(kind):
    """{stream: {type: layer}} of the oracle's processTextures() on scene(kind)'s raw frame"""
    return _oracle_layers(kind)


@functools.lru_cache(maxsize=None)
def _oracle_layers(kind):
    sc = scene(kind)
    o = OracleRecon(sc, **KW)
    o.upload_raw_frame(sc)
    o.clearOccupiedBricks()
    o.processTextures()
    p = o.preprocessed()
    col = np.ascontiguousarray(sc["color"], np.uint8)
    return {s: {0: col[s], 1: p["depth_b"][s], 2: p["quality"][s], 3: p["normals"][s], 4: p["silhouette"][s], 5: p["depth2"][s], 6: p["lab"][s]}
            for s in range(sc["n"])}


def sensor_case(sides, layers_of, name, kind="small"):
    """layers_of(side name, stream) -> {type: layer}"""
    types, stream, rect, clip = SENSOR_CASES[name]
    before = framebuffer("random", name)
    out = []
    for type in types:
        layers = {k: layers_of(k, stream)[type] for k in sides}
        out.append(sensor_check(sides, layers, type, stream, rect, clip, before, f"{kind} {name}"))
    return out


def sensor_two_windows_case(sides, layers_of):
    """two windows side by side over a drawn frame, and a third over both: each over the framebuffer its side's twin left"""
    before = framebuffer("drawF", "front")
    w, h = [float(x) for x in TS.view_size(36.0, (160, 120))]
    for type, stream, rect in ((3, 0, (4.0, 4.0, 4.0 + w, 4.0 + h)), (0, 1, (4.0 + w + 2.0, 4.0, 4.0 + w + 2.0 + w, 4.0 + h)),
                               (5, 1, (20.75, 30.25, 20.75 + w, 30.25 + h))):     # (at x 20.5 every third column's NEAREST coordinate is an integer)
        layers = {k: layers_of(k, stream)[type] for k in sides}
        sensor_check(sides, layers, type, stream, rect, None, before, "two windows")
        first = next(iter(sides))
        before = Twins().sensor(type, stream, layers[first], rect, None, before)


# ---------------------------------------------------------------------------------------------------------------- all of it
def all_cpu_cases():
    for eye, fb in LINE_CASES:
        yield frustums_case, (eye, fb)
        yield bbox_case, (eye, fb)
        yield bricks_case, (eye, fb)
    yield bricks_case, TINY_CASE
    for c in CALIBVIS_CASES:
        yield calibvis_case, c
    for which in (0, 1):
        yield blit_case, (which,)


def print_measurements():
    """python -c 'import overlay_gl_cases as C; C.print_measurements()' from tests/: what TABLE was filled from"""
    global NEED, STATS
    MC.MEASURE, NEED, STATS = {}, {}, {}
    try:
        sides = only_twins()
        for f, a in all_cpu_cases():
            f(sides, *a)
        for kind in ("small", "colour"):
            for name in SENSOR_CASES:
                if kind == "small" or name == "all types":
                    sensor_case(sides, lambda k, s: oracle_layers(kind)[s], name, kind)
        sensor_two_windows_case(sides, lambda k, s: oracle_layers("small")[s])
    finally:
        m, need, stats, MC.MEASURE, NEED, STATS = MC.MEASURE, NEED, STATS, None, None, None
    for k, v in m.items():
        print(f"{k:18s} draws {v['cases']:3d}  dev {v['dev']:.3g}  worst exact mismatch at {v['need']:.3g} of its bound  excluded {v['excluded']:.2%}")
    for kind, terms in need.items():
        print(f"{kind:18s} decided differently at margins up to " + ", ".join(f"{k} {v:.3g}" for k, v in terms.items()))
    for kind, rows in stats.items():
        for r in rows:
            print(f"{kind:9s} {r['what']:48s} compared {r['compared']:5d}  excluded {r['excluded']:.2%}  depth dev {r['depth']:.3g}  colour dev {r['colour']:.3g}")
    return m, need, stats
