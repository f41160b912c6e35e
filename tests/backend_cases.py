"""Inputs, float64 references and the acceptance rule of the back-end tests, shared by tests/test_backend_reference.py (the oracle against
tests/backend_reference.py, no GPU) and tests/test_gpu_backends.py (kernels and oracle against it).  HIP-free.

The acceptance rule is main_path_cases.compare: a pixel is excluded only where the reference's own margin is below its bound; every other
pixel must agree; the excluded share must stay under the cap; enough pixels must have been compared.  The reference's margin has four terms
(backend_reference.TERMS), each with its own bound; the margin handed to compare() is the smallest term / bound ratio, so its bound is 1.
The references are computed once per input (functools.lru_cache) and never modified.

The quantities of a draw: coverage (depth < 1), window depth, rgb, alpha (1 where covered).  MVT has no CPU oracle; the side called
"oracle" there is the fp32 restatement tests/mvt_reference.draw_mvt, the one tests/test_gpu_mvt.py compares the kernels with.

Changes to the inputs the cases were first given, and why:
* the eye inside the cloud looks through a 140 degree field of view, not 50.  A triangle that reaches behind the eye and is still seen lies
  within about one triangle's length of the eye, however fine the grid: at 50 degrees no pose found more than 6 of them, at 120 degrees 19,
  where 20 are wanted.  The pose was picked by a random search over eyes inside the box and under the sphere's surface.
* MVT draws a 96x72 frame: its 13 x 13 bilateral filter wants 65 % of its taps on the surface and leaves no vertex of a 48x40 frame, and 109 of
  64x48, valid.
* the frontal and the oblique eye stand 0.9 to 1 m from the sphere's centre: min_length 0.05 rejects nearly half of the triangles, and only
  from there do the remaining ones still cover 800 pixels.
"""
import functools

import numpy as np

import backend_reference as B
import main_path_cases as MC
import mvt_reference as M
import rgbd_recon_amd as rr
from main_path_cases import close_abs, compare
from oracle.oracle import OracleRecon

S = rr.scene

# Measured on the CPU (print_measurements()), oracle against reference, over the cases of all_cpu_cases():
#   dev       largest deviation on non-excluded pixels                                   -> tol = 4 x dev, rounded up
#   need      per term of the margin, the largest value at which a side decides a pixel's coverage differently (a mismatch belongs to the term
#             that is smallest in units of PRIOR)                                        -> bound = 4 x need, rounded up; a term without any
#             mismatch gets 4 x PRIOR, the fp32 error of the operation behind it
#   excluded  largest share of excluded pixels of any case at those bounds (of the view for coverage, of the covered pixels otherwise)
# back-end   depth dev   colour dev   coverage mismatches   excluded (coverage / covered)
# trigrid    3.04e-6     2.24e-5      none                  0.04 % / 0.10 %     (the depth deviation is the eye inside, near plane 0.01)
# points     1.35e-7     9.22e-6      none                  0.49 % / 0.49 %     (all of it the z gap: sprites of mirrored points tie)
# mvt        2.39e-7     7.51e-6      none                  0.00 % / 0.00 %
# The oracle decides no pixel's coverage otherwise than the reference, at any margin: every bound is 4 x PRIOR.
PRIOR = dict(edge=2e-5,     # pixels: window coordinates up to 128 carry ulps of 7.6e-6, an edge function a few of them
             test=2.5e-7,   # operands of magnitude 1 (positions in metres, texture coordinates, a dot product of unit vectors, window z): 2 ulp
             eps=4e-5,      # metres: position_curr_es is unprojected from window z; d z_eye / d z_window = z_eye^2 / near reaches 200 at a near plane
                            # of 0.01 and 1.5 m, times the 1.2e-7 of z, plus the interpolated pos_es
             zgap=2.5e-7)   # window z just below 1: 2 ulp each side
TABLE = {
    "trigrid": dict(depth=1.3e-5, colour=9e-5, bounds=dict(edge=8e-5, test=1e-6, eps=1.6e-4, zgap=1e-6)),
    "mvt":     dict(depth=1e-6, colour=4e-5, bounds=dict(edge=8e-5, test=1e-6, eps=1.6e-4, zgap=1e-6)),
    "points":  dict(depth=6e-7, colour=4e-5, bounds=dict(edge=8e-5, test=1e-6, eps=1.6e-4, zgap=1e-6)),
}
ATOMIC_ORDER = 2e-5        # tests/test_gpu_trigrid.py: the kernels' blend adds in arrival order; on top of the colour tolerance, for the kernels only
CAP = 0.05                 # conditions, not measurements: the excluded share of the view's pixels (coverage) resp. of the covered pixels
MIN_PIXELS = 800           # compared per case and quantity
MIN_BEHIND = 20

KW = dict(res=(16, 16, 16), brick_size=[2.0 / 8, 2.2 / 8, 2.0 / 8], limit=0.04)
FRAMES = {"landscape": (48, 40), "portrait": (40, 48), "large": (64, 48),       # portrait: the swapped loop bounds run off the other axis
          "mvt": (96, 72),
          # the box moved to where stream 0 sees it in the band the swapped loop bounds leave out: columns >= 40 resp. rows >= 40 (asserted)
          "landscape band": (48, 40, (0.3, 0.4, -0.8)), "portrait band": (40, 48, (0.8, 1.9, 0.0))}
EYES = {"frontal": ((0.07, 1.17, 0.95), (0.0, 1.1, 0.0)),                       # (off the scene's planes of symmetry: mirrored points tie in z)
        "near": ((0.04, 1.14, 0.72), (0.0, 1.1, 0.0)), "oblique": ((0.62, 1.55, 0.62), (0.0, 1.0, 0.0)),
        "inside": ((0.475, 0.407, 0.317), (0.74, 1.019, -0.428)),               # inside the box, under its top
        "close": ((0.1, 1.2, 0.72), (0.0, 1.1, 0.0)),
        "landscape band": ((-0.11, 0.27, -0.95), (0.3, 0.4, -0.8)), "portrait band": ((0.39, 2.09, -0.08), (0.8, 1.9, 0.0))}
# (the band eyes stand 0.45 m BEHIND the moved box as stream 0 sees it: with these images' v axis pointing up, the fragment shader's back-face test
# keeps the side of a surface that faces away from its sensor)                           # 0.27 m off the sphere: sprites of tens of pixels
LENS = {"inside": (140.0, 0.01)}                                                # (field of view, near plane); everyone else (50, 0.1)

# name -> (frame, view, eye, min_length, shade modes)
TRIGRID_CASES = {
    "landscape frontal": ("landscape", (96, 54), "frontal", 0.1, (0, 1, 3)),
    "landscape oblique": ("landscape", (101, 57), "oblique", 0.05, (0, 1, 3)),
    "portrait oblique": ("portrait", (96, 54), "oblique", 0.1, (0, 3)),
    "portrait frontal": ("portrait", (101, 57), "frontal", 0.1, (1,)),      # (its coarser grid: 0.05 accepts 2 % of it)
    "large frontal": ("large", (101, 57), "frontal", 0.05, (0,)),
    "inside": ("landscape", (96, 54), "inside", 0.1, (0, 3)),
    "landscape band": ("landscape band", (96, 54), "landscape band", 0.1, (3,)),
    "portrait band": ("portrait band", (101, 57), "portrait band", 0.1, (3,)),
}
ACCEPTED_SHARE = {0.1: (0.60, 1.0), 0.05: (0.15, 0.85)}                         # of the triangles with three valid depths, on the reference alone
POINTS_CASES = {
    "landscape frontal": ("landscape", (96, 54), "frontal", None, (0, 1, 2, 3)),
    "portrait oblique": ("portrait", (101, 57), "oblique", None, (0, 1, 2, 3)),
    "large close": ("large", (101, 57), "close", None, (0, 1, 2, 3)),
}
MVT_CASES = {"near": ("mvt", (96, 54), "near", 0.1, (0, 3))}                    # (the filter leaves the middle of the sphere: from nearer, 800 pixels)


@functools.lru_cache(maxsize=None)
def scene(frame):
    w, h = FRAMES[frame][:2]
    return S.make_scene(n_streams=3, width=w, height=h, lut_res=16, inv_res=8, box_c=(FRAMES[frame] + (None,))[2])


def matrices(eye, view):
    fov, near = LENS.get(eye, (50.0, 0.1))
    return S.gl_flat(S.look_at(*EYES[eye])), S.gl_flat(S.perspective(fov, view[0] / float(view[1]), near, 200.0))


def _frozen(t):
    for a in t:
        a.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def trigrid_grid(name):
    frame, view, eye, ml, _ = TRIGRID_CASES[name]
    return B.trigrid(scene(frame), *matrices(eye, view), view, ml)


@functools.lru_cache(maxsize=None)
def trigrid_reference(name, mode):
    return _frozen(trigrid_grid(name).resolve(mode))


@functools.lru_cache(maxsize=None)
def points_reference(name, mode):
    frame, view, eye, _, _ = POINTS_CASES[name]
    stats = {}
    return _frozen(B.draw_points(scene(frame), scene(frame)["normals"], *matrices(eye, view), view, mode, stats)) + (stats,)


@functools.lru_cache(maxsize=None)
def mvt_vertices(frame):
    """the vertex stage's (filtered depth, lateral quality): tests/test_mvt_reference.py and tests/test_gpu_mvt.py hold it on its own"""
    v = M.vertex_stage(scene(frame)["depth_raw"])
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def mvt_grid(name):
    frame, view, eye, ml, _ = MVT_CASES[name]
    return B.mvt_raster(scene(frame), mvt_vertices(frame), *matrices(eye, view), view, ml)


@functools.lru_cache(maxsize=None)
def mvt_reference(name, mode):
    return _frozen(mvt_grid(name).resolve(mode))


# ---------------------------------------------------------------------------------------------------------------- the acceptance rule
NEED = None                # print_measurements() sets a dict: per back-end and term, the largest margin of a coverage mismatch


def check_draw(kind, what, ref, sides):
    """ref: (rgba, depth, margin [h][w][4]) of backend_reference; sides: {"kernel ...": (rgba, depth), "oracle": ...} framebuffers.  Returns the
    number of covered pixels compared."""
    rgba, depth, margin = ref[:3]
    t = TABLE[kind]
    bounds = np.array([t["bounds"][k] for k in B.TERMS])
    ex = (margin < bounds).any(-1)
    ratio = (margin / bounds).min(-1)
    covered = depth < 1.0
    kw = dict(excluded=ex, minimum=0 if MC.MEASURE is not None else MIN_PIXELS)
    got_c = {k: np.asarray(v[0], np.float64) for k, v in sides.items()}
    got_d = {k: np.asarray(v[1], np.float64) for k, v in sides.items()}
    if NEED is not None:
        _record_need(kind, margin, covered, got_d)
    compare(f"{kind} coverage: {what}", covered, ratio, 1.0, CAP, {k: d < 1.0 for k, d in got_d.items()}, lambda a, b: a == b, **kw)
    compare(f"{kind} depth: {what}", depth, ratio, 1.0, CAP, got_d, close_abs(t["depth"]), count=covered, **kw)
    for k, c in got_c.items():
        tol = t["colour"] + (ATOMIC_ORDER if k.startswith("kernel") and kind != "points" else 0.0)
        compare(f"{kind} colour: {what}", rgba[..., :3], ratio, 1.0, CAP, {k: np.where(covered[..., None], c[..., :3], 0.0)}, close_abs(tol), count=covered, **kw)
    compare(f"{kind} alpha: {what}", rgba[..., 3], ratio, 1.0, CAP, {k: np.where(covered, c[..., 3], 0.0) for k, c in got_c.items()}, lambda a, b: a == b, count=covered, **kw)
    return int((covered & ~ex).sum())


def _record_need(kind, margin, covered, got_d):
    prior = np.array([PRIOR[k] for k in B.TERMS])
    for d in got_d.values():
        bad = (d < 1.0) != covered
        if bad.any():
            m = margin[bad]
            term = (m / prior).argmin(-1)
            for i, k in enumerate(B.TERMS):
                if (term == i).any():
                    NEED.setdefault(kind, {}).setdefault(k, 0.0)
                    NEED[kind][k] = max(NEED[kind][k], float(m[term == i, i].max()))


# ---------------------------------------------------------------------------------------------------------------- ties
EXACT_VIEW = (64, 64)


@functools.lru_cache(maxsize=None)
def exact_scene():
    """A 32x32 frame whose grid projects onto window coordinates 8.5 + 1.5 i: every other vertex on a pixel centre, vertical, horizontal and
    diagonal edges through pixel centres.  Sizes are powers of two and every value has a few fraction bits, so LUT fetches, transforms and edge
    functions are exact in fp32 and in float64 alike: a pixel centre ON an edge is on it for everyone, and only the top-left rule says whose it is.
    Stream 0 is a plane of depth 0.5, seen by the orthographic matrices of exact_matrices(); the other streams are invalid (depth -1)."""
    sc = dict(S.make_scene(n_streams=3, width=32, height=32, lut_res=16, inv_res=8))
    c = (np.arange(16) + 0.5) / 16.0
    _, v, u = np.meshgrid(c, c, c, indexing="ij")
    xyz = np.stack([-0.7578125 + 1.5 * u, 0.3671875 + 1.5 * v, np.full(u.shape, 0.25)], -1).reshape(-1, 3)
    sc["cv_xyz"] = np.ascontiguousarray(np.stack([xyz] * 3), np.float32)
    depth = np.full((3, 32, 32, 2), -1.0, np.float32)
    depth[0, ..., 0] = 0.5
    depth[0, 5:9, 20:27, 0] = -1.0                           # a hole, for inner silhouettes
    sc["depth"] = depth
    sc["quality"] = np.ones((3, 32, 32), np.float32)
    return sc


def exact_matrices():
    """eye space = camera space moved down by 1.125; clip = (x, y, -z / 2, 1): window x = 32 + 32 x, window z = 0.4375 on the plane"""
    mv, pr = np.eye(4), np.diag([1.0, 1.0, -0.5, 1.0])
    mv[1, 3] = -1.125
    return S.gl_flat(mv), S.gl_flat(pr)


def exact_case(make):
    """the grid and the sprites of exact_scene().  GL asks that a pixel centre on the common edge of two triangles be produced by exactly one
    of them and leaves open by which (OpenGL 4.4, 14.6.1): the reference owns left and top edges, the oracle and the kernels right and top ones.
    So a centre on an edge of the mesh's OUTLINE may go either way and is excluded; one on an edge INSIDE the mesh (all eight neighbours covered)
    must be covered, whichever triangle takes it; every other pixel must agree.  The sprites' boundary rule is the oracle's header's: no exclusion."""
    sc = exact_scene()
    objs = make(sc, view=EXACT_VIEW, **KW)
    mv, pr = exact_matrices()
    rgba, depth, margin = B.draw_trigrid(sc, mv, pr, EXACT_VIEW, 0.1, 3)
    cov = depth < 1.0
    pad = np.pad(cov, 1)
    inner = np.logical_and.reduce([pad[1 + dy:pad.shape[0] - 1 + dy, 1 + dx:pad.shape[1] - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    tie = margin[..., B.EDGE] == 0.0
    assert int((tie & inner).sum()) >= 300 and int((tie & ~inner).sum()) >= 1, "too few pixel centres on edges"
    for o in objs.values():
        o.setMinLength(0.1)
        o.setShadeMode(3)
        o.drawTrigrid(mv, pr)
    open_ = tie & ~inner
    never = np.zeros(depth.shape, bool)
    sides = {k: o.framebuffer() for k, o in objs.items()}
    compare("trigrid coverage: exact grid", cov, margin[..., B.EDGE], 0.0, 1.0, {k: v[1] < 1.0 for k, v in sides.items()}, lambda a, b: a == b, excluded=open_, minimum=3800)
    compare("trigrid depth: exact grid", depth, margin[..., B.EDGE], 0.0, 1.0, {k: np.asarray(v[1], np.float64) for k, v in sides.items()}, close_abs(TABLE["trigrid"]["depth"]), excluded=open_)
    rgba, depth, margin = B.draw_points(sc, sc["normals"], mv, pr, EXACT_VIEW, 3)
    for o in objs.values():
        o.upload_normals(sc["normals"])
        o.drawPoints(mv, pr)
    sides = {k: o.framebuffer() for k, o in objs.items()}
    compare("points coverage: exact grid", depth < 1.0, margin[..., B.EDGE], 0.0, 0.0, {k: v[1] < 1.0 for k, v in sides.items()}, lambda a, b: a == b, excluded=never, minimum=4096)
    return int((tie & inner).sum())


# ---------------------------------------------------------------------------------------------------------------- drivers
class MvtRestatement:
    """tests/mvt_reference.draw_mvt behind the draw calls' names: the fp32 side of the MVT cases where no kernel runs"""

    def __init__(self, scene, view=None, **kw):
        self.scene, self.view, self.mode, self.ml = scene, tuple(view), 0, 0.0125
        self._orc = OracleRecon(scene, view=view, **kw)                     # draw()'s image_to_eye, as the library forms it

    def upload_raw_frame(self, scene): self.vtx = M.vertex_stage(scene["depth_raw"])
    def setShadeMode(self, m): self.mode = int(m)
    def setMinLength(self, v): self.ml = float(v)

    def drawMVT(self, mv, pr):
        i2e = self._orc.view_matrices(mv, pr)[0]
        self._fb = M.draw_mvt(self.scene, self.vtx, mv, pr, self.view, i2e, min_length=self.ml, shade_mode=self.mode)

    def framebuffer(self): return self._fb


def only_oracle(scene, mvt=False, **kw):
    return {"oracle": (MvtRestatement if mvt else OracleRecon)(scene, **kw)}


def trigrid_case(make, name):
    frame, view, eye, ml, modes = TRIGRID_CASES[name]
    objs = make(scene(frame), view=view, **KW)
    mv, pr = matrices(eye, view)
    st = trigrid_grid(name).stats
    share = st["accepted"] / float(st["depth_valid"])
    lo, hi = ACCEPTED_SHARE[ml]
    assert lo < share < hi or (share == hi == 1.0), f"trigrid {name}: min_length {ml} accepts {share:.0%} of the triangles with valid depths"
    if frame.endswith("band"):
        d, n = scene(frame)["depth"][..., 0], min(FRAMES[frame][:2])
        left_out = int(((d[:, :, n:] if d.shape[2] > n else d[:, n:, :]) > 0).sum())
        assert left_out >= 25, f"trigrid {name}: only {left_out} valid depth pixels in the band the vertex buffer leaves out"
    if eye == "inside":
        assert st["behind"] >= MIN_BEHIND, f"trigrid {name}: only {st['behind']} accepted triangles reach behind the eye and are still seen"
    for mode in modes:
        for o in objs.values():
            o.setMinLength(ml)
            o.setShadeMode(mode)
            o.drawTrigrid(mv, pr)
        check_draw("trigrid", f"{name} mode {mode}", trigrid_reference(name, mode), {k: o.framebuffer() for k, o in objs.items()})
    return st


def points_case(make, name):
    frame, view, eye, _, modes = POINTS_CASES[name]
    sc = scene(frame)
    objs = make(sc, view=view, **KW)
    mv, pr = matrices(eye, view)
    for mode in modes:
        for o in objs.values():
            o.upload_normals(sc["normals"])
            o.setShadeMode(mode)
            o.drawPoints(mv, pr)
        ref = points_reference(name, mode)
        if eye == "close":
            assert ref[3]["largest"] >= (8.0 if mode == 3 else 20.0), f"points {name}: the largest sprite is {ref[3]['largest']:.1f} pixels"
            assert ref[3]["centre_dropped"] >= 1, f"points {name}: no point is dropped by its centre while its square reaches into the view"
        check_draw("points", f"{name} mode {mode}", ref, {k: o.framebuffer() for k, o in objs.items()})


def mvt_case(make, name):
    frame, view, eye, ml, modes = MVT_CASES[name]
    sc = scene(frame)
    objs = make(sc, mvt=True, view=view, **KW)
    mv, pr = matrices(eye, view)
    for mode in modes:
        for o in objs.values():
            o.upload_raw_frame(sc)
            o.setMinLength(ml)
            o.setShadeMode(mode)
            o.drawMVT(mv, pr)
        check_draw("mvt", f"{name} mode {mode}", mvt_reference(name, mode), {k: o.framebuffer() for k, o in objs.items()})


def all_cpu_cases():
    for name in TRIGRID_CASES:
        yield trigrid_case, name
    for name in POINTS_CASES:
        yield points_case, name
    for name in MVT_CASES:
        yield mvt_case, name


def print_measurements():
    """python -c 'import backend_cases as C; C.print_measurements()' from tests/: what TABLE was filled from"""
    global NEED
    MC.MEASURE, NEED = {}, {}
    try:
        for f, name in all_cpu_cases():
            f(only_oracle, name)
    finally:
        m, need, MC.MEASURE, NEED = MC.MEASURE, NEED, None, None
    for k, v in m.items():
        print(f"{k:18s} draws {v['cases']:3d}  dev {v['dev']:.3g}  worst exact mismatch at {v['need']:.3g} of its bound  excluded {v['excluded']:.2%}")
    for kind, terms in need.items():
        print(f"{kind:18s} coverage decided differently at margins up to " + ", ".join(f"{k} {v:.3g}" for k, v in terms.items()))
    return m, need
