"""Inputs, float64 references and the acceptance rule of the main-path tests, shared by tests/test_main_path_reference.py (the oracle
against tests/main_path_reference.py, no GPU) and tests/test_gpu_main_path.py (kernels and oracle against it).  HIP-free.

Acceptance rule, the same everywhere: an element is excluded only where the reference's own margin is below the bound of TABLE; every other
element must agree; the share of excluded elements must stay under the cap; and enough elements must have been compared.  The references
are computed once per input (functools.lru_cache) and never modified.

The table above TABLE holds what was measured on the CPU, oracle against reference, over every case of this module (print_measurements()
repeats the measurement): the tolerances are 4 x the oracle's largest deviation on non-excluded elements (oracle and kernels are
bit-identical by construction, so the tolerance only has to absorb a future reordering of fp32 operations), the margin bounds 4 x the
smallest bound at which the oracle has no unexplained mismatch.  No case had to change its inputs to stay under a cap, with one exception:
the NaN voxels of march_volume() lie in free space, four steps off the band -- a hit refined against a NaN sample is a NaN gl_FragDepth,
which GL leaves undefined (the reference gives such a pixel margin 0; the oracle's depth clamp turns it into depth 0), and a NaN plane
through the slab made that the outcome of 174 pixels of one view.
"""
import functools

import numpy as np

import main_path_reference as R
from helpers import tsdf_close
import rgbd_recon_amd as rr
from oracle.oracle import OracleRecon

S = rr.scene

LIMIT = 0.04
F32_LIMIT = float(np.float32(LIMIT))

# Measured on the CPU (print_measurements()), oracle against reference, over the cases of all_cpu_cases():
#   dev       largest deviation on non-excluded elements          -> tol = 4 x dev, rounded up
#   need      largest margin of an element on which the oracle decides differently (sample count, hit flag, coverage, a +-limit flip)
#                                                                  -> bound = 4 x need, rounded up; where no element disagrees at all
#             (shade) the bound is 4 x the fp32 error of the compared |depth - z|, z about 0.5: 4 x 3 ulp(0.5) = 1e-6
#   excluded  largest share of excluded elements of any case at that bound (cap: what the share may never pass)
# quantity      dev        need       excluded
# tsdf          (fixed)    1.41e-6    1.50 %     helpers.tsdf_close is the tolerance; margins in TSDF units resp. texels of the depth image
# peel          3.45e-7    6.39e-7    2.14 %     window z; margin = distance to a projected face edge, pixels
# march_depth   2.40e-6    1.21e-6    0.37 %     gl_FragDepth; margin = |density| resp. distance of the ceil()'s argument to an integer
# colour        4.42e-4    none       0.00 %     modes 0 and 3 (3.1e-5 in mode 3)
# normal        4.66e-4    none       0.00 %     mode 2
TABLE = {
    "tsdf":        dict(tol=None, bound=6e-6, cap=0.05),
    "peel":        dict(tol=1.4e-6, bound=3e-6, cap=0.25),
    "march_depth": dict(tol=1e-5, bound=5e-6, cap=0.05),
    "normal":      dict(tol=1.9e-3, bound=1e-6, cap=0.05),
    "colour":      dict(tol=1.8e-3, bound=1e-6, cap=0.05),
}
EDGE_CAP_PX = 1.0          # depth limits: only pixels within 1 px of a projected edge may be excluded at all
MIN_BAND_VOXELS, MIN_HIT_PIXELS, MIN_PEEL_PIXELS = 500, 300, 300


class Mismatch(AssertionError):
    pass


MEASURE = None             # print_measurements() sets a dict: compare() then records instead of raising


def compare(what, ref, margin, bound, cap, sides, agree, count=None, minimum=0, excluded=None):
    """sides: {"kernel": array, "oracle": array}; agree(candidate, ref) -> bool array.  Raises Mismatch naming the side(s) that disagree with
    the reference, the worst element and its margin.  Returns the share of excluded elements and the number compared."""
    ex = (margin < bound) if excluded is None else excluded
    if MEASURE is not None:
        return _record(what, ref, margin, ex, sides, agree, count)
    base = np.ones(ex.shape, bool) if count is None else count
    share = float((ex & base).sum()) / max(int(base.sum()), 1)
    assert share <= cap, f"{what}: the reference's margin excludes {share:.2%} of the elements, more than the cap of {cap:.0%}: choose other inputs"
    compared = int((base & ~ex).sum())
    assert compared >= minimum, f"{what}: only {compared} elements compared, {minimum} wanted"
    wrong = {}
    for side, val in sides.items():
        ok = agree(val, ref)
        ok = ok.reshape(ok.shape[:ex.ndim] + (-1,)).all(-1) if ok.ndim > ex.ndim else ok
        bad = ~ok & ~ex
        if bad.any():
            at = np.argwhere(bad)
            worst = tuple(at[np.argmax(margin[bad])])
            wrong[side] = f"{int(bad.sum())} elements, e.g. {worst}: {side} {np.asarray(val)[worst]} reference {np.asarray(ref)[worst]} margin {margin[worst]:.3g}"
    if wrong:
        who = f"the {next(iter(wrong))} disagrees" if len(wrong) == 1 else " and ".join(wrong) + (" all" if len(wrong) == len(sides) else "") + " disagree"
        raise Mismatch(f"{what}: {who} with the float64 reference (bound {bound:g}). " + "; ".join(f"[{k}] {v}" for k, v in wrong.items()))
    return share, compared


def _record(what, ref, margin, ex, sides, agree, count):
    base = np.ones(ex.shape, bool) if count is None else count
    m = MEASURE.setdefault(what.split(":")[0], dict(dev=0.0, need=0.0, excluded=0.0, cases=0))
    m["cases"] += 1
    m["excluded"] = max(m["excluded"], float((ex & base).sum()) / max(int(base.sum()), 1))
    for val in sides.values():
        if getattr(agree, "tolerance", False):
            m["dev"] = max(m["dev"], deviation(val, ref, base & ~ex))
        else:
            ok = agree(val, ref)
            ok = ok.reshape(ok.shape[:ex.ndim] + (-1,)).all(-1) if ok.ndim > ex.ndim else ok
            if (~ok).any():
                m["need"] = max(m["need"], float(margin[~ok].max()))
    return m["excluded"], int((base & ~ex).sum())


def close_abs(tol):
    def f(a, b):
        with np.errstate(invalid="ignore"):
            return (np.abs(np.asarray(a, np.float64) - b) <= tol) | (np.isnan(a) & np.isnan(b))
    f.tolerance = True
    return f


def deviation(a, b, keep):
    """largest |a - b| over keep (NaN pairs count as equal)"""
    with np.errstate(invalid="ignore"):
        d = np.abs(np.asarray(a, np.float64) - b)
    d = np.where(np.isnan(a) & np.isnan(b), 0.0, d)
    d = d.reshape(d.shape[:keep.ndim] + (-1,)).max(-1) if d.ndim > keep.ndim else d
    return float(np.nan_to_num(d[keep], nan=np.inf).max()) if keep.any() else 0.0


# ---------------------------------------------------------------------------------------------------------------- integrate
INT_RES = (37, 44, 29)                      # no axis a multiple of the 8-voxel tile, all three different
INT_BRICK = [0.23, 0.26, 0.21]              # unrelated to the tiles
INT_KW = dict(res=INT_RES, brick_size=INT_BRICK, limit=LIMIT, view=(173, 99))
CLASS0_INV_RES = 40                         # under INT_RES a tile's LUT box is past the LDS budget: helpers.lut_box_class == 0 (asserted)


@functools.lru_cache(maxsize=None)
def integrate_scene(kind):
    """'base': 3 streams, 96x72, lut 16, inverse lut 24; 'class0': inverse lut 40; 'class2': inverse lut 16 (the LUT box class at
    which the separable integrate form exists); 'moved': base's calibration, the objects elsewhere"""
    kw = dict(n_streams=3, width=96, height=72, lut_res=16, inv_res={"class0": CLASS0_INV_RES, "class2": 16}.get(kind, 24))
    if kind == "moved":
        kw.update(sphere_c=(0.35, 0.9, -0.3), box_c=(-0.45, 0.5, 0.4))
    return S.make_scene(**kw)


@functools.lru_cache(maxsize=None)
def integrate_reference(kind):
    vol, margin = R.integrate(integrate_scene(kind), INT_RES, LIMIT)
    vol.setflags(write=False)
    margin.setflags(write=False)
    return vol, margin


def check_integrate(what, kind, sides, written=None):
    """sides: fp32 volumes; written: the voxels a culled integrate covers (None: all), the others hold the cleared -limit"""
    vol, margin = integrate_reference(kind)
    if written is not None:
        vol = np.where(written, vol, -F32_LIMIT)
        margin = np.where(written, margin, np.inf)
    t = TABLE["tsdf"]
    band = np.abs(vol) < F32_LIMIT
    share, _ = compare("tsdf: " + what, vol, margin, t["bound"], t["cap"], sides, lambda a, b: tsdf_close(np.asarray(a, np.float64), b, F32_LIMIT))
    n = int((band & (margin >= t["bound"])).sum())
    assert n >= MIN_BAND_VOXELS, f"{what}: only {n} band voxels compared"
    return share


# ---------------------------------------------------------------------------------------------------------------- views
VIEW = (173, 99)                            # neither a multiple of 8 nor of 16


def projection():
    return S.gl_flat(S.perspective(50.0, VIEW[0] / float(VIEW[1]), 0.1, 200.0))


def look(eye, at):
    return S.gl_flat(S.look_at(eye, at))


@functools.lru_cache(maxsize=None)
def small_scene():
    """the suite's small_scene fixture (tests/conftest.py)"""
    return S.make_scene(n_streams=4, width=160, height=120, lut_res=32, inv_res=32)


# ---------------------------------------------------------------------------------------------------------------- depth limits
def peel_eyes(brick_size, bbox_min):
    """name -> (eye, at): far outside; on the plane of the brick faces of x index 7 (those faces are seen edge-on: grazing); inside an occupied
    brick (on the sphere's surface); inside the volume looking along -z, with occupied bricks behind the eye and across the near plane"""
    gx = float(np.float32(bbox_min[0]) + np.float32(7.0) * np.float32(brick_size[0]))
    return {"far": ((2.6, 2.0, 2.2), (0.0, 1.0, 0.0)), "grazing": ((gx, 1.3, 2.8), (gx, 1.0, 0.0)),
            "in_brick": ((0.0, 1.1, 0.45), (0.9, 1.3, -0.7)), "axis": ((0.2, 1.0, 0.3), (0.2, 1.0, -1.0)),
            "near": ((1.3, 1.9, 1.6), (-0.1, 1.35, 0.0))}                     # for the few bricks of hand_counters()


def hand_counters(res_bricks):
    """counters set by hand (min_voxels 10, so every brick >= 10 is drawn): name -> array.  The neighbour test is `> 10`."""
    rx, ry, rz = res_bricks
    n = rx * ry * rz
    gid = lambda x, y, z: (z * ry + y) * rx + x
    out = {}
    c = np.zeros(n, np.uint32)
    c[gid(4, 4, 4)] = 50
    c[gid(5, 4, 4)] = 10                       # exactly 10: occupied, yet no neighbour in the test of bricks.gs -> the +x face of (4,4,4) is drawn
    c[gid(3, 4, 4)] = 11                       # exactly 11: a neighbour -> the -x face of (4,4,4) is not drawn
    out["ten_eleven"] = c
    c = np.zeros(n, np.uint32)
    for x in range(2, 7):
        c[gid(x, ry - 1, 5)] = 40              # the last row of bricks, which divideBox clips to the bounding box; the shader draws it whole
    c[gid(3, ry - 2, 5)] = 40
    out["last_row"] = c
    c = np.zeros(n, np.uint32)
    c[0] = 30                                  # index 0: the -1 neighbours' ids wrap past the buffer and read 0
    c[gid(0, 3, 4)] = 30                       # x index 0: its -x neighbour's id is that of (rx-1, 2, 4) ...
    c[gid(rx - 1, 2, 4)] = 30                  # ... which is occupied: the shader drops the -x face of (0, 3, 4)
    c[gid(0, 6, 6)] = 30                       # the same one row higher, while (rx-1, 6, 6) is a real neighbour of nobody's -x face
    c[gid(rx - 1, 5, 6)] = 30
    c[gid(rx - 1, 6, 6)] = 30
    out["wrap"] = c
    return out


def check_peels(what, ref, sides):
    """ref = R.depth_limits(...); sides: peel images [h][w][>=3].  Coverage (r < 1) must be equal and the three channels within tolerance at
    every pixel further than the bound from a projected face edge."""
    peels, covered, edge = ref
    t = TABLE["peel"]
    assert t["bound"] <= EDGE_CAP_PX
    anyc = covered.copy()
    for v in sides.values():
        anyc |= np.asarray(v)[..., 0] < 1
    share, n = compare("peel coverage: " + what, covered, edge, t["bound"], t["cap"], {k: np.asarray(v)[..., 0] < 1 for k, v in sides.items()},
                       lambda a, b: a == b, count=anyc)
    compare("peel: " + what, peels, edge, t["bound"], t["cap"], {k: np.asarray(v)[..., :3] for k, v in sides.items()}, close_abs(t["tol"]), count=anyc)
    kept = int((covered & (edge >= t["bound"])).sum())
    return share, kept


# ---------------------------------------------------------------------------------------------------------------- march
MARCH_RES = ((40, 56, 72), (37, 61, 50))
MARCH_BRICK = [2.0 / 8, 2.2 / 8, 2.0 / 8]
MARCH_EYES = {"far": ((0.0, 1.1, 3.0), (0.0, 1.1, 0.0)), "grazing": ((2.6, 2.0, 2.2), (0.0, 1.0, 0.0)),
              "inside": ((0.2, 1.0, 0.3), (0.0, 1.1, -1.0)), "axis": ((0.0, 5.0, 0.001), (0.0, 0.0, 0.0))}


@functools.lru_cache(maxsize=None)
def march_volume(kind, res):
    """fp32 [z][y][x]: 'sphere' = an off-centre sphere's clamped distance, 'slab' = a tilted slab; both with a box of exact -limit and a plane
    of NaN voxels"""
    p = R.voxel_positions(res)
    lim = np.float32(LIMIT)
    if kind == "sphere":
        d = 0.31 - np.linalg.norm((p - (0.47, 0.52, 0.44)) * (1.0, 1.1, 1.0), axis=-1)
    else:
        d = 0.5 * (0.17 - np.abs((p - (0.5, 0.45, 0.55)) @ np.array([0.36, 0.48, 0.8])))
    v = np.clip(d, -LIMIT, LIMIT).astype(np.float32)
    v = np.where(d <= -LIMIT, -lim, v)
    v[: res[2] // 5, :, : res[0] // 3] = -lim
    y = res[1] - 3                            # NaN where the plane y = res_y - 3 runs through free space, at least four steps off the band: a ray
    v[:, y, :][d[:, y, :] <= -3.0 * LIMIT] = np.nan       # walks through NaN samples and on, but never refines a hit against a NaN (undefined output)
    return np.ascontiguousarray(v)


def shell_counters(kind, res_bricks):
    """hand-set brick counters for skipSpace: 25 in every brick whose centre lies near the surface of march_volume(kind), 0 elsewhere"""
    rx, ry, rz = res_bricks
    c = R.voxel_positions(res_bricks)
    if kind == "sphere":
        near = np.abs(0.31 - np.linalg.norm((c - (0.47, 0.52, 0.44)) * (1.0, 1.1, 1.0), axis=-1)) < 0.16
    else:
        near = np.abs(0.17 - np.abs((c - (0.5, 0.45, 0.55)) @ np.array([0.36, 0.48, 0.8]))) < 0.14
    return np.where(near, 25, 0).astype(np.uint32).reshape(-1)


def observed_march(images):
    """(sample count, hit, depth) from view_images(): the count image holds n * 0.0027 (tsdf_raymarch.fs:395-398), a hit wrote a depth < 1"""
    _, depth, ns, _ = images
    return np.rint(np.asarray(ns, np.float64) / 0.0027), np.asarray(depth) < 1, np.asarray(depth, np.float64)


def check_march(what, ref, sides):
    """ref = R.march(...); sides: view_images() tuples.  Sample counts and hit flags equal, gl_FragDepth within tolerance, wherever the
    reference's margin is at least the bound."""
    t = TABLE["march_depth"]
    with np.errstate(invalid="ignore"):
        seen = ref["hit"] & (np.clip(ref["depth"], 0.0, 1.0) < 1.0)            # a fragment passes GL_LESS against the cleared 1
    obs = {k: observed_march(v) for k, v in sides.items()}
    touched = ref["n"] > 0
    for o in obs.values():
        touched = touched | (o[0] > 0)
    kw = dict(count=touched)
    share, _ = compare("march count: " + what, ref["n"], ref["margin"], t["bound"], t["cap"], {k: o[0] for k, o in obs.items()}, lambda a, b: a == b, **kw)
    compare("march hit: " + what, seen, ref["margin"], t["bound"], t["cap"], {k: o[1] for k, o in obs.items()}, lambda a, b: a == b, **kw)
    compare("march_depth: " + what, np.where(seen, np.clip(ref["depth"], 0.0, 1.0), 1.0), ref["margin"], t["bound"], t["cap"],
            {k: o[2] for k, o in obs.items()}, close_abs(t["tol"]), **kw)
    return share, int((seen & (ref["margin"] >= t["bound"])).sum())


# ---------------------------------------------------------------------------------------------------------------- shade
SHADE_RES = (64, 64, 64)
SHADE_KW = dict(res=SHADE_RES, brick_size=MARCH_BRICK, limit=LIMIT, view=VIEW)
SHADE_EYE = ((1.9, 1.9, 2.3), (0.1, 0.9, 0.0))


def check_shade(what, mode, march_ref, shade_ref, sides):
    """sides: view_images() tuples of a draw in `mode`; compared at the reference's hit pixels"""
    key = "normal" if mode == 2 else "colour"
    t, tm = TABLE[key], TABLE["march_depth"]
    with np.errstate(invalid="ignore"):
        seen = march_ref["hit"] & (np.clip(march_ref["depth"], 0.0, 1.0) < 1.0)
    margin = np.full(seen.shape, np.inf)
    margin[march_ref["hit"]] = shade_ref["margin"]
    ex = (margin < t["bound"]) | (march_ref["margin"] < tm["bound"])
    ref = np.zeros(seen.shape + (4,))
    ref[march_ref["hit"]] = shade_ref["rgba"]
    ref[~seen] = 0.0
    share, n = compare(f"{key}: {what} mode {mode}", ref, margin, t["bound"], t["cap"], {k: np.where(seen[..., None], np.asarray(v[0], np.float64), 0.0) for k, v in sides.items()},
                       close_abs(t["tol"]), count=seen, minimum=MIN_HIT_PIXELS, excluded=ex)
    return share, n


# ---------------------------------------------------------------------------------------------------------------- drivers
# Each takes the objects to drive -- OracleRecon and / or ReconIntegrationHip, which share their method names -- and returns what the
# check_* functions take.  `orc` is always among them: it supplies the brick layout and counters the reference reads as inputs.
def refresh_bricks(o):
    o.clearOccupiedBricks()
    o.markBricks()
    o.updateOccupiedBricks()


def drive_integrate(objs, use_bricks, then=None):
    """integrate() of the uploaded frame; `then`: upload that scene as a second frame and integrate again"""
    for o in objs:
        o.setUseBricks(use_bricks)
        refresh_bricks(o)
        o.integrate()
        if then is not None:
            o.upload_frame(then)
            refresh_bricks(o)
            o.integrate()


def written_voxels(orc):
    return brick_voxel_mask_of(orc, orc.counters() >= 10)


def brick_voxel_mask_of(orc, occupied):
    return R.brick_voxel_mask(orc.res, orc.brick_ranges().astype(np.int64), occupied)


def peel_reference(orc, counters, mv, pr):
    occ = np.flatnonzero(np.asarray(counters) >= 10)                        # updateOccupiedBricks, m_min_voxels_per_brick 10
    return R.depth_limits(counters, occ, orc.res_bricks, orc.brick_size, orc.scene["bbox_min"], mv, pr, VIEW)


def drive_peels(objs, mv, pr, counters=None):
    """skipSpace draw -> the peel images"""
    out = []
    for o in objs:
        o.setUseBricks(True)
        o.setSpaceSkip(True)
        o.setColorFilling(False)
        if counters is None:
            refresh_bricks(o)
        else:
            o.set_counters(counters)
            o.updateOccupiedBricks()
        o.draw(mv, pr)
        out.append(o.view_images()[3])
    return out


def drive_march(objs, volume, mv, pr, counters=None):
    """march of an uploaded volume, dense (counters None) or with skipSpace from hand-set counters -> view_images() per object"""
    out = []
    for o in objs:
        o.setColorFilling(False)
        o.setUseBricks(counters is not None)
        o.setSpaceSkip(counters is not None)
        if counters is not None:
            o.set_counters(counters)
            o.updateOccupiedBricks()
        o.set_tsdf(volume)
        o.draw(mv, pr)
        out.append(o.view_images())
    return out


@functools.lru_cache(maxsize=None)
def march_reference_dense(kind, res, eye):
    sc = small_scene()
    return R.march(march_volume(kind, res), None, look(*MARCH_EYES[eye]), projection(), VIEW, LIMIT, sc["bbox_min"], sc["bbox_max"])


def march_reference_skip(kind, res, eye, peels):
    sc = small_scene()
    return R.march(march_volume(kind, res), peels, look(*MARCH_EYES[eye]), projection(), VIEW, LIMIT, sc["bbox_min"], sc["bbox_max"])


def shade_references(volume, mode):
    """(march, shade) references of the shade view on an fp32 volume"""
    sc = small_scene()
    m = R.march(volume, None, look(*SHADE_EYE), projection(), VIEW, LIMIT, sc["bbox_min"], sc["bbox_max"])
    return m, R.shade(sc, volume, m["pos"][m["hit"]], m["view"], LIMIT, mode)


def drive_shade(objs, volume, mode):
    out = []
    for o in objs:
        o.setColorFilling(False)
        o.setUseBricks(False)
        o.setSpaceSkip(False)
        o.setShadeMode(mode)
        o.set_tsdf(volume)
        o.draw(look(*SHADE_EYE), projection())
        out.append(o.view_images())
    return out


# ---------------------------------------------------------------------------------------------------------------- the cases
# make(scene, **kw) -> {"oracle": OracleRecon, ["kernel ...": ReconIntegrationHip, ...]}: the CPU tests pin the oracle alone, the GPU tests
# hold kernels and oracle to the same references on the same inputs.
def only_oracle(scene, **kw):
    return {"oracle": OracleRecon(scene, **kw)}


def integrate_case(make, kind, use_bricks, moved=False):
    objs = make(integrate_scene(kind), **INT_KW)
    drive_integrate(objs.values(), use_bricks, integrate_scene("moved") if moved else None)
    written = written_voxels(objs["oracle"]) if use_bricks else None
    what = f"integrate {kind}{' then moved' if moved else ''} {'culled' if use_bricks else 'dense'}"
    return check_integrate(what, "moved" if moved else kind, {k: o.tsdf() for k, o in objs.items()}, written), objs


def brick_clip(orc, ids, mv, pr):
    """clip coordinates [n][8][4] of the corners of the bricks `ids`"""
    rx, ry = orc.res_bricks[0], orc.res_bricks[1]
    ids = np.asarray(ids, np.int64)
    idx = np.stack([ids % (rx * ry) % rx, ids % (rx * ry) // rx, ids // (rx * ry)], -1).astype(np.float64)
    bs, lo = np.asarray(orc.brick_size, np.float64), np.asarray(orc.scene["bbox_min"], np.float64)
    world = (idx * bs + lo)[:, None, :] + R.CUBE[None] * bs
    return R._xf(R.mat(pr) @ R.mat(mv), world)


def peel_case(make, eye=None, counters=None):
    """one of peel_eyes() with the bricks the scene marks, or one of hand_counters() seen from nearby"""
    objs = make(small_scene(), **INT_KW)
    orc = objs["oracle"]
    eyes = peel_eyes(orc.brick_size, orc.scene["bbox_min"])
    mv, pr = look(*eyes[eye or "near"]), projection()
    cnt = None if counters is None else hand_counters(orc.res_bricks)[counters]
    images = drive_peels(objs.values(), mv, pr, cnt)
    cnt = orc.counters() if cnt is None else cnt
    occ = np.flatnonzero(cnt >= 10)
    ref = peel_reference(orc, cnt, mv, pr)
    clip = brick_clip(orc, occ, mv, pr)
    if eye == "in_brick":                                    # the situation really occurs: the eye's own brick is occupied
        e = np.asarray(eyes[eye][0])
        i = np.floor((e - np.asarray(orc.scene["bbox_min"], np.float64)) / np.asarray(orc.brick_size, np.float64)).astype(int)
        assert cnt[(i[2] * orc.res_bricks[1] + i[1]) * orc.res_bricks[0] + i[0]] >= 10, "the eye's brick is not occupied"
    if eye == "axis":                                        # bricks wholly behind the eye, and bricks across the near plane
        behind = (clip[..., 3] <= 0).all(-1)
        inside = clip[..., 2] + clip[..., 3] >= 0
        assert behind.any() and (inside.any(-1) & ~inside.all(-1)).any(), "no brick behind the eye / across the near plane"
    what = f"depth limits {eye or counters}"
    share, kept = check_peels(what, ref, dict(zip(objs, images)))
    assert kept >= MIN_PEEL_PIXELS or MEASURE is not None, f"{what}: only {kept} peel pixels compared"
    return share, kept, ref, objs


def march_case(make, kind, res, skip, eyes=tuple(MARCH_EYES)):
    objs = make(small_scene(), res=res, brick_size=MARCH_BRICK, limit=LIMIT, view=VIEW)
    orc = objs["oracle"]
    cnt = shell_counters(kind, orc.res_bricks) if skip else None
    vol = march_volume(kind, res)
    shares, hits = [], 0
    for eye in eyes:
        mv, pr = look(*MARCH_EYES[eye]), projection()
        images = dict(zip(objs, drive_march(objs.values(), vol, mv, pr, cnt)))
        ref = march_reference_skip(kind, res, eye, images["oracle"][3]) if skip else march_reference_dense(kind, res, eye)
        share, n = check_march(f"march {kind} {res} {'skipSpace' if skip else 'dense'} eye {eye}", ref, images)
        shares.append(share)
        hits += n
    assert hits >= MIN_HIT_PIXELS or MEASURE is not None, f"march {kind} {res}: only {hits} hit pixels compared"
    return max(shares), hits


@functools.lru_cache(maxsize=None)
def shade_volume():
    """the oracle's dense integrate of small_scene: an fp32 input of the shade cases"""
    o = OracleRecon(small_scene(), **SHADE_KW)
    o.setUseBricks(False)
    o.integrate()
    v = o.tsdf()
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def shade_reference(mode):
    return shade_references(shade_volume(), mode)


def shade_case(make, mode):
    objs = make(small_scene(), **SHADE_KW)
    images = dict(zip(objs, drive_shade(objs.values(), shade_volume(), mode)))
    m, sh = shade_reference(mode)
    return check_shade("shade", mode, m, sh, images)


def all_cpu_cases():
    for kind in ("base", "class0"):
        for ub in (False, True):
            yield integrate_case, (kind, ub)
    for ub in (False, True):
        yield integrate_case, ("class2", ub)
    yield integrate_case, ("base", True, True)
    for eye in ("far", "grazing", "in_brick", "axis"):
        yield peel_case, (eye, None)
    for c in ("ten_eleven", "last_row", "wrap"):
        yield peel_case, (None, c)
    for res in MARCH_RES:
        for kind in ("sphere", "slab"):
            for skip in (False, True):
                yield march_case, (kind, res, skip)
    for mode in (0, 2, 3):
        yield shade_case, (mode,)


def print_measurements():
    """python -c 'import main_path_cases as C; C.print_measurements()' from tests/: what TABLE was filled from"""
    global MEASURE
    MEASURE = {}
    try:
        for f, a in all_cpu_cases():
            f(only_oracle, *a)
    finally:
        m, MEASURE = MEASURE, None
    for k, v in m.items():
        print(f"{k:14s} cases {v['cases']:3d}  dev {v['dev']:.3g}  margin of the worst exact mismatch {v['need']:.3g}  excluded {v['excluded']:.2%}")
    return m
