"""The pre-processing passes against the float64 reference of tests/preprocess_reference.py: the cases, the drivers and the measured
tolerances, shared by tests/test_preprocess_reference.py (the oracle, no GPU) and tests/test_gpu_preprocess_reference.py (kernels and oracle).
HIP-free.  The inputs are those of tests/preprocess_cases.py, unchanged, plus saturated(); the acceptance rule is compare() of
tests/main_path_cases.py.

The chain is cut between the passes: pass k of the reference is fed the candidate's OWN product of pass k - 1 (the oracle's on the CPU, the
kernels' and the oracle's on the GPU), so a decision that goes the other way in one pass does not change what the next pass is asked, and
every pass is judged alone.  The boundary pass is judged with the reference's own Lab image (computed from the colours, cv_uv and the
candidate's filter input): inside the pipeline the kernels never materialise one.  The Lab image a context hands out is compared separately.

PASSES, measured on the CPU (print_measurements() repeats it), oracle against reference, over all_cases() -- tiny, odd, edge_depths,
compressed, saturated and sensor under the flag sets of the GPU shape tests, each as built and under mirrored():
  dev       largest deviation on pixels whose margin is at least the bound (quality: relative to max(|q|, 1)) -> tol = 4 x dev, rounded up
  need      largest margin of a pixel that deviates by more than tol, i.e. on which the oracle decided differently -> bound >= 4 x need.
            The oracle decides differently NOWHERE (the one `need` that is not 0 belongs to normalize(0) pixels, see normals), so each bound
            is 4 x the fp32 error of what the margin measures, rounded up
  excluded  largest share of excluded pixels of any case, of ALL the pass's pixels (what the 5 % cap is held against) / of those with a depth
  fewest    fewest pixels with a depth compared in any case (tiny; wanted: 200, and 3 000 for the others)
quantity     dev       need      bound   excluded          fewest
depth2       3.58e-7   none      1e-5    0.00 % / 0.00 %   359   margin |avg - tap| - 0.2 in metres: avg is a sum of <= 8 depths <= 4.5, error ~ 2e-6
depth_rg     1.28e-6   none      1e-5    0.10 % / 0.30 %   260   world position to a box face, metres: 7 lerps of values <= 2.5, error ~ 2.5e-6; | |tap - c| - limit |
lab          1.50e-5   none      1e-6    3.61 % / 3.61 %   360   normalised depth to 0 / 1: error ~ 1.5e-7 (edge_depths plants depths one ulp inside the limits: 3.6 %)
depth_b      0         none      1e-4    0.00 % / 0.01 %   260   mean colour distance to 0.5: <= 25 distances of Lab values that carry 1.5e-5 each (lab's dev)
silhouette   0         none      1e-4    0.00 % / 0.01 %   260   (the same decision; depth_b and silhouette are copies and constants: tolerance 0)
normals      7.57e-4   3.97e-8   1e-6    1.60 % / 7.80 %   224   |cross product|, m^2: two differences of world positions, 2 * 0.05 * 2.5e-6.  The excluded pixels are flat
                                                                 patches in the outermost rows / columns, where both taps fall into the LUT's clamped rim: normalize(0)
quality      1.06e-5   none      1e-6    2.92 % / 13.4 %   224   | |tap - c| - 0.35 c | in normalised depth: error ~ 1e-7.  Excluded: the NaN normals above and their neighbours
bricks       0         1e-7      1e-5    0.27 %            224   world position to a brick face / the 0.1 test, metres, as depth_rg; `need` on a decade grid; share of the marking pixels

The colour comparison of the boundary pass decides nothing on the inputs of preprocess_cases: inc_color.glsl:14-16 divides by 255 what
texture() already returned in [0, 1], so n <= 1 / 255 < 0.04045 for every 8-bit colour, pivot_RGB never takes its pow() branch, X / Xn,
Y / Yn and Z / Zn stay below 0.0004 < epsilon, pivot_XYZ never takes its cube root, and L <= 0.28.  Those two branches are dead in the
pipeline and are checked directly against closed form (tests/test_preprocess_reference.py::test_rgb_to_lab_every_branch).  The distance
threshold itself is NOT out of reach, though: a and b carry factors of 3 900 and 1 560, pure green and pure magenta are 0.99 apart
(test_8_bit_colours_never_leave_the_linear_branches_yet_reach_the_distance_threshold), while make_scene's palette stays below 0.29 -- the
largest mean distance of any candidate of the cases above is 0.27.  saturated(odd) is the one input added: green / magenta texels at random,
on which 2 888 of 3 315 candidates are rejected by their colour and 427 kept, the closest 9e-5 from the threshold.

The range cells k_pre_quality writes have no download; they stay with tests/test_gpu_preprocess_shapes.py::test_raw_path_volume_is_exact.
"""
import functools
import hashlib

import numpy as np

import main_path_cases as M
import preprocess_cases as pc
import preprocess_reference as P
from oracle.oracle import OracleRecon

CAP = 0.05
MINIMUM = dict(tiny=200, odd=3000, edge_depths=3000, compressed=3000, saturated=3000, sensor=3000)

PASSES = {
    "depth2":     dict(tol=1.5e-6, bound=1e-5),
    "depth_rg":   dict(tol=5.2e-6, bound=1e-5),
    "lab":        dict(tol=6e-5, bound=1e-6),
    "depth_b":    dict(tol=0.0, bound=1e-4),
    "silhouette": dict(tol=0.0, bound=1e-4),
    "normals":    dict(tol=3.1e-3, bound=1e-6),
    "quality":    dict(tol=4.3e-5, bound=1e-6),
    "bricks":     dict(tol=0, bound=1e-5),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    """built once; nobody writes to them"""
    if name.endswith("/mirrored"):
        return mirrored(scene(name[:-len("/mirrored")]))
    if name in ("tiny", "odd", "sensor"):
        return getattr(pc, name)()
    return dict(edge_depths=pc.edge_depths, compressed=pc.compressed, saturated=saturated)[name](scene("odd"))


# pc.KW's bricks (2 / 8, 2.2 / 8, 2 / 8) put the planes plant_edges plants for stream 0 (1.65 m: x = 0.85) exactly on the 0.1 * brick_size
# test of inc_bricks.glsl:52 (|0.85 - 0.875| = 0.025), tiny's plane for stream 0 (2.5 m: x = 0) and the cameras' own height 1.1 on brick faces
# (4 * 0.25 - 1, 4 * 0.275): a third of the marking pixels would be in doubt, against a cap of 5 %.  The brick size belongs to the context, not
# to the input.  setBrickSize snaps it to whole voxels (recon_integration.cpp:463); these snap to 3 voxels per axis under tiny's 32^3 and to
# (7, 7, 6) voxels under the 64^3 of the others, which puts none of x = 0, 0.2, 0.85 and y = 1.1 on a face or on the 0.1 test.
BRICKS = dict(tiny=[0.19, 0.2, 0.19], odd=[0.22, 0.24, 0.2], sensor=[0.22, 0.24, 0.2])


def kw_of(name):
    name = name if name in pc.KW else "odd"
    return dict(pc.KW[name], brick_size=BRICKS[name])


def mirrored(sc):
    """The same frame under a calibration whose image rows run top-down, as a sensor's do: cv_xyz's world y mirrored about the cameras' height
    (the bounding box 0 .. 2.2 and the cameras at 1.1 map onto themselves; every image, and so every planted pixel, stays where it is).
    make_scene's rows run bottom-up, and pre_normal.fs:55 then yields normals that point AWAY from the camera: the angle of pre_quality.fs:46
    is negative at every pixel of every case of preprocess_cases, pow(angle, 2.0) of :114 undefined, and the quality pass would be excluded
    whole.  Under this calibration the angle is positive and the quality pass is judged."""
    out = dict(sc)
    xyz = np.array(sc["cv_xyz"], np.float64)
    xyz[..., 1] = float(sc["bbox_min"][1]) + float(sc["bbox_max"][1]) - xyz[..., 1]
    out["cv_xyz"] = np.ascontiguousarray(xyz, np.float32)
    r = [int(x) for x in sc["inv_res"]]
    inv = np.asarray(sc["cv_xyz_inv"]).reshape(sc["n"], r[2], r[1], r[0], 4)[:, :, ::-1]
    out["cv_xyz_inv"] = np.ascontiguousarray(inv.reshape(sc["n"], -1, 4))
    return out


def saturated(sc, seed=7):
    """the same frame with every colour texel pure green or pure magenta, at random: the two corners of the colour cube that are furthest
    apart under inc_color.glsl as written (0.99).  The mean distance of a boundary candidate's Lab colour to its 25 taps then falls on both
    sides of the 0.5 of pre_boundary.fs:105 -- the only input of this suite on which the colour comparison decides anything."""
    out = dict(sc)
    pick = np.random.default_rng(seed).random(sc["color"].shape[:3]) < 0.5
    out["color"] = np.where(pick[..., None], np.array([0, 255, 0], np.uint8), np.array([255, 0, 255], np.uint8)).astype(np.uint8)
    return out


def flags_of(flags):
    f = dict(filter_textures=True, processed_depth=True, refine=True)
    f.update(dict(flags))
    return f


def flag_id(flags):
    f = flags_of(flags)
    return "".join(c if f[k] else "-" for c, k in zip("FPR", ("filter_textures", "processed_depth", "refine")))


# ---------------------------------------------------------------------------------------------------------------- the reference, cached by input
_CACHE = {}


def _cached(fn, *arrays, extra=()):
    """fn(*arrays, *extra) once per distinct input: kernels and oracle usually hand the same bytes to the next pass"""
    h = hashlib.sha1(fn.__name__.encode())
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype, a.shape)).encode())
        h.update(a.tobytes())
    h.update(repr(extra).encode())
    k = h.hexdigest()
    if k not in _CACHE:
        _CACHE[k] = fn(*arrays, *extra)
    return _CACHE[k]


def _filter(depth_in, colour, i, name, filter_textures, compression):
    sc = scene(name)
    return P.filter_pass(depth_in, colour, P.lut(sc["cv_xyz"][i], sc["lut_res"], 3), P.lut(sc["cv_uv"][i], sc["lut_res"], 2), sc["bbox_min"], sc["bbox_max"],
                         sc["depth_limits"], filter_textures, compression)


def _normal(depth_b, i, name, brick_size, res_bricks):
    sc = scene(name)
    return P.normal_pass(depth_b, P.lut(sc["cv_xyz"][i], sc["lut_res"], 3), sc["bbox_min"], brick_size, res_bricks)


def _quality(depth_b, normals, i, name):
    sc = scene(name)
    return P.quality_pass(depth_b, normals, P.lut(sc["cv_xyz"][i], sc["lut_res"], 3), sc["camera_positions"][i])


def reference(name, flags, pp, raw, colour, brick_size, res_bricks):
    """every pass of the reference on one candidate's own products `pp` -> {quantity: (ref [n]..., margin [n][h][w])}, marks"""
    sc, f = scene(name), flags_of(flags)
    out = {k: [] for k in ("depth2", "depth_rg", "lab", "depth_b", "silhouette", "normals", "quality")}
    marks = []
    npx = sc["height"] * sc["width"]
    for i in range(sc["n"]):
        comp = sc.get("depth_compression")
        comp = tuple(comp[i][1:]) if comp is not None and comp[i][0] else None
        out["depth2"].append(_cached(P.morph, raw[i]))
        rg, lab, m = _cached(_filter, pp["depth2"][i] if f["processed_depth"] else raw[i], colour[i], extra=(i, name, f["filter_textures"], comp))
        out["depth_rg"].append((rg, m["depth_rg"]))
        out["lab"].append((lab, m["lab"]))
        db, sil, mb, _ = _cached(P.boundary, pp["depth_rg"][i], lab, extra=(f["refine"],))
        out["depth_b"].append((db, mb))
        out["silhouette"].append((sil, mb))
        n, mn, mk = _cached(_normal, pp["depth_b"][i], extra=(i, name, tuple(float(b) for b in brick_size), tuple(int(r) for r in res_bricks)))
        out["normals"].append((n, mn))
        marks.append(dict(mk, pixel=mk["pixel"] + i * npx))
        out["quality"].append(_cached(_quality, pp["depth_b"][i], pp["normals"][i], extra=(i, name)))
    ref = {k: (np.stack([a for a, _ in v]), np.stack([b for _, b in v])) for k, v in out.items()}
    return ref, {k: np.concatenate([m[k] for m in marks]) for k in marks[0]}


# ---------------------------------------------------------------------------------------------------------------- one candidate against it
def has_depth(a):
    with np.errstate(invalid="ignore"):
        return np.asarray(a) > 0


def judge(what, name, side, pp, counters, ref, marks, res_bricks):
    """compare() of every pass for one candidate; the quality pass under a mirrored calibration only (mirrored()).
    -> {quantity: (excluded share, compared)}"""
    res = {}
    minimum = MINIMUM[name.split("/")[0]]

    def one(q, val, count, scale=None, minimum=minimum):
        t = PASSES[q]
        r, m = ref[q]
        s = 1.0 if scale is None else scale
        share, _ = M.compare(f"{q}: {what}", r / s, m, t["bound"], CAP, {side: np.asarray(val, np.float64) / s}, M.close_abs(t["tol"]))
        kept = int((count & ~(m < t["bound"])).sum())                          # the cap counts all compared pixels, the minimum those with a depth
        assert kept >= minimum or M.MEASURE is not None, f"{q}: {what}: only {kept} pixels with a depth compared, {minimum} wanted"
        res[q] = (share, kept, float((count & (m < t["bound"])).sum()) / max(int(count.sum()), 1))

    one("depth2", pp["depth2"], has_depth(ref["depth2"][0]) | has_depth(pp["depth2"]))
    rgd = has_depth(ref["depth_rg"][0][..., 0]) | has_depth(pp["depth_rg"][..., 0])
    one("depth_rg", pp["depth_rg"], rgd)
    if "lab" in pp:
        one("lab", pp["lab"], np.ones(rgd.shape, bool))
    one("depth_b", pp["depth_b"], has_depth(pp["depth_rg"][..., 0]))
    one("silhouette", pp["silhouette"], has_depth(pp["depth_rg"][..., 0]))
    with np.errstate(invalid="ignore"):
        inside = (pp["depth_b"][..., 0] > 0) & (pp["depth_b"][..., 0] < 1)
    one("normals", pp["normals"], inside)
    if name.endswith("/mirrored"):
        one("quality", pp["quality"], inside, scale=np.maximum(np.abs(ref["quality"][0]), 1.0))
    # the brick counters: per brick, off by at most the number of its marking pixels whose margin is below the bound
    t = PASSES["bricks"]
    nb = int(np.prod(res_bricks))
    unsure = marks["margin"] < t["bound"]
    want, slack = P.brick_counts(marks, nb), P.brick_slack(marks, unsure, res_bricks)
    share = float(unsure.sum()) / max(unsure.size, 1)
    if M.MEASURE is None:
        assert share <= CAP, f"bricks: {what}: {share:.2%} of the marking pixels lie within {t['bound']:g} of a decision of mark_brick, more than the cap"
        assert unsure.size - int(unsure.sum()) >= minimum, f"bricks: {what}: only {unsure.size - int(unsure.sum())} marking pixels"
        bad = np.abs(np.asarray(counters, np.int64) - want) > slack
        if bad.any():
            b = int(np.flatnonzero(bad)[0])
            raise M.Mismatch(f"bricks: {what}: the {side} disagrees with the float64 reference (bound {t['bound']:g}) in {int(bad.sum())} bricks, e.g. brick {b}: "
                             f"{side} {int(counters[b])} reference {int(want[b])} with {int(slack[b])} pixels in doubt")
    else:
        m = M.MEASURE.setdefault("bricks", dict(dev=0.0, need=0.0, excluded=0.0, cases=0))
        m["cases"] += 1
        m["excluded"] = max(m["excluded"], share)
        for b in [0.0] + [10.0 ** e for e in range(-12, -1)]:                 # the smallest bound of a decade grid at which the counters agree
            if (np.abs(np.asarray(counters, np.int64) - want) <= P.brick_slack(marks, marks["margin"] < b, res_bricks)).all():
                break
        m["need"] = max(m["need"], b)
    res["bricks"] = (share, unsure.size - int(unsure.sum()))
    return res


def products(obj, sc):
    """(products, counters, raw depth, colour) of a processed context: the oracle's, or the kernels' through their downloads"""
    if isinstance(obj, OracleRecon):
        return obj.preprocessed(), obj.counters(), np.asarray(sc["depth_raw"], np.float32), np.asarray(sc["color"], np.uint8)
    raw, rgba = obj.raw_frame()
    return obj.preprocessed(lab=True), obj.bricks()[0], raw, rgba[..., :3]


def variants(name):
    """a case runs twice: on the input as preprocess_cases builds it, and on the same frame under mirrored()'s calibration"""
    return name, name + "/mirrored"


def run_case(make, name, flags=()):
    """make(scene, **kw) -> {"oracle": ..., ["kernel": ...]} as in main_path_cases.  Every side is judged against the reference of its own
    products; a failure names the kernel, the oracle or both."""
    wrong, res = {}, {}
    for var in variants(name):
        sc = scene(var)
        objs = make(sc, **kw_of(name))
        what = f"{var} {flag_id(flags)}"
        for side, o in objs.items():
            pc.process(o, sc, dict(flags))
            pp, counters, raw, colour = products(o, sc)
            ref, marks = reference(var, flags, pp, raw, colour, o.brick_size, o.res_bricks)
            try:
                res[var, side] = judge(what, var, side, pp, counters, ref, marks, o.res_bricks)
            except M.Mismatch as e:
                wrong.setdefault(side, []).append(str(e))
            if hasattr(o, "close"):
                o.close()
    if wrong:
        who = "kernel and oracle both disagree" if len(wrong) > 1 else f"only the {next(iter(wrong))} disagrees"
        raise M.Mismatch(f"{name} {flag_id(flags)}: {who} with the float64 reference.  " + "  ".join(sum(wrong.values(), [])))
    return res


def only_oracle(sc, **kw):
    return {"oracle": OracleRecon(sc, **kw)}


GPU_CASES = ([("tiny", tuple(f.items())) for f in pc.TWO_FLAGS] + [("odd", tuple(f.items())) for f in pc.ALL_FLAGS] +
             [("edge_depths", ()), ("compressed", ()), ("compressed", (("processed_depth", False),)), ("saturated", ())])
CPU_ONLY_CASES = [("sensor", tuple(f.items())) for f in pc.TWO_FLAGS]


def all_cases():
    return GPU_CASES + CPU_ONLY_CASES


def case_id(c):
    return f"{c[0]}-{flag_id(c[1])}"


def print_measurements(cases=None):
    """python -c 'import preprocess_reference_cases as C; C.print_measurements()' from tests/: what PASSES was filled from.  Two rounds: the
    deviations at the bounds of PASSES, then the largest margin among the elements that deviate by more than the tolerance."""
    out = {}
    for c in [(v, c[1]) for c in (cases or all_cases()) for v in variants(c[0])]:
        sc = scene(c[0])
        o = OracleRecon(sc, **kw_of(c[0].split("/")[0]))
        pc.process(o, sc, dict(c[1]))
        pp, counters, raw, colour = products(o, sc)
        ref, marks = reference(c[0], c[1], pp, raw, colour, o.brick_size, o.res_bricks)
        M.MEASURE = {}
        try:
            res = judge(case_id(c), c[0], "oracle", pp, counters, ref, marks, o.res_bricks)
        finally:
            meas, M.MEASURE = M.MEASURE, None
        for q, m in meas.items():
            t = PASSES[q]
            d = out.setdefault(q, dict(dev=0.0, need=0.0, excluded=0.0, dev0=0.0, of_depth=0.0, kept=1 << 30))
            d["dev"], d["excluded"] = max(d["dev"], m["dev"]), max(d["excluded"], m["excluded"])
            d["kept"] = min(d["kept"], res[q][1])
            d["of_depth"] = max(d["of_depth"], res[q][-1] if q != "bricks" else res[q][0])
            if q == "bricks":
                d["need"] = max(d["need"], m["need"])
                continue
            r, mg = ref[q]
            s = np.maximum(np.abs(r), 1.0) if q == "quality" else 1.0
            with np.errstate(invalid="ignore"):
                dv = np.abs(np.asarray(pp[q], np.float64) / s - r / s)
            dv = np.where(np.isnan(pp[q]) & np.isnan(r), 0.0, np.nan_to_num(dv, nan=np.inf))
            dv = dv.reshape(dv.shape[:3] + (-1,)).max(-1)
            d["dev0"] = max(d["dev0"], float(dv.max()))
            if (dv > t["tol"]).any():
                d["need"] = max(d["need"], float(mg[dv > t["tol"]].max()))
    for q, d in out.items():
        print(f"{q:12s} dev {d['dev']:.3g}  (over all elements: {d['dev0']:.3g})  need {d['need']:.3g}  excluded {d['excluded']:.2%} of all pixels, "
              f"{d['of_depth']:.2%} of those with a depth; fewest compared with a depth {d['kept']}")
    return out
