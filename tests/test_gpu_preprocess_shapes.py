"""-m gpu: the pre-processing passes (tsdf_process_textures) at image shapes other than the suite's 160 x 120 -- the cases of
tests/preprocess_cases.py: smaller than one block and than the 13 x 13 window, partial in x and y for every tiling the passes use, the
reference's own 512 x 424, a colour size unequal to the depth size -- under every flag combination, with non-finite and limit raw depths
behind the morph pass, with per-stream depth compression, with the candidate list overflowing, and through the lanes.

Tolerances are those of tests/test_gpu_preprocess.py: everything without pow() bit for bit, Lab 1e-6 absolute, quality 1e-5 relative.
test_raw_path_volume_is_exact removes pow() from the comparison altogether: the raw path's volume against three integrations of its own
quality values."""
import functools

import numpy as np
import pytest

import preprocess_cases as pc
from helpers import assert_same
from oracle.oracle import OracleRecon

pytestmark = pytest.mark.gpu

EXACT = ("depth2", "depth_rg", "depth_b", "silhouette", "normals")


@functools.lru_cache(maxsize=None)
def scene(name):
    """built once per session; nobody writes to them (edge_depths / compressed / processed_scene copy)"""
    if name in ("tiny", "odd", "sensor"):
        return getattr(pc, name)()
    return dict(edge_depths=pc.edge_depths, compressed=pc.compressed)[name](scene("odd"))


def kw_of(name):
    return pc.KW[name if name in pc.KW else "odd"]


@functools.lru_cache(maxsize=None)
def oracle_products(name, flags=()):
    """(products, brick counters) of the oracle's passes on a case, computed once for the tests that share it"""
    o = OracleRecon(scene(name), **kw_of(name))
    pc.process(o, scene(name), dict(flags))
    return o.preprocessed(), o.counters()


def check_products(hip, name, flags=(), lab=True):
    sc = scene(name)
    b, counters = oracle_products(name, tuple(sorted(dict(flags).items())))
    a = hip.preprocessed(lab=lab)
    what = f"{name} {dict(flags)}"
    for k in EXACT:
        assert_same(a[k], b[k], f"{what}: {k}")
    if lab:
        assert np.abs(a["lab"] - b["lab"]).max() <= 1e-6, what
    with np.errstate(invalid="ignore"):
        ok = (np.abs(a["quality"] - b["quality"]) <= 1e-5 * np.maximum(np.abs(b["quality"]), 1e-3)) | (np.isnan(a["quality"]) & np.isnan(b["quality"]))
    assert ok.all(), f"{what}: quality, {(~ok).sum()} of {ok.size} pixels"
    np.testing.assert_array_equal(hip.bricks()[0], counters, err_msg=what)
    raw, rgba = hip.raw_frame()
    assert_same(raw, sc["depth_raw"], f"{what}: raw depth")
    np.testing.assert_array_equal(rgba[..., :3], sc["color"], err_msg=f"{what}: re-laid-out colour")      # (odd: the last, partial quad of the colour layer)
    assert (rgba[..., 3] == 255).all(), what
    assert (b["silhouette"] > 0).sum() > 0 and counters.sum() > 0


def run_hip(rr, name, flags=()):
    hip = rr.ReconIntegrationHip(scene(name), **kw_of(name))
    pc.process(hip, scene(name), dict(flags))
    return hip


# odd: all eight (filter_textures, processed_depth, refine) combinations; the other two: the default and the raw, unrefined one
FLAG_CASES = [("odd", tuple(f.items())) for f in pc.ALL_FLAGS] + [(n, tuple(f.items())) for n in ("tiny", "sensor") for f in pc.TWO_FLAGS]


def flag_id(flags):
    f = dict(filter_textures=True, processed_depth=True, refine=True)
    f.update(dict(flags))
    return "".join(c if f[k] else "-" for c, k in zip("FPR", ("filter_textures", "processed_depth", "refine")))


@pytest.mark.parametrize("name,flags", FLAG_CASES, ids=[f"{n}-{flag_id(f)}" for n, f in FLAG_CASES])
def test_passes_match_oracle_at_shape(rr, name, flags):
    hip = run_hip(rr, name, flags)
    check_products(hip, name, flags)
    hip.close()


@pytest.mark.parametrize("name,flags", [("edge_depths", ()), ("compressed", ()), ("compressed", (("processed_depth", False),))], ids=["edge_depths", "compressed", "compressed-raw"])
def test_edge_depths_and_compression(rr, name, flags):
    """NaN, +-inf, negative, subnormal raw depths and the limits 0.5 / 4.5 themselves (behind the morph pass, which makes all of them "no return");
    sqrt-coded depth with a different setDepthCompression per stream."""
    hip = run_hip(rr, name, flags)
    check_products(hip, name, flags)
    hip.close()


def test_candidate_list_overflow_with_partial_blocks(rr, monkeypatch):
    """Capacity 1 (test hook) against the 52 candidate blocks of `odd`: all but one take the boundary pass's in-order path, whose block index is split
    by the 7 x 5 block grid of a 100 x 75 image -- candidates lie in its partial last column and row."""
    monkeypatch.setenv("RR_TEST_PRE_CAND_CAP", "1")
    b, counters = oracle_products("odd")
    c = pc.counts(b, counters)
    cand = (b["depth_rg"][..., 0] > 0) & ~(b["depth_rg"][..., 1] > 0.65)
    assert c["candidate_blocks"] >= 10 and cand[:, 64:, :].any() and cand[:, :, 96:].any()
    hip = run_hip(rr, "odd")
    check_products(hip, "odd")
    hip.close()


def full_frame(o, mv, pr, raw_scene=None, proc_scene=None, flags=None):
    if raw_scene is not None:
        o.upload_raw_frame(raw_scene); o.setPreprocess(**(flags or {})); o.clearOccupiedBricks(); o.processTextures()
    else:
        o.upload_frame(proc_scene); o.clearOccupiedBricks(); o.markBricks()
    ratio = o.updateOccupiedBricks()
    o.integrate()
    o.drawF(mv, pr)
    return ratio


@pytest.mark.parametrize("use_bricks", [True, False], ids=["bricks", "dense"])
@pytest.mark.parametrize("flags", [{}, pc.LONE_FLAGS], ids=["default", "unfiltered"])
@pytest.mark.parametrize("name", ["odd", "sensor"])
def test_raw_path_volume_is_exact(rr, monkeypatch, name, flags, use_bricks):
    """The raw path's volume is otherwise compared through tolerances only (quality goes through powf).  Here context A runs the raw frame through the
    passes, and A's OWN products {depth_b, quality, silhouette, normals} are fed as a processed frame to B (upload_frame: packed texel, depth plane and
    8 x 8 range cells from k_pack_frame_fused), to C (the same without the uniform-pair shortcut that reads the range cells) and to the oracle.  All four
    integrate the same quality values, so powf drops out: brick counters, occupied ratio, volume and framebuffer (shade mode 0: no pow()) are equal bit for bit.
    A range cell of k_pre_quality that is NARROWER than its pixels shows here (a wider one only sends its tiles to the full evaluation).  The unfiltered runs
    keep the lone cells of preprocess_cases.plant_edges, which is where a range-cell store past the end of its row (odd) or of its stream (sensor) lands:
    with a lone cell's range lost its tiles are carved.  That pins a cell that is lost for good; an unguarded store (the `cx < rcw && cy < rch` test dropped)
    races with the cell's rightful writer, which has far more work in front of its store and so usually lands last and repairs the cell -- this test sees
    that mutation only when the stray store lands last, not reliably.  Where A differs from B, C and the oracle say which side is wrong."""
    sc, kw = scene(name), kw_of(name)
    mv, pr = rr.scene.default_view(*kw["view"])

    def make(s, **extra):
        o = rr.ReconIntegrationHip(s, **kw, **extra)
        o.setUseBricks(use_bricks); o.setShadeMode(0)
        return o
    a = make(sc, upload=False)
    a.set_calibration(sc)
    ra = full_frame(a, mv, pr, raw_scene=sc, flags=flags)
    sc2 = pc.processed_scene(sc, a.preprocessed(lab=False))
    b = make(sc2)
    monkeypatch.setenv("RR_K1_RANGES", "0")
    c = make(sc2)
    monkeypatch.delenv("RR_K1_RANGES")
    o = OracleRecon(sc2, **kw)
    o.setUseBricks(use_bricks); o.setShadeMode(0)
    ro = full_frame(o, mv, pr, proc_scene=sc2)
    vo, (oc, od) = o.tsdf(), o.framebuffer()
    assert (np.abs(vo) < kw["limit"]).sum() > 100 and (od < 1).sum() > 50 and ro > 0
    for who, x in (("B (processed frame)", b), ("C (processed frame, no range shortcut)", c), ("A (raw frame)", a)):
        r = ra if x is a else full_frame(x, mv, pr, proc_scene=sc2)
        np.testing.assert_array_equal(x.bricks()[0], o.counters(), err_msg=who)
        assert r == ro, f"{who}: occupied ratio {r} != {ro}"
        assert_same(x.tsdf(), vo, f"{who}: volume")
        xc, xd = x.framebuffer()
        assert_same(xd, od, f"{who}: framebuffer depth"); assert_same(xc, oc, f"{who}: framebuffer colour")
    for x in (a, b, c):
        x.close()


def test_odd_size_through_the_lanes(rr):
    """Four moving `odd` frames through tsdf_frame_raw_dev from device arrays, nothing read in between (the lane ahead: morph + filter in front of the
    gate, the colour re-layout alone behind it), against a context with every kernel on one stream running the separate calls."""
    import torch
    scs = [scene("odd"), pc.odd(sphere_c=(0.4, 0.7, -0.3), box_c=(-0.5, 1.5, 0.2)), pc.odd(sphere_c=(-0.3, 1.3, 0.2))]
    kw = pc.KW["odd"]
    pr = rr.scene.gl_flat(rr.scene.perspective(50.0, 16.0 / 9.0, 0.1, 200.0))
    mvs = [rr.scene.gl_flat(rr.scene.look_at(e, (0.0, 1.1, 0.0))) for e in [(0.0, 1.1, 3.0), (1.6, 1.4, 2.4), (-2.2, 0.6, 1.2)]]
    dev = [(torch.from_numpy(np.ascontiguousarray(sc["depth_raw"], np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(sc["color"], np.uint8)).cuda()) for sc in scs]
    torch.cuda.synchronize()
    lanes, serial = rr.ReconIntegrationHip(scs[0], **kw), rr.ReconIntegrationHip(scs[0], **kw)
    serial.set_stage_overlap(False)
    lanes.set_preprocess_calibration(scs[0])
    order = [1, 2, 0, 1]
    for n, k in enumerate(order):
        lanes.frame_raw_dev(mvs[n % 3], pr, new_frame=(dev[k][0].data_ptr(), dev[k][1].data_ptr()), complete=True)
    for n, k in enumerate(order):
        serial.upload_raw_frame(scs[k]); serial.clearOccupiedBricks(); serial.processTextures(); serial.updateOccupiedBricks(False); serial.integrate(); serial.drawF(mvs[n % 3], pr)
    a, b = lanes.preprocessed(), serial.preprocessed()
    for key in a:
        assert_same(a[key], b[key], f"{key}: lanes vs one stream")
    np.testing.assert_array_equal(lanes.bricks()[0], serial.bricks()[0])
    np.testing.assert_array_equal(lanes.raw_frame()[1], serial.raw_frame()[1])
    assert_same(lanes.tsdf(), serial.tsdf(), "volume: lanes vs one stream")
    (lc, ld), (sc_, sd) = lanes.framebuffer(), serial.framebuffer()
    assert_same(ld, sd, "framebuffer depth: lanes vs one stream"); assert_same(lc, sc_, "framebuffer colour: lanes vs one stream")
    assert (sd < 1).sum() > 50 and serial.bricks()[0].sum() > 0 and (np.abs(serial.tsdf()) < kw["limit"]).sum() > 100
    lanes.close(); serial.close()
