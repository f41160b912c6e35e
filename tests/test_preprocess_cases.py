"""The cases of tests/preprocess_cases.py under the oracle alone (CPU only): each must give the passes something to decide, or the device
comparison of tests/test_gpu_preprocess_shapes.py compares empty images.  The floors are well under what the oracle gives (odd: 3 315
candidates in 52 blocks, 452 kept, 2 863 rejected, 4 053 silhouette pixels, 119 bricks; make_scene's own content alone, which stays clear of
every partial block: 2 605 in 30, 204, 2 401, 1 017, 44): a case that misses one is changed, not the floor."""
import numpy as np
import pytest

import preprocess_cases as pc
from helpers import assert_same, same
from oracle.oracle import OracleRecon


def run(sc, kw, flags=None):
    o = OracleRecon(sc, **kw)
    pc.process(o, sc, flags)
    pp = o.preprocessed()
    return o, pp, pc.counts(pp, o.counters())


@pytest.fixture(scope="module")
def odd():
    return pc.odd()


@pytest.fixture(scope="module")
def sensor():
    return pc.sensor()


def test_shapes_are_partial_for_every_tiling(odd, sensor):
    sc = odd
    w, h, n_col = sc["width"], sc["height"], sc["n"] * sc["color_width"] * sc["color_height"]
    assert (w % 16, h % 16, w % 8, h % 8, w % 64, h % 4) == (4, 11, 4, 3, 36, 3) and n_col % 4 == 2
    t = pc.tiny()
    assert t["width"] < 13 and t["height"] < 13 and (t["color_width"], t["color_height"]) != (t["width"], t["height"])
    s = sensor
    assert (s["width"], s["height"]) == (512, 424) and s["height"] % 16 == 8 and (s["color_width"], s["color_height"]) == (320, 270)


def test_odd_has_work_for_every_pass(odd):
    _, _, c = run(odd, pc.KW["odd"])
    assert c["candidates"] >= 1000 and c["candidate_blocks"] >= 10
    assert c["kept"] >= 100 and c["rejected"] >= 1000
    assert c["silhouette"] >= 500 and c["bricks"] >= 10


@pytest.mark.parametrize("case", ["odd", "sensor"])
def test_content_reaches_the_partial_blocks_and_cells(case, odd, sensor):
    """The partial last block column / row (odd: x >= 96, y >= 64) and the partial last 8-cells (x >= 96, y >= 72) hold boundary candidates, kept depths with a
    quality, silhouette pixels and background side by side -- so a wrong clamped tap, block index or range cell there changes a product -- and so does the
    left border.  Most of what lies there is finite (the outermost pixels' normals are NaN by the reference's own rule: both LUT taps clamp to one texel)."""
    sc = dict(odd=odd, sensor=sensor)[case]
    w, h = sc["width"], sc["height"]
    _, pp, _ = run(sc, pc.KW[case])
    cand = (pp["depth_rg"][..., 0] > 0) & ~(pp["depth_rg"][..., 1] > 0.65)
    depth, sil = pp["depth_b"][..., 0] > 0, pp["silhouette"] > 0
    with np.errstate(invalid="ignore"):
        good = pp["quality"] > 0
    bx, by, cx, cy = w // 16 * 16, h // 16 * 16, w // 8 * 8, h // 8 * 8
    assert h > by and (case == "sensor" or (w > cx >= bx and h > cy >= by))     # odd: the last block and the last cell are partial in x and in y; sensor: half a block row
    regions = [("last block row", np.s_[:, by:, :]), ("last cell row", np.s_[:, -(h - cy or 8):, :]), ("first columns", np.s_[:, :, :16]), ("last columns", np.s_[:, :, -16:])]
    if case == "odd":
        regions += [("last block column", np.s_[:, :, bx:]), ("last cell column", np.s_[:, :, cx:]), ("corner block", np.s_[:, by:, bx:])]
    for what, region in regions:
        assert depth[region].sum() >= 3 and sil[region].sum() >= 3 and good[region].sum() >= 3, what
        assert (~depth[region]).any(), what                                     # a range cell there is not uniform
    assert cand[:, by:, :].sum() >= 20
    if case == "odd":
        assert cand[:, :, bx:].sum() >= 3 and depth[0, cy:, cx:].all() and good[0, cy:, cx:].any()     # the 4 x 3 corner cell is full of depth (its quality is mostly NaN, see above)
    assert all(depth[i, -(h - cy or 8):, :].any() for i in range(sc["n"]))                  # every stream has depth in its last cell row


@pytest.mark.parametrize("case", ["odd", "sensor"])
def test_lone_cells_differ_from_all_their_neighbours(case, odd, sensor):
    """Processed unfiltered (LONE_FLAGS), each lone cell of plant_edges is one whole 8 x 8 range cell of kept depth -- silhouette 1, one depth value -- and the
    eight cells around it are background without exception: its range {d, d, 1, 1} is the only thing that keeps the tiles over it from being carved.  The cells
    are those an unguarded range store reaches: (cy, 0) of stream 0 behind cell column 13 = rcw of row cy - 1 (odd), (0, cx) of stream 1 behind cell row
    53 = rch of stream 0 (sensor)."""
    sc = dict(odd=odd, sensor=sensor)[case]
    w, h = sc["width"], sc["height"]
    assert (2 * -(-w // 16) > -(-w // 8)) == (case == "odd") and (2 * -(-h // 16) > -(-h // 8)) == (case == "sensor")   # block cells past the cell grid: in x (odd), in y (sensor)
    _, pp, _ = run(sc, pc.KW[case], pc.LONE_FLAGS)
    d, s = pp["depth_b"][..., 0], pp["silhouette"]
    assert len(pc.lone_cells(sc)) >= 1
    for l, cy, cx, n in pc.lone_cells(sc):
        own = np.s_[l, 8 * cy:8 * cy + 8, 8 * cx:8 * (cx + n)]
        around = np.s_[l, max(8 * cy - 8, 0):8 * cy + 16, max(8 * cx - 8, 0):8 * (cx + n) + 8]
        assert (s[own] == 1).all() and (d[own] > 0).all() and len(np.unique(d[own])) == 1, (l, cy, cx)
        assert (d[around] != 0).sum() == 64 * n and (s[around] != 0).sum() == 64 * n, (l, cy, cx)       # nothing but the cells themselves
        assert (pp["quality"][own] != 0).all(), (l, cy, cx)    # a weight (tiny: 64 of 169 window taps; NaN beside the image border): integrated to sdist or NaN, never to the carved -limit


@pytest.mark.parametrize("flags", pc.ALL_FLAGS)
def test_odd_keeps_a_surface_under_every_flag_combination(odd, flags):
    _, pp, c = run(odd, pc.KW["odd"], flags)
    assert c["silhouette"] >= 500 and c["quality"] >= 500 and c["bricks"] >= 10
    assert (c["candidates"] >= 1000) == flags["filter_textures"]            # (unfiltered: range quality 1 everywhere, nothing for the boundary pass)
    if flags["filter_textures"]:
        assert (c["kept"] >= 100) == flags["refine"] and c["rejected"] >= 1000


def test_tiny_runs_the_fill_and_the_quality_branch():
    sc = pc.tiny()
    _, pp, c = run(sc, pc.KW["tiny"])
    assert c["silhouette"] >= 1 and c["quality"] >= 1
    assert c["candidates"] >= 10 and c["kept"] >= 1 and c["rejected"] >= 1     # the depth step of the last stream
    d2 = pp["depth2"]
    assert sc["depth_raw"][pc.TINY_HOLE_1] == 0 and d2[pc.TINY_HOLE_1] == np.float32(2.5)
    hole = d2[pc.TINY_HOLE_9]
    assert hole[1, 1] == 0 and (np.delete(hole.reshape(-1), 4) == np.float32(2.5)).all()   # rim filled, centre without a valid neighbour
    _, _, c = run(sc, pc.KW["tiny"], pc.TWO_FLAGS[1])
    assert c["silhouette"] >= 1 and c["quality"] >= 1


def test_sensor_has_work_for_every_pass(sensor):
    for flags in pc.TWO_FLAGS:
        _, _, c = run(sensor, pc.KW["sensor"], flags)
        assert c["silhouette"] >= 20000 and c["candidate_blocks"] >= 50


def test_edge_depths_are_defined_behind_the_morph_pass(odd):
    sc = pc.edge_depths(odd)
    _, pp, c = run(sc, pc.KW["odd"])
    raw, d2, kind = sc["depth_raw"], pp["depth2"], sc["planted"]
    assert np.isfinite(d2).all() and np.isfinite(pp["depth_rg"]).all() and np.isfinite(pp["depth_b"]).all()
    for k, (name, v) in enumerate(pc.EDGE_KINDS):
        at = kind == k
        assert at.sum() >= 20, name
        if name in pc.EDGE_KEPT:
            assert (d2[at] == v).all(), name                                   # strictly inside (0.5, 4.5): survives unchanged
        else:
            assert ((d2[at] == 0) | ((d2[at] > 0.5) & (d2[at] < 4.5))).all(), name     # "no return": empty, or the mean of valid neighbours
            assert (d2[at] == 0).any() and (d2[at] > 0.5).any(), name
    assert (kind >= 0).sum() >= raw.size // 60
    assert c["silhouette"] >= 500 and c["candidates"] >= 1000


def test_compressed_streams_differ_and_all_hold_a_surface(odd):
    sc = pc.compressed(odd)
    for flags in (dict(), dict(processed_depth=False)):
        _, pp, c = run(sc, pc.KW["odd"], flags)
        for i in range(sc["n"]):
            assert (pp["silhouette"][i] > 0).sum() >= 100, f"stream {i}"
        assert (pp["depth_rg"][1] != pp["depth_rg"][0]).any()
    _, plain, _ = run(odd, pc.KW["odd"])
    _, pp, _ = run(sc, pc.KW["odd"])
    # uncompress() adds 0.15 * (far - near) / 255 to the squared code: 0.15 * 4 / 255 = 2.35e-3 of the normalised depth -- close to the metres' result, not equal
    both = (pp["depth_rg"][0, ..., 0] > 0) & (plain["depth_rg"][0, ..., 0] > 0)
    diff = np.abs(pp["depth_rg"][0, ..., 0] - plain["depth_rg"][0, ..., 0])[both]
    assert both.sum() >= 500 and np.median(diff) > 2.2e-3 and diff.max() < 2.5e-3
    assert_same(pp["depth_rg"][1], plain["depth_rg"][1], "the uncompressed stream")
    # why stream 1 keeps its metres: the codes, taken for metres as its setDepthCompression(0, ...) says, lie at most 1 m from the camera -- outside the box
    _, lit, _ = run(pc.compressed(odd, coded=(0, 1, 2)), pc.KW["odd"])
    assert (lit["silhouette"][1] > 0).sum() == 0 and (lit["depth_rg"][1] != 0).sum() == 0
    assert (pp["depth_rg"][2] != plain["depth_rg"][2]).mean() > 0.01           # the second near / far pair moves stream 2's surface


@pytest.mark.parametrize("use_bricks", [True, False])
def test_oracle_raw_path_equals_its_processed_path(odd, use_bricks):
    """The premise of test_raw_path_volume_is_exact, on the oracle alone: a processed frame made of the raw path's own products
    {depth_b, quality, silhouette} integrates and draws to the same volume, counters, ratio and framebuffer, bit for bit."""
    kw = pc.KW["odd"]
    mv, pr = pc.rr.scene.default_view(*kw["view"])
    a = OracleRecon(odd, **kw)
    a.setUseBricks(use_bricks)
    a.upload_raw_frame(odd); a.clearOccupiedBricks(); a.processTextures()
    ra = a.updateOccupiedBricks(); a.integrate(); a.drawF(mv, pr)
    sc = pc.processed_scene(odd, a.preprocessed())
    b = OracleRecon(sc, **kw)
    b.setUseBricks(use_bricks)
    b.upload_frame(sc); b.clearOccupiedBricks(); b.markBricks()
    rb = b.updateOccupiedBricks(); b.integrate(); b.drawF(mv, pr)
    assert ra == rb > 0
    np.testing.assert_array_equal(a.counters(), b.counters())
    assert_same(a.tsdf(), b.tsdf(), "volume")
    assert (np.abs(a.tsdf()) < kw["limit"]).sum() > 100
    (ac, ad), (bc, bd) = a.framebuffer(), b.framebuffer()
    assert_same(ad, bd, "framebuffer depth"); assert_same(ac, bc, "framebuffer colour")
    assert (ad < 1).sum() > 50


@pytest.mark.parametrize("case", ["odd", "sensor"])
def test_a_lost_lone_cell_carves_its_voxels(case, odd, sensor):
    """The last step of the argument for the lone cells, on the oracle: a tile whose rectangle of range cells has lost the lone cell's range sees background
    only -- silhouette {0}, depth {0} -- and is classed kPairCarve, i.e. its stream treats every voxel as it would over background pixels.  Emulated by
    turning the cell's 64 pixels into background in the processed frame (dense integration, so the brick counters, which the range cells do not touch, stay
    out of it): for each lone patch alone, at least eight voxels change -- what the device test's bit-for-bit volume comparison notices."""
    sc, kw = dict(odd=odd, sensor=sensor)[case], pc.KW[case]

    def volume(frame):
        o = OracleRecon(frame, **kw)
        o.setUseBricks(False)
        o.upload_frame(frame); o.integrate()
        return o.tsdf()
    _, pp, _ = run(sc, kw, pc.LONE_FLAGS)
    whole = pc.processed_scene(sc, pp)
    v = volume(whole)
    for l, cy, cx, n in pc.lone_cells(sc):
        lost = dict(whole)
        for key in ("depth", "quality", "silhouette"):
            lost[key] = whole[key].copy()
            lost[key][l, 8 * cy:8 * cy + 8, 8 * cx:8 * (cx + n)] = 0
        changed = ~same(volume(lost), v)
        assert changed.sum() >= 8, (l, cy, cx, int(changed.sum()))
