"""-m gpu: the stateful shortcuts of the frame loop against state-free runs.

  * image-space dirty tiles (peel clear + march skip): a sequence of frames with a moving camera, moving objects and
    toggled options through ONE context equals a fresh context per frame, bit for bit;
  * two-pass march (rays handed to k_march_long after RR_MARCH_CAP samples) equals the single-pass march bit for bit,
    on frames where rays really are handed over;
  * every foreign write of the framebuffer forces exactly one full hole-filling pass, against a twin without the shortcuts;
  * at BASELINE.json's full size (512^3 x 4 streams, 1280x720) the same through size-independent properties:
    idempotence, culled == dense inside the occupied bricks, slab partition == whole volume, wire upload == raw upload.
"""
import os
from contextlib import contextmanager

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(res=(64, 64, 64), brick_size=[2.0 / 8, 2.2 / 8, 2.0 / 8], limit=0.04, view=(160, 90))


@contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def frame(o, mv, pr):
    o.clearOccupiedBricks(); o.markBricks(); o.updateOccupiedBricks(False)
    o.integrate()
    o.drawF(mv, pr)


def outputs(o):
    rgba, d, ns, pe = o.view_images()
    fc, fd = o.framebuffer()
    return dict(rgba=rgba, depth=d, nsamples=ns, fb_color=fc, fb_depth=fd)


def assert_same(a, b, what):
    for k in a:
        same = (a[k] == b[k]) | (np.isnan(a[k]) & np.isnan(b[k]))
        assert same.all(), f"{what}: {k} differs in {(~same).sum()} of {same.size} values"


def views(rr, w, h):
    pr = rr.scene.gl_flat(rr.scene.perspective(50.0, w / float(h), 0.1, 200.0))
    eyes = [(0.0, 1.1, 3.0), (1.6, 1.4, 2.4), (-2.2, 0.6, 1.2), (0.0, 1.1, 3.0)]
    return [(rr.scene.gl_flat(rr.scene.look_at(e, (0.0, 1.1, 0.0))), pr) for e in eyes]


def test_image_tile_history_equals_fresh_contexts(rr):
    kw = dict(n_streams=3, width=128, height=96, lut_res=24, inv_res=32)
    scenes = [rr.scene.make_scene(**kw), rr.scene.make_scene(sphere_c=(0.4, 0.7, -0.3), box_c=(-0.5, 1.5, 0.2), **kw)]
    one = rr.ReconIntegrationHip(scenes[0], **KW)
    steps = []
    for vi, (mv, pr) in enumerate(views(rr, *KW["view"])):
        steps.append((scenes[vi % 2], mv, pr, dict()))
    mv0, pr0 = views(rr, *KW["view"])[0]
    steps += [(scenes[0], mv0, pr0, dict(skip=False)), (scenes[1], mv0, pr0, dict(skip=True)),       # history dropped and rebuilt
              (scenes[1], mv0, pr0, dict(fill=False)), (scenes[0], mv0, pr0, dict(fill=True)), (scenes[0], mv0, pr0, dict())]
    skip, fill = True, True
    touched_any = []
    for i, (sc, mv, pr, opt) in enumerate(steps):
        skip, fill = opt.get("skip", skip), opt.get("fill", fill)
        fresh = rr.ReconIntegrationHip(sc, **KW)
        for o in (one, fresh):
            o.setSpaceSkip(skip); o.setColorFilling(fill)
        one.upload_frame(sc)
        frame(one, mv, pr); frame(fresh, mv, pr)
        a, b = outputs(one), outputs(fresh)
        assert_same(a, b, f"step {i}")
        touched_any.append((b["depth"] < 1).sum())
    assert min(touched_any) > 100 and len(set(touched_any)) > 3            # the frames really differ


FOREIGN_WRITERS = ["drawPoints", "drawTrigrid", "drawCalibVis", "drawFrustums", "drawBBox", "drawOccupiedBricks", "drawTextures0", "drawTextures1",
                   "set_framebuffer"]


@pytest.fixture(scope="module")
def tile_scenes(rr):
    kw = dict(n_streams=3, width=128, height=96, lut_res=24, inv_res=32)
    return [rr.scene.make_scene(**kw), rr.scene.make_scene(sphere_c=(0.4, 0.7, -0.3), box_c=(-0.5, 1.5, 0.2), **kw)]


@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("writer", FOREIGN_WRITERS)
def test_foreign_framebuffer_write_forces_one_full_hole_filling(rr, tile_scenes, writer, overlap):
    """Whoever else writes the framebuffer -- a point or triangle-grid draw, an overlay, the texture view, an uploaded framebuffer -- costs the
    hole filling exactly one pass through every tile: the pass after it.  A twin without tile history and without hole filling by tiles
    (RR_IMAGE_TILES=0, RR_FILL_TILES=0) goes through the same calls and must show the same pictures, bit for bit."""
    w, h = KW["view"]
    mv, pr = views(rr, w, h)[0]
    one = rr.ReconIntegrationHip(tile_scenes[0], **KW)
    with env(RR_IMAGE_TILES=0, RR_FILL_TILES=0):
        twin = rr.ReconIntegrationHip(tile_scenes[0], **KW)
    both = (one, twin)
    for o in both:
        o.set_stage_overlap(overlap)
    touched = np.zeros((h, w), bool)
    n = [0]

    def step(what):
        for o in both:
            o.upload_frame(tile_scenes[n[0] % 2]); frame(o, mv, pr)
        n[0] += 1
        a, b = outputs(one), outputs(twin)
        assert_same(a, b, what)
        np.logical_or(touched, b["depth"] < 1, out=touched)

    for k in range(3):
        step(f"frame {k}")
    assert one.fill_stats() == (3, 1)                                       # the third draw of a history is the first to fill by tiles
    rng = np.random.default_rng(11)
    image = rng.random((h, w, 4), dtype=np.float32), rng.random((h, w), dtype=np.float32)
    for o in both:
        if writer == "drawPoints":
            o.upload_normals(tile_scenes[0]["normals"]); o.drawPoints(mv, pr)
        elif writer == "drawTextures0":
            o.drawTextures(0)
        elif writer == "drawTextures1":
            o.drawTextures(1)
        elif writer == "set_framebuffer":
            o.set_framebuffer(*image)
        else:
            getattr(o, writer)(mv, pr)
    (ac, ad), (bc, bd) = one.framebuffer(), twin.framebuffer()
    assert_same(dict(fb_color=ac, fb_depth=ad), dict(fb_color=bc, fb_depth=bd), writer)
    step("first frame after the write")
    assert one.fill_stats() == (4, 1)                                       # every tile: the framebuffer held someone else's pixels
    step("second frame after the write")
    assert one.fill_stats() == (5, 2)                                       # ... and only that once
    assert twin.fill_stats() == (5, 0)
    tiles = touched[:h // 8 * 8, :w // 8 * 8].reshape(h // 8, 8, w // 8, 8).any(axis=(1, 3))
    assert not tiles.all() and tiles.any()                                  # a tile no draw touched: there a pass by tiles and a full pass can differ


def test_two_pass_march_equals_single_pass(rr, small_scene):
    """Small cap so that most marching rays are handed to the 8-lanes-per-ray pass."""
    mv, pr = rr.scene.default_view(*KW["view"])
    res = {}
    for cap in (0, 2, 8):
        with env(RR_MARCH_CAP=cap):
            o = rr.ReconIntegrationHip(small_scene, **KW)
        frame(o, mv, pr)
        frame(o, mv, pr)                                                    # second frame: alternating hit/long counters
        res[cap] = outputs(o)
    n = np.rint(np.abs(res[0]["nsamples"]) / 0.0027)
    assert (n > 8).sum() > 200 and (n > 2).sum() > 1000                     # rays that outlive both caps exist
    assert_same(res[2], res[0], "cap 2")
    assert_same(res[8], res[0], "cap 8")


# ---------------------------------------------------------------------------------------------- BASELINE.json full size
@pytest.fixture(scope="module")
def full(rr):
    scene = rr.scene.make_scene(n_streams=4, width=640, height=480, lut_res=128, inv_res=128)
    ext = scene["bbox_max"] - scene["bbox_min"]
    kw = dict(res=(512, 512, 512), brick_size=[float(ext[a]) / 512 * 8 for a in range(3)], limit=0.01, view=(1280, 720))
    mv, pr = rr.scene.default_view(1280, 720)
    return scene, kw, mv, pr


def test_full_size_idempotent_and_two_pass(rr, full):
    scene, kw, mv, pr = full
    a = rr.ReconIntegrationHip(scene, **kw)
    frame(a, mv, pr)
    first = outputs(a)
    v1 = a.tsdf()
    frame(a, mv, pr)                                                        # same input again: every dirty-state shortcut is a no-op
    assert_same(outputs(a), first, "second frame")
    assert (a.tsdf() == v1).all()
    n = np.rint(np.abs(first["nsamples"]) / 0.0027)
    assert (n > 24).sum() > 1000 and n.max() > 64                           # long rays went through k_march_long (default cap 24)
    with env(RR_MARCH_CAP=0, RR_IMAGE_TILES=0):
        b = rr.ReconIntegrationHip(scene, **kw)
    frame(b, mv, pr)
    assert_same(outputs(b), first, "single-pass march, no tile history")
    assert (first["depth"] < 1).sum() > 40000


def test_full_size_culled_equals_dense_inside_occupied_bricks(rr, full):
    scene, kw, mv, pr = full
    a, b = rr.ReconIntegrationHip(scene, **kw), rr.ReconIntegrationHip(scene, **kw)
    b.setUseBricks(False)
    for o in (a, b):
        o.clearOccupiedBricks(); o.markBricks(); o.updateOccupiedBricks(False); o.integrate()
    va, vb = a.tsdf(), b.tsdf()
    flags = a.bricks()[1].astype(bool)
    # the voxel lists of the occupied bricks (VolumeSampler::containedVoxels; the brick grid is 64 x 65 x 64 here: fp32 sliver)
    from oracle.oracle import OracleRecon
    ranges = OracleRecon(scene, **kw).brick_ranges()
    assert len(ranges) == flags.size and 0.002 < flags.mean() < 0.05
    mask = np.zeros(va.shape, bool)
    for lo_x, lo_y, lo_z, hi_x, hi_y, hi_z in ranges[flags]:
        mask[lo_z:hi_z, lo_y:hi_y, lo_x:hi_x] = True
    assert (va[mask] == vb[mask]).all()                                     # drawn voxels: identical to the dense pass
    assert (va[~mask] == np.float32(-0.01)).all()                           # everything else holds the clear value (:249-250)
    assert (vb[~mask] != np.float32(-0.01)).mean() > 0.01                   # ... where the dense pass does write other values


def test_full_size_slab_partition_equals_whole_volume(rr, full):
    import torch  # noqa: F401
    from importlib import import_module
    mgpu = import_module("rgbd-recon_amd.multigpu")
    scene, kw, mv, pr = full
    whole = rr.ReconIntegrationHip(scene, **kw)
    frame(whole, mv, pr)
    slabs = [rr.ReconIntegrationHip(scene, slab=mgpu.slab_range(512, k, 2), recompute_halo=True, **kw) for k in range(2)]
    mgpu.frame_slabs_on_one_device(slabs, mv, pr, "cuda:0", halo="recompute", composite="compact")
    (wa, wd, wn, _), (sa, sd, sn, _) = whole.view_images(), slabs[0].view_images()
    assert (sd == wd).all() and (sn == wn).all() and ((sa == wa) | (np.isnan(sa) & np.isnan(wa))).all()
    (wc, wdd), (sc, sdd) = whole.framebuffer(), slabs[0].framebuffer()
    assert (sdd == wdd).all() and ((sc == wc) | (np.isnan(sc) & np.isnan(wc))).all()


def test_full_size_wire_upload_equals_raw_upload(rr, full):
    scene, kw, mv, pr = full
    a, b = rr.ReconIntegrationHip(scene, **kw), rr.ReconIntegrationHip(scene, **kw)
    a.upload_raw_frame(scene)
    b.setWireFormat(rr.COLOR_RGB8, rr.DEPTH_F32)
    b.upload_wire_frame(rr.scene.make_wire_message(scene, 0, 0), scene)
    for o in (a, b):
        o.clearOccupiedBricks(); o.processTextures(); o.updateOccupiedBricks(False); o.integrate(); o.drawF(mv, pr)
    assert_same(outputs(a), outputs(b), "wire vs raw")
    pa, pb = a.preprocessed(), b.preprocessed()
    for k in pa:
        assert ((pa[k] == pb[k]) | (np.isnan(pa[k]) & np.isnan(pb[k]))).all(), k


# ---------------------------------------------------------------------------------------------- the lane ahead (csrc/lane_ahead.hpp)
@pytest.fixture(scope="module")
def lane_scenes(rr):
    """four frames of a moving two-stream scene, on the host and (pre-processed and raw) in device memory"""
    import torch
    kw = dict(n_streams=2, width=128, height=96, lut_res=24, inv_res=32)
    moves = [dict(), dict(sphere_c=(0.4, 0.7, -0.3), box_c=(-0.5, 1.5, 0.2)), dict(sphere_c=(-0.3, 1.3, 0.2)), dict(sphere_c=(0.1, 0.9, 0.4), box_c=(0.4, 1.2, -0.4))]
    scs = [rr.scene.make_scene(**kw, **m) for m in moves]
    dev = [{k: torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ("depth", "quality", "silhouette", "color", "depth_raw")} for sc in scs]
    torch.cuda.synchronize()
    return scs, dev


def _bricks(o):
    o.clearOccupiedBricks(); o.markBricks(); o.updateOccupiedBricks(False)


def _plain(o, k, scs, dev, mv, pr):
    o.upload_frame(scs[k]); _bricks(o); o.integrate(); o.drawF(mv, pr)


def _two_clears(o, k, scs, dev, mv, pr):
    o.upload_frame(scs[k]); o.clearOccupiedBricks(); o.clearOccupiedBricks(); o.markBricks(); o.updateOccupiedBricks(False); o.integrate(); o.drawF(mv, pr)


def _two_updates(o, k, scs, dev, mv, pr):
    o.upload_frame(scs[k]); _bricks(o); o.updateOccupiedBricks(False); o.integrate(); o.drawF(mv, pr)


def _two_uploads(o, k, scs, dev, mv, pr):
    o.upload_frame(scs[(k + 1) % 4]); o.upload_frame(scs[k]); _bricks(o); o.integrate(); o.drawF(mv, pr)


def _upload_without_colour(o, k, scs, dev, mv, pr):
    """the second upload of the frame brings new images and no colour: the slot has flipped, the first upload's colour stays"""
    d = dev[(k + 1) % 4]
    o.upload_frame(scs[k]); o.upload_frame_dev(d["depth"].data_ptr(), d["quality"].data_ptr(), d["silhouette"].data_ptr(), 0, complete=True)
    _bricks(o); o.integrate(); o.drawF(mv, pr)


def _draw_between_mark_and_update(o, k, scs, dev, mv, pr):
    o.upload_frame(scs[k]); o.clearOccupiedBricks(); o.markBricks(); o.drawF(mv, pr); o.updateOccupiedBricks(False); o.integrate(); o.drawF(mv, pr)


def _ratio_between_clear_and_mark(o, k, scs, dev, mv, pr):
    o.upload_frame(scs[k]); o.clearOccupiedBricks(); o.occupiedRatio(); o.markBricks(); o.updateOccupiedBricks(False); o.integrate(); o.drawF(mv, pr)


def _integrate_before_the_clear(o, k, scs, dev, mv, pr):
    o.upload_frame(scs[k]); o.integrate(); _bricks(o); o.integrate(); o.drawF(mv, pr)


def _new_brick_size(o, k, scs, dev, mv, pr):
    if k in (0, 2):                                          # (frame 0: the size the context was created with, or back to it)
        o.setBrickSize(KW["brick_size"] if k == 0 else [2.0 / 6, 2.2 / 6, 2.0 / 6])
    _plain(o, k, scs, dev, mv, pr)


def _stage_overlap_off_and_on(o, k, scs, dev, mv, pr):
    """off and on again in front of frame 1; frame 2 runs with it off (the context's stream takes over what the lane left), frame 3 with it on again"""
    if o.lanes_on:
        if k == 1:
            o.set_stage_overlap(False); o.set_stage_overlap(True)
        elif k >= 2:
            o.set_stage_overlap(k == 3)
    _plain(o, k, scs, dev, mv, pr)


def _select_frame_slot(o, k, scs, dev, mv, pr):
    if k == 2:
        o.select_frame_slot(o.current_frame_slot())          # an explicit slot call: the lanes are off from here on
    _plain(o, k, scs, dev, mv, pr)


def _raw_fused_and_separate(o, k, scs, dev, mv, pr):
    """tsdf_frame_raw_dev defers the lane's gate wait behind its first two passes; the separate calls do not"""
    d = dev[k]
    if k % 2 == 0:
        o.frame_raw_dev(mv, pr, new_frame=(d["depth_raw"].data_ptr(), d["color"].data_ptr()), complete=True)
    else:
        o.upload_raw_frame_dev(d["depth_raw"].data_ptr(), d["color"].data_ptr(), complete=True)
        o.clearOccupiedBricks(); o.processTextures(); o.updateOccupiedBricks(False); o.integrate(); o.drawF(mv, pr)


LANE_ORDERS = [_plain, _two_clears, _two_updates, _two_uploads, _upload_without_colour, _draw_between_mark_and_update, _ratio_between_clear_and_mark,
               _integrate_before_the_clear, _new_brick_size, _stage_overlap_off_and_on, _select_frame_slot, _raw_fused_and_separate]


@pytest.mark.parametrize("order", LANE_ORDERS, ids=lambda f: f.__name__.lstrip("_"))
def test_lane_ahead_call_orders_equal_one_stream(rr, lane_scenes, order):
    """The lane ahead prepares frame f + 1 while the context's stream works on frame f; frame slot, brick counters and occupancy set alternate
    under it (csrc/lane_ahead.hpp).  Every per-frame call order that reaches another branch of that bookkeeping, over four frames that differ
    from one another (a read of the wrong slot, counter buffer or occupancy set shows), against a twin created with every kernel on one stream:
    volume, brick counters and flags, occupied ratio and framebuffer, bit for bit -- first the four frames queued back to back with nothing
    read in between (the lanes really overlap), then the four frames again with everything read back behind each."""
    scs, dev = lane_scenes
    vs = views(rr, *KW["view"])
    lanes, twin = rr.ReconIntegrationHip(scs[0], **KW), rr.ReconIntegrationHip(scs[0], lane_flags=rr.LANES_ONE_STREAM, **KW)
    lanes.lanes_on, twin.lanes_on = True, False
    for o in (lanes, twin):
        o.set_preprocess_calibration(scs[0])

    def compare(what):
        assert_same(dict(tsdf=lanes.tsdf()), dict(tsdf=twin.tsdf()), what)
        (lc, lf), (tc, tf) = lanes.bricks(), twin.bricks()
        np.testing.assert_array_equal(lc, tc, err_msg=f"{what}: brick counters"); np.testing.assert_array_equal(lf, tf, err_msg=f"{what}: brick flags")
        assert lanes.occupiedRatio() == twin.occupiedRatio(), what
        a, b = outputs(lanes), outputs(twin)
        assert_same(dict(fb_color=a["fb_color"], fb_depth=a["fb_depth"]), dict(fb_color=b["fb_color"], fb_depth=b["fb_depth"]), what)
        return twin.tsdf(), b["fb_depth"]

    for k in range(4):
        for o in (lanes, twin):
            order(o, k, scs, dev, *vs[k])
    compare("four frames back to back")
    seen = []
    for k in range(4):
        for o in (lanes, twin):
            order(o, k, scs, dev, *vs[k])
        seen.append(compare(f"frame {k}, read back"))
    assert all((d < 1).sum() > 100 for _, d in seen)
    for a in range(4):
        for b in range(a + 1, 4):
            assert (seen[a][0] != seen[b][0]).any(), f"frames {a} and {b} leave the same volume"


# ---------------------------------------------------------------------------------------------- the integrate and fill lanes (csrc/draw_lanes.hpp)
def _march_then_integrate(o, k, scs, dev, mv, pr):
    """frames 0 and 2: a march with no fillColors() behind it -- the next integrate() marks the draw's end itself; frames 1 and 3: the two calls apart"""
    o.upload_frame(scs[k]); _bricks(o); o.integrate(); o.draw(mv, pr)
    if k % 2:
        o.fillColors()


def _two_integrates(o, k, scs, dev, mv, pr):
    """another frame integrated first: two integrates with no draw in between, each into the other volume set"""
    o.upload_frame(scs[(k + 1) % 4]); _bricks(o); o.integrate()
    _plain(o, k, scs, dev, mv, pr)


def _two_draws(o, k, scs, dev, mv, pr):
    o.upload_frame(scs[k]); _bricks(o); o.integrate(); o.drawF(*o.vs[(k + 1) % 4]); o.drawF(mv, pr)


def _hole_filling_off(o, k, scs, dev, mv, pr):
    """off for frames 1 and 2: one pyramid, no fill lane, the march writes the framebuffer"""
    o.setColorFilling(k in (0, 3))
    _plain(o, k, scs, dev, mv, pr)


def _bbox_after_draw(o, k, scs, dev, mv, pr):
    _plain(o, k, scs, dev, mv, pr); o.drawBBox(mv, pr)


def _mesh_stream_after_draw(o, k, scs, dev, mv, pr):
    """the frame's mesh behind its draw; every slot is taken and released two frames late"""
    if not hasattr(o, "meshes"):
        o.mesh_stream_config(normals=True, colours=True, max_vertices=1 << 18, max_triangles=1 << 19, max_surface_tiles=1 << 12, slots=4)
        o.meshes, o.meshed = [], 0
    _plain(o, k, scs, dev, mv, pr)
    o.mesh_stream(tag=o.meshed)
    o.meshed += 1
    if o.meshed > 2:
        v, t, info = o.mesh_stream_take(wait=True)
        assert info["overflow"] == 0 and info["tag"] == o.meshed - 3 and info["n_triangles"] > 100
        o.meshes.append((v.tobytes(), t.tobytes()))


def _present_after_draw(o, k, scs, dev, mv, pr):
    """the frame's read-out behind its draw; acquired and released one frame late"""
    if not hasattr(o, "presented"):
        o.present_config(slots=3)
        o.presented, o.n_presented = [], 0
    _plain(o, k, scs, dev, mv, pr)
    o.present(tag=o.n_presented)
    o.n_presented += 1
    if o.n_presented > 1:
        a, tag, _ = o.present_acquire(wait=True)
        assert tag == o.n_presented - 2
        o.presented.append(a.tobytes())
        o.present_release()


def _timers_for_one_frame(o, k, scs, dev, mv, pr):
    """timers on: the hole filling is queued by the caller's thread, behind whatever the helper thread still holds"""
    o.enable_timers(k == 1)
    _plain(o, k, scs, dev, mv, pr)
    o.enable_timers(False)


DRAW_LANE_ORDERS = [_plain, _march_then_integrate, _two_integrates, _two_draws, _hole_filling_off, _bbox_after_draw, _mesh_stream_after_draw, _present_after_draw,
                    _stage_overlap_off_and_on, _timers_for_one_frame]
DRAW_LANE_CASES = [(f, None) for f in DRAW_LANE_ORDERS] + [(f, flag) for flag in ("LANES_NO_FILL_THREAD", "LANES_NO_INTEGRATE_LANE") for f in (_plain, _bbox_after_draw)]


@pytest.mark.parametrize("order,flag", DRAW_LANE_CASES, ids=[f.__name__.lstrip("_") + ("-" + flag[6:].lower() if flag else "") for f, flag in DRAW_LANE_CASES])
def test_draw_lane_call_orders_equal_one_stream(rr, lane_scenes, order, flag):
    """integrate() of frame f + 1 runs on a lane of its own beside the draw of frame f, the hole filling of draw f on another (issued by a helper
    thread) beside whatever follows; two volume sets and two pyramids alternate under them (csrc/draw_lanes.hpp).  Every call order that reaches
    another branch of that bookkeeping, over four frames that differ from one another (a read of the wrong set or pyramid, an integrate that
    overtakes the draw of its set, a fill that overtakes its march shows), against a twin created with every kernel on one stream: volume,
    brick state and framebuffer, bit for bit, and what the mesh stream and the read-out delivered -- first the four frames back to back with
    nothing read in between, then again with everything read back behind each.  plain and the overlay order also without the helper thread
    and without the integrate lane."""
    scs, dev = lane_scenes
    vs = views(rr, *KW["view"])
    lanes = rr.ReconIntegrationHip(scs[0], lane_flags=getattr(rr, flag) if flag else 0, **KW)
    twin = rr.ReconIntegrationHip(scs[0], lane_flags=rr.LANES_ONE_STREAM, **KW)
    lanes.lanes_on, twin.lanes_on = True, False
    lanes.vs = twin.vs = vs

    def compare(what):
        assert_same(dict(tsdf=lanes.tsdf()), dict(tsdf=twin.tsdf()), what)
        (lc, lf), (tc, tf) = lanes.bricks(), twin.bricks()
        np.testing.assert_array_equal(lc, tc, err_msg=f"{what}: brick counters"); np.testing.assert_array_equal(lf, tf, err_msg=f"{what}: brick flags")
        a, b = outputs(lanes), outputs(twin)
        assert_same(dict(fb_color=a["fb_color"], fb_depth=a["fb_depth"]), dict(fb_color=b["fb_color"], fb_depth=b["fb_depth"]), what)
        return twin.tsdf(), b["fb_depth"]

    for k in range(4):
        for o in (lanes, twin):
            order(o, k, scs, dev, *vs[k])
    compare("four frames back to back")
    seen = []
    for k in range(4):
        for o in (lanes, twin):
            order(o, k, scs, dev, *vs[k])
        seen.append(compare(f"frame {k}, read back"))
    assert all((d < 1).sum() > 100 for _, d in seen)
    for a in range(4):
        for b in range(a + 1, 4):
            assert (seen[a][0] != seen[b][0]).any(), f"frames {a} and {b} leave the same volume"
    for what in ("meshes", "presented"):
        got, want = getattr(lanes, what, []), getattr(twin, what, [])
        assert len(got) == len(want) and all(g == w for g, w in zip(got, want)), f"{what}: the lanes delivered something else"
        assert not hasattr(lanes, what) or (len(got) >= 6 and len(set(got)) >= 4)


# ---------------------------------------------------------------------------------------------- the frame intake (csrc/frame_intake.hpp)
TSDF_ERR_STATE = -4
WINDOW = (3.0, 2.0, 40.0, 50.0)


def _process(o, mv, pr):
    o.clearOccupiedBricks(); o.processTextures(); o.updateOccupiedBricks(False); o.integrate(); o.drawF(mv, pr)


def _raw_dev(o, d):
    o.upload_raw_frame_dev(d["depth_raw"].data_ptr(), d["color"].data_ptr(), complete=True)


def _raw_host_then_process(o, k, scs, dev, mv, pr):
    o.upload_raw_frame(scs[k]); _process(o, mv, pr)


def _wire_both_buffers(o, k, scs, dev, mv, pr):
    """every message takes the other pinned buffer; from the third on its previous copy has to have left it"""
    o.upload_wire_frame(o.messages[k]); _process(o, mv, pr)


def _raw_download_before_process(o, k, scs, dev, mv, pr):
    """the read-back asks for the colour the first pass would have re-laid out"""
    _raw_dev(o, dev[k])
    o.delivered += [a.tobytes() for a in o.raw_frame()]
    _process(o, mv, pr)


def _process_twice(o, k, scs, dev, mv, pr):
    """the second run finds the colour taken and the slot written"""
    _raw_dev(o, dev[k]); o.clearOccupiedBricks(); o.processTextures(); o.processTextures(); o.updateOccupiedBricks(False); o.integrate(); o.drawF(mv, pr)


def _points_then_process(o, k, scs, dev, mv, pr):
    """the point draw reads the normal image the next frame's passes rewrite"""
    _raw_dev(o, dev[k]); _process(o, mv, pr); o.drawPoints(mv, pr)


def _mvt_then_raw_upload(o, k, scs, dev, mv, pr):
    """the MVT draw reads the raw depth the next upload (host, then wire) rewrites"""
    if k % 2:
        o.upload_wire_frame(o.messages[k])
    else:
        o.upload_raw_frame(scs[k])
    _process(o, mv, pr); o.drawMVT(mv, pr)


def _windows_then_process(o, k, scs, dev, mv, pr):
    """windows on the single-buffered products (type 6 also reads the raw depth) in front of the next frame's upload and passes"""
    o.upload_raw_frame(scs[k]); _process(o, mv, pr)
    for n, type in enumerate((1, 3, 5, 6)):
        o.drawSensorTexture(type, (k + n) % 2, (WINDOW[0] + 30 * n, WINDOW[1], WINDOW[2] + 30 * n, WINDOW[3]))


def _async_upload_and_select(o, k, scs, dev, mv, pr):
    o.upload_frame_async(scs[k]); o.select_frame_slot(1 - o.current_frame_slot())
    _bricks(o); o.integrate(); o.drawF(mv, pr)


def _preprocessed_after_raw(o, k, scs, dev, mv, pr):
    """a raw frame nobody processes, a pre-processed one over it"""
    _raw_dev(o, dev[(k + 1) % 4]); o.upload_frame(scs[k]); _bricks(o); o.integrate(); o.drawF(mv, pr)


INTAKE_ORDERS = [_raw_host_then_process, _wire_both_buffers, _raw_download_before_process, _process_twice, _points_then_process, _mvt_then_raw_upload,
                 _windows_then_process, _async_upload_and_select, _preprocessed_after_raw]


def _raises_state(rr, call):
    with pytest.raises(rr.TsdfError) as e:
        call()
    assert e.value.code == TSDF_ERR_STATE


def _state_verdicts(rr, o, scs):
    """what the intake's state allows, absolutely: nothing of a raw frame before it is processed; of a frame handed over processed no morphed depth,
    no Lab image and no normals until some are uploaded; no Lab image once a newer raw frame has replaced the processed one's inputs"""
    o.upload_raw_frame(scs[0])
    for type in range(7):
        _raises_state(rr, lambda: o.drawSensorTexture(type, 0, WINDOW))
    o.clearOccupiedBricks(); o.processTextures()
    for type in range(7):
        o.drawSensorTexture(type, 1, WINDOW)
    assert set(o.preprocessed()) >= {"lab", "normals"}
    o.upload_raw_frame(scs[1])
    _raises_state(rr, o.preprocessed)
    assert "lab" not in o.preprocessed(lab=False)
    o.upload_frame(scs[2])
    for type in (3, 5, 6):
        _raises_state(rr, lambda: o.drawSensorTexture(type, 0, WINDOW))
    for type in (0, 1, 2, 4):
        o.drawSensorTexture(type, 0, WINDOW)
    o.upload_normals(scs[2]["normals"])
    o.drawSensorTexture(3, 0, WINDOW)
    for type in (5, 6):
        _raises_state(rr, lambda: o.drawSensorTexture(type, 0, WINDOW))


@pytest.mark.parametrize("order", INTAKE_ORDERS, ids=lambda f: f.__name__.lstrip("_"))
def test_frame_intake_call_orders_equal_one_stream(rr, lane_scenes, order):
    """Which frame slot is current and what it holds, the two pinned rings, the raw frame and what was made of it, the three read fences behind
    draws that read single-buffered images (csrc/frame_intake.hpp): every per-frame call order that reaches a branch of that bookkeeping the
    orders above do not, over the same four frames against the same one-stream twin -- volume, brick counters and flags, framebuffer (with
    whatever the order drew over it), bit for bit, back to back and then read back behind each frame; and what a read-back in the middle of a
    frame delivered.  Then the state verdicts on both contexts, absolutely."""
    scs, dev = lane_scenes
    vs = views(rr, *KW["view"])
    lanes, twin = rr.ReconIntegrationHip(scs[0], **KW), rr.ReconIntegrationHip(scs[0], lane_flags=rr.LANES_ONE_STREAM, **KW)
    messages = [rr.scene.make_wire_message(sc, 0, 0) for sc in scs]
    for o in (lanes, twin):
        o.set_preprocess_calibration(scs[0])
        o.messages, o.delivered = messages, []

    def compare(what):
        assert_same(dict(tsdf=lanes.tsdf()), dict(tsdf=twin.tsdf()), what)
        (lc, lf), (tc, tf) = lanes.bricks(), twin.bricks()
        np.testing.assert_array_equal(lc, tc, err_msg=f"{what}: brick counters"); np.testing.assert_array_equal(lf, tf, err_msg=f"{what}: brick flags")
        a, b = outputs(lanes), outputs(twin)
        assert_same(dict(fb_color=a["fb_color"], fb_depth=a["fb_depth"]), dict(fb_color=b["fb_color"], fb_depth=b["fb_depth"]), what)
        return twin.tsdf(), b["fb_depth"], b["depth"]

    for k in range(4):
        for o in (lanes, twin):
            order(o, k, scs, dev, *vs[k])
    compare("four frames back to back")
    seen = []
    for k in range(4):
        for o in (lanes, twin):
            order(o, k, scs, dev, *vs[k])
        seen.append(compare(f"frame {k}, read back"))
    # The pictures are not empty.  The bound of 100 pixels is the march's, as in the tests above; an MVT draw REPLACES the framebuffer by the mesh of
    # the 128 x 96 raw depth images, whose cover is tests/test_gpu_mvt.py's matter: there the march's own depth image carries the bound, and the
    # framebuffer has to show a mesh at all.
    assert all((m < 1).sum() > 100 for _, _, m in seen)
    assert all((d < 1).sum() > (0 if order is _mvt_then_raw_upload else 100) for _, d, _ in seen)
    for a in range(4):
        for b in range(a + 1, 4):
            assert (seen[a][0] != seen[b][0]).any(), f"frames {a} and {b} leave the same volume"
    assert lanes.delivered == twin.delivered and (order is not _raw_download_before_process or len(set(lanes.delivered[0::2])) == 4)   # (the four raw depth images)
    for o in (lanes, twin):
        _state_verdicts(rr, o, scs)
