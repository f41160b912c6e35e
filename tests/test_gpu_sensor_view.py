"""-m gpu: the GUI's "Show textures" windows (tsdf_draw_sensor_texture) against tests/sensor_view_reference.py.  Every comparison is bit
for bit: the reference is fed the framebuffer downloaded just before the call and the source array as the library itself returns it
(preprocessed(), raw_frame(), the uploaded arrays) -- the products themselves are pinned to the oracle by test_gpu_preprocess.py."""
import ctypes as C

import numpy as np
import pytest

import sensor_view_reference as S
from helpers import assert_same, same

pytestmark = pytest.mark.gpu

TSDF_ERR_INVALID_ARGUMENT, TSDF_ERR_STATE = -1, -4
VIEW = (160, 90)
KW = dict(res=(64, 64, 64), brick_size=[2.0 / 8, 2.2 / 8, 2.0 / 8], limit=0.04, view=VIEW)
RECT = (3.25, 2.5, 3.25 + 40.0, 2.5 + 53.375)                             # ImGui cursor positions are not integers


def random_framebuffer(hip, seed=7):
    rng = np.random.default_rng(seed)
    w, h = hip.view
    fc = rng.uniform(-1, 2, (h, w, 4)).astype(np.float32)
    fd = rng.uniform(0, 1, (h, w)).astype(np.float32)
    hip.set_framebuffer(fc, fd)
    return fc, fd


def raw_processed(rr, scene, **kw):
    hip = rr.ReconIntegrationHip(scene, **{**KW, **kw})
    hip.upload_raw_frame(scene)
    hip.clearOccupiedBricks()
    hip.processTextures()
    return hip


def layers_of(hip, stream, lab=True):
    p = hip.preprocessed(lab=lab)
    col = hip.raw_frame()[1]
    out = {0: col[stream], 1: p["depth_b"][stream], 2: p["quality"][stream], 3: p["normals"][stream], 4: p["silhouette"][stream], 5: p["depth2"][stream]}
    if lab:
        out[6] = p["lab"][stream]
    return out


def window_and_check(hip, type, stream, layer, rect=RECT, clip=None, min_covered=1):
    fc, fd = hip.framebuffer()
    hip.drawSensorTexture(type, stream, rect, clip)
    gc, gd = hip.framebuffer()
    wc = S.draw(type, layer, rect, clip, fc)
    assert same(gd, fd).all(), "the window wrote depth"
    bad = ~same(gc, wc)
    assert not bad.any(), f"type {type} stream {stream}: {int(bad.sum())} colour values differ"
    covered = S.coverage(rect, clip, hip.view)[0]
    assert covered.sum() >= min_covered
    assert same(gc[~covered], fc[~covered]).all()
    return fc, gc, covered


def test_all_seven_types_of_every_stream_after_process_textures(rr, small_scene):
    hip = raw_processed(rr, small_scene)
    random_framebuffer(hip)
    assert hip.sensorViewSize(40.0) == tuple(float(x) for x in S.view_size(40.0, (small_scene["width"], small_scene["height"])))
    distinct = set()
    for stream in range(small_scene["n"]):
        L = layers_of(hip, stream)
        assert (L[5] > 0).sum() > 100 and (L[4] > 0).sum() > 100 and np.unique(L[6]).size > 100     # a real frame came through (the Lab values are small: inc_color.glsl divides the normalised colour by 255 again)
        for type in range(7):
            _, gc, covered = window_and_check(hip, type, stream, L[type], min_covered=40 * 53)
            distinct.add(gc[covered].tobytes())
    assert len(distinct) >= 14                                            # the types and the streams really show different things


def punch_through_message(rr, scene):
    """a DXT1 message whose first block row of sensor 0 holds hand-built three-colour blocks (c0 = 0x001f <= c1 = 0xf800: index 3 is
    transparent black): blocks 2 .. 11 all transparent, 12 .. 21 the texel pattern c0, transparent, c1, transparent"""
    msg = bytearray(rr.scene.make_wire_message(scene, 1, 0))
    for b in range(2, 22):
        msg[8 * b: 8 * b + 8] = bytes([0x1f, 0x00, 0x00, 0xf8]) + bytes([0xff if b < 12 else 0xdc] * 4)
    return bytes(msg)


@pytest.mark.parametrize("cf", [0, 1, 5])
def test_wire_frames(rr, small_scene, cf):
    hip = rr.ReconIntegrationHip(small_scene, **KW)
    hip.setWireFormat(cf, 0)
    hip.upload_wire_frame(punch_through_message(rr, small_scene) if cf == 1 else rr.scene.make_wire_message(small_scene, cf, 0), small_scene)
    hip.clearOccupiedBricks()
    hip.processTextures()
    random_framebuffer(hip, 11)
    rect = (2.0, 2.0, 62.0, 82.0)
    for stream in (0, 3):
        L = layers_of(hip, stream)
        for type in range(7):
            window_and_check(hip, type, stream, L[type], rect)
    if cf == 1:                                                           # the blend really ran: partly and wholly transparent samples
        col = hip.raw_frame()[1][0]
        assert (col[..., 3] == 0).sum() >= 10 * 16 + 10 * 8 and (col[..., 3] == 255).sum() > 1000
        covered, cx, cy = S.coverage(rect, None, hip.view)
        u, v = S.rotate(*S.frag_uv(rect, cx, cy))
        alpha = S.sample(S.texel_vec4(0, col), u, v, False)[..., 3][covered]
        assert ((alpha > 0) & (alpha < 1)).any() and (alpha == 0).any() and (alpha == 1).any()
        fc, gc, _ = window_and_check(hip, 0, 0, col, rect)
        a0 = covered & (S.sample(S.texel_vec4(0, col), u, v, False)[..., 3] == 0)
        assert same(gc[a0], fc[a0]).all()                                 # a transparent sample leaves the pixel
    elif cf == 0:
        assert (hip.raw_frame()[1][..., 3] == 255).all()


def test_colour_resolution_differs_from_the_depth_resolution(rr):
    sc = rr.scene.make_scene(n_streams=2, width=160, height=120, lut_res=24, inv_res=24, color_width=200, color_height=88)
    hip = raw_processed(rr, sc)
    random_framebuffer(hip, 5)
    for stream in range(2):
        L = layers_of(hip, stream)
        assert L[0].shape == (88, 200, 4) and L[5].shape == (120, 160)
        for type in (0, 1, 6):
            window_and_check(hip, type, stream, L[type])


def test_over_a_drawn_frame_two_windows_side_by_side(rr, small_scene):
    hip = raw_processed(rr, small_scene)
    mv, pr = rr.scene.default_view(*VIEW)
    hip.updateOccupiedBricks(); hip.integrate(); hip.drawF(mv, pr)
    hip.drawBBox(mv, pr)
    assert (hip.framebuffer()[1] < 1).sum() > 100
    w, h = [float(x) for x in S.view_size(36.0, (160, 120))]
    L0, L1 = layers_of(hip, 0), layers_of(hip, 1)
    window_and_check(hip, 3, 0, L0[3], (4.0, 4.0, 4.0 + w, 4.0 + h))
    window_and_check(hip, 0, 1, L1[0], (4.0 + w + 2.0, 4.0, 4.0 + w + 2.0 + w, 4.0 + h))
    window_and_check(hip, 5, 1, L1[5], (20.5, 30.25, 20.5 + w, 30.25 + h))   # ... and one over both


def test_clip_rect_and_quads_that_leave_the_view(rr, small_scene):
    hip = raw_processed(rr, small_scene)
    random_framebuffer(hip, 3)
    L = layers_of(hip, 2)
    _, _, cov = window_and_check(hip, 4, 2, L[4], RECT, (10.0, 8.5, 30.75, 40.25))
    assert cov.sum() == S.scissor_box((10.0, 8.5, 30.75, 40.25), VIEW)[2] * S.scissor_box((10.0, 8.5, 30.75, 40.25), VIEW)[3]
    window_and_check(hip, 6, 2, L[6], RECT, (-50.0, -20.0, 500.0, 300.0))   # a clip rect larger than the view
    window_and_check(hip, 1, 2, L[1], (-13.5, -20.25, 26.5, 33.0))          # over the top left corner
    window_and_check(hip, 2, 2, L[2], (140.0, 60.0, 180.0, 113.5))          # over the bottom right corner
    window_and_check(hip, 0, 2, L[0], (-30.0, -30.0, 400.0, 300.0))         # larger than the view
    fc, _ = hip.framebuffer()
    for rect, clip in (((200.0, 10.0, 240.0, 60.0), None), ((-80.0, 10.0, -40.0, 60.0), None), ((10.0, 100.0, 50.0, 150.0), None),
                       (RECT, (50.0, 60.0, 90.0, 80.0)), (RECT, (30.0, 8.0, 10.0, 40.0))):
        hip.drawSensorTexture(5, 2, rect, clip)                           # wholly outside the view / the clip rect, an inverted clip rect
        assert same(hip.framebuffer()[0], fc).all()


def test_a_colour_mask_mode_is_allowed_and_ignored(rr, small_scene):
    hip = raw_processed(rr, small_scene)
    L = layers_of(hip, 1)
    fc, fd = random_framebuffer(hip, 9)
    _, plain, _ = window_and_check(hip, 0, 1, L[0])
    for mode in (1, 2):
        hip.set_framebuffer(fc, fd)
        hip.setColorMaskMode(mode)
        _, masked, _ = window_and_check(hip, 0, 1, L[0])
        assert same(masked, plain).all()
    hip.setColorMaskMode(0)


def test_a_frame_handed_over_already_processed(rr, small_scene):
    sc = small_scene
    hip = rr.ReconIntegrationHip(sc, **KW)                               # tsdf_upload_frame
    random_framebuffer(hip, 2)
    for stream in (0, 2):
        window_and_check(hip, 0, stream, np.ascontiguousarray(sc["color"], np.uint8)[stream])
        window_and_check(hip, 1, stream, np.asarray(sc["depth"], np.float32)[stream][..., 0])     # (r, 0, 0, 1): the slot keeps depth.r alone
        window_and_check(hip, 2, stream, np.asarray(sc["quality"], np.float32)[stream])
        window_and_check(hip, 4, stream, np.asarray(sc["silhouette"], np.float32)[stream])
    for type in (3, 5, 6):
        with pytest.raises(rr.TsdfError) as e:
            hip.drawSensorTexture(type, 0, RECT)
        assert e.value.code == TSDF_ERR_STATE
    hip.upload_normals(sc["normals"])
    window_and_check(hip, 3, 1, np.asarray(sc["normals"], np.float32)[1])
    for type in (5, 6):
        with pytest.raises(rr.TsdfError) as e:
            hip.drawSensorTexture(type, 0, RECT)
        assert e.value.code == TSDF_ERR_STATE
    # the asynchronous upload into the other slot + select
    hip.upload_frame_async(sc)
    hip.select_frame_slot(1 - hip.current_frame_slot())
    window_and_check(hip, 4, 3, np.asarray(sc["silhouette"], np.float32)[3])
    # a raw frame after it: nothing until it is processed, everything afterwards -- and a processed frame after THAT has no normals of its own
    hip.upload_raw_frame(sc)
    for type in range(7):
        with pytest.raises(rr.TsdfError) as e:
            hip.drawSensorTexture(type, 0, RECT)
        assert e.value.code == TSDF_ERR_STATE
    hip.clearOccupiedBricks(); hip.processTextures()
    L = layers_of(hip, 0)
    for type in range(7):
        window_and_check(hip, type, 0, L[type])
    hip.upload_frame(sc)
    with pytest.raises(rr.TsdfError) as e:
        hip.drawSensorTexture(3, 0, RECT)
    assert e.value.code == TSDF_ERR_STATE
    window_and_check(hip, 2, 0, np.asarray(sc["quality"], np.float32)[0])


def test_errors(rr, small_scene):
    fresh = rr.ReconIntegrationHip(small_scene, upload=False, **KW)
    with pytest.raises(rr.TsdfError) as e:
        fresh.drawSensorTexture(0, 0, RECT)
    assert e.value.code == TSDF_ERR_STATE
    hip = raw_processed(rr, small_scene)
    fc, _ = random_framebuffer(hip, 4)
    nan, inf = float("nan"), float("inf")
    bad = [(7, 0, RECT, None), (0, small_scene["n"], RECT, None), (0, 0, (nan, 2, 40, 50), None), (0, 0, (3, 2, inf, 50), None),
           (0, 0, RECT, (0, 0, nan, 90)), (0, 0, RECT, (-inf, 0, 160, 90)), (0, 0, (40, 2, 40, 50), None), (0, 0, (3, 50, 40, 50), None),
           (0, 0, (41, 2, 40, 50), None), (0, 0, (3, 51, 40, 50), None)]
    for type, stream, rect, clip in bad:
        with pytest.raises(rr.TsdfError) as e:
            hip.drawSensorTexture(type, stream, rect, clip)
        assert e.value.code == TSDF_ERR_INVALID_ARGUMENT, (type, stream, rect, clip)
    assert rr.load_library().tsdf_draw_sensor_texture(hip._c, C.c_uint32(0), C.c_uint32(0), None, None) == TSDF_ERR_INVALID_ARGUMENT
    for setup, undo in ((lambda: hip.setViewportOrigin(8, 0), lambda: hip.setViewportOrigin(0, 0)),
                        (lambda: hip.setViewportOffset(0.5, 0), lambda: hip.setViewportOffset(0, 0))):
        setup()
        with pytest.raises(rr.TsdfError) as e:
            hip.drawSensorTexture(2, 0, RECT)
        assert e.value.code == TSDF_ERR_STATE
        undo()
    assert same(hip.framebuffer()[0], fc).all()                           # none of them drew
    # the Lab image's own rule, as for tsdf_download_preprocessed: its inputs must still be the processed frame's
    hip.drawSensorTexture(6, 0, RECT)
    hip.setPreprocess(processed_depth=False)
    with pytest.raises(rr.TsdfError) as e:
        hip.preprocessed()
    assert e.value.code == TSDF_ERR_STATE
    with pytest.raises(rr.TsdfError) as e:
        hip.drawSensorTexture(6, 0, RECT)
    assert e.value.code == TSDF_ERR_STATE
    hip.drawSensorTexture(5, 0, RECT)


def test_sparse_pool_context(rr, small_scene):
    hip = raw_processed(rr, small_scene, sparse_pool_tiles=4096)
    mv, pr = rr.scene.default_view(*VIEW)
    hip.updateOccupiedBricks(); hip.integrate(); hip.drawF(mv, pr)
    L = layers_of(hip, 3)
    for type in range(7):
        window_and_check(hip, type, 3, L[type])


def test_windows_between_raw_frames_through_the_lanes(rr):
    """stage overlap on: eight moving frames through tsdf_frame_raw_dev with a window after each.  The window must show the frame just processed (it
    is ordered behind the lane that writes the products) and the next frame's passes must not overtake it; with overlap off everything is on
    one stream.  The frames themselves must not notice the windows."""
    import torch
    mk = dict(n_streams=3, width=160, height=120, lut_res=24, inv_res=32)
    scs = [rr.scene.make_scene(**mk), rr.scene.make_scene(**mk, sphere_c=(0.4, 0.7, -0.3), box_c=(-0.5, 1.5, 0.2)), rr.scene.make_scene(**mk, sphere_c=(-0.3, 1.3, 0.2))]
    kw = dict(res=(96, 96, 96), brick_size=[2.0 / 12, 2.2 / 12, 2.0 / 12], limit=0.04, view=VIEW)
    pr = rr.scene.gl_flat(rr.scene.perspective(50.0, 16.0 / 9.0, 0.1, 200.0))
    mvs = [rr.scene.gl_flat(rr.scene.look_at(e, (0.0, 1.1, 0.0))) for e in [(0.0, 1.1, 3.0), (1.6, 1.4, 2.4), (-2.2, 0.6, 1.2)]]
    dev = [(torch.from_numpy(np.ascontiguousarray(sc["depth_raw"], np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(sc["color"], np.uint8)).cuda()) for sc in scs]
    torch.cuda.synchronize()
    order = [0, 1, 2, 1, 0, 2, 2, 1]
    types = [5, 6, 1, 3, 0, 2, 4, 6]
    rects = [RECT, (60.5, 10.0, 100.5, 63.375)]

    def run(overlap, windows, read_every_frame):
        o = rr.ReconIntegrationHip(scs[0], **kw)
        o.set_stage_overlap(overlap)
        o.set_preprocess_calibration(scs[0])
        before, after = [], []
        for n, k in enumerate(order):
            o.frame_raw_dev(mvs[n % 3], pr, new_frame=(dev[k][0].data_ptr(), dev[k][1].data_ptr()), complete=True)
            last = n == len(order) - 1
            if read_every_frame or last:
                before.append(o.framebuffer())
            if windows:
                o.drawSensorTexture(types[n], n % 3, rects[0])
                o.drawSensorTexture(types[(n + 3) % 8], (n + 1) % 3, rects[1])
                if read_every_frame or last:
                    after.append(o.framebuffer())
        return o, before, after

    serial, s_before, s_after = run(False, True, True)
    lanes, l_before, l_after = run(True, True, True)
    queued, q_before, q_after = run(True, True, False)                    # nothing is read until the last frame
    bare, b_before, _ = run(True, False, True)
    for n in range(len(order)):
        assert_same(l_before[n][0], s_before[n][0], f"frame {n}: framebuffer before the windows, lanes vs one stream")
        assert_same(l_before[n][0], b_before[n][0], f"frame {n}: framebuffer before the windows, with vs without windows")
        assert_same(l_before[n][1], b_before[n][1], f"frame {n}: depth before the windows, with vs without windows")
        assert_same(l_after[n][0], s_after[n][0], f"frame {n}: the windows, lanes vs one stream")
        assert_same(l_after[n][1], l_before[n][1], f"frame {n}: the windows wrote depth")
        assert not same(l_after[n][0], l_before[n][0]).all()
    assert_same(q_before[0][0], s_before[-1][0], "last frame of the queued run: framebuffer before the windows")
    assert_same(q_after[0][0], s_after[-1][0], "last frame of the queued run: the windows")
    # the serial run's last windows against the reference, from the products it holds
    p, col = serial.preprocessed(), serial.raw_frame()[1]
    n = len(order) - 1
    src = {4: p["silhouette"], 6: p["lab"]}
    want = S.draw(types[n], src[types[n]][n % 3], rects[0], None, s_before[-1][0])
    want = S.draw(types[(n + 3) % 8], p["depth_b"][(n + 1) % 3], rects[1], None, want)
    assert types[n] == 6 and types[(n + 3) % 8] == 1
    assert_same(s_after[-1][0], want, "the last frame's windows against the reference")
    for o in (lanes, queued, bare):
        assert_same(o.tsdf(), serial.tsdf(), "volume")
        a, b = o.preprocessed(), p
        for key in a:
            assert_same(a[key], b[key], key)
        np.testing.assert_array_equal(o.bricks()[0], serial.bricks()[0])
    assert col.shape[0] == 3


def test_frame_harness_draws_a_window_per_sensor(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host, lib = os.path.join(root, "rgbd-recon_amd", "host"), os.path.join(root, "rgbd-recon_amd")
    exe = str(tmp_path / "frame_harness")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(host, "frame_harness.cpp"), "-o", exe,
                           "-L" + lib, "-lrgbd_recon_hip", "-Wl,-rpath," + lib])
    for type in (0, 2):
        r = subprocess.run([exe, "--sensor-view", str(type), "6"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert 0 < int(r.stdout.split(" pixels changed")[0].split()[-1]) <= 36      # the quad covers 6 x 6 pixels
    r = subprocess.run([exe, "--sensor-view", "5", "6"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "SensorTextureViewHip" in r.stderr      # no morphed raw depth for a frame handed over already processed
