"""GPU: the frame read-out (tsdf_present and its ring) against tests/present_reference.py, byte for byte: planted framebuffers at the sizes where
the kernels' index arithmetic can go wrong, a rendered frame, the ring's bookkeeping, and eight moving frames through the lanes with the presented
frames picked up two frames late."""
import time

import numpy as np
import pytest

import present_reference as P

pytestmark = pytest.mark.gpu

FORMATS = [(P.RGBA8, "rgba8"), (P.DXT1, "dxt1")]
KW = dict(res=(64, 64, 64), brick_size=[2.0 / 8, 2.2 / 8, 2.0 / 8], limit=0.04)


def planted(w, h, seed):
    """random values in [-0.5, 1.5] with NaN / +-inf / -0.0 and exact half-way products sprinkled in; depth is of no interest"""
    rng = np.random.default_rng(seed)
    fb = rng.uniform(-0.5, 1.5, (h, w, 4)).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.5, 0.1, 0.7, 1.0, 0.0, -1.0], np.float32)
    hit = rng.random((h, w, 4)) < 0.15
    fb[hit] = special[rng.integers(0, special.size, int(hit.sum()))]
    return fb, np.full((h, w), 1.0, np.float32)


def expect(fb, fmt, flags):
    want = P.present(fb, fmt, flags)
    return want.reshape(fb.shape) if fmt == P.RGBA8 else want


def take(hip, wait=True):
    got = hip.present_acquire(wait)
    assert got is not None
    hip.present_release()
    return got


@pytest.fixture(scope="module")
def scene(rr):
    return rr.scene.make_scene(n_streams=2, width=160, height=120, lut_res=32, inv_res=32)


@pytest.fixture(scope="module")
def ctx(rr, scene):
    hip = rr.ReconIntegrationHip(scene, view=(64, 36), **KW)
    yield hip
    hip.close()


# 4 x 4: a single block; 20 x 12: whole blocks, a strip that is not full; 22 x 9: partial blocks on both axes; 132 x 8: 33 blocks across = 8 full
# strips and one with a single block, rows that no wave of the RGBA8 kernel starts on
@pytest.mark.parametrize("w,h", [(4, 4), (20, 12), (22, 9), (132, 8)])
def test_planted_framebuffers_equal_the_reference(ctx, w, h):
    ctx.resize(w, h)
    fb, depth = planted(w, h, seed=w * 100 + h)
    ctx.set_framebuffer(fb, depth)
    for fmt, name in FORMATS:
        for flags in (0, P.TOP_DOWN):
            ctx.present_config(fmt, flags, 3)
            assert ctx.present_size() == P.size_bytes(w, h, fmt)
            ctx.present(tag=7)
            got, tag, size = take(ctx)
            assert tag == 7 and size == (w, h)
            np.testing.assert_array_equal(got, expect(fb, fmt, flags), f"{name} flags {flags} at {w} x {h}")
    back, _ = ctx.framebuffer()
    np.testing.assert_array_equal(back.view(np.uint32), fb.view(np.uint32))       # presenting only reads the framebuffer


def test_rendered_frame_equals_the_reference(rr, ctx):
    """one frame of the two-stream scene, colour filling on, lanes on: the present joins the hole filling in flight on its own lane"""
    ctx.resize(64, 36)
    mv, pr = rr.scene.default_view(64, 36)
    for fmt, name in FORMATS:
        for flags in (0, P.TOP_DOWN):
            ctx.present_config(fmt, flags, 2)
            ctx.frame_dev(mv, pr)
            ctx.present(tag=1)                                                   # (no synchronisation in between)
            got, _, size = take(ctx)
            fb, fd = ctx.framebuffer()
            assert size == (64, 36) and (fd < 1).sum() > 50                        # a picture, not a blank frame
            np.testing.assert_array_equal(got, expect(fb, fmt, flags), f"{name} flags {flags}")


def test_ring_of_three_slots(rr, ctx):
    w, h = 132, 8
    ctx.resize(w, h)
    ctx.present_config(P.RGBA8, 0, 3)
    with pytest.raises(rr.TsdfError) as e:
        ctx.present_acquire()                                                     # nothing queued
    assert e.value.code == -4
    with pytest.raises(rr.TsdfError) as e:
        ctx.present_release()                                                     # nothing held
    assert e.value.code == -4
    fbs = [planted(w, h, seed=40 + k) for k in range(5)]
    for k in range(3):
        ctx.set_framebuffer(*fbs[k])
        ctx.present(tag=10 + k)
    with pytest.raises(rr.TsdfError) as e:
        ctx.present(tag=99)                                                       # the fourth: every slot is queued
    assert e.value.code == -4
    for call in (lambda: ctx.resize(64, 36), lambda: ctx.present_config(P.DXT1, 0, 3)):
        with pytest.raises(rr.TsdfError) as e:
            call()
        assert e.value.code == -4
    got, tag, _ = take(ctx)
    assert tag == 10
    np.testing.assert_array_equal(got, expect(fbs[0][0], P.RGBA8, 0))
    # one slot is free again: present a fourth frame, then poll without waiting -- a frame is handed out whole or not at all
    ctx.set_framebuffer(*fbs[3])
    ctx.present(tag=13)
    for k in (1, 2, 3):
        deadline = time.monotonic() + 20.0
        got = ctx.present_acquire(wait=False)
        while got is None and time.monotonic() < deadline:
            got = ctx.present_acquire(wait=False)
        assert got is not None, "the copy never finished"
        with pytest.raises(rr.TsdfError):
            ctx.present_acquire()                                                 # one frame is held at a time
        np.testing.assert_array_equal(got[0], expect(fbs[k][0], P.RGBA8, 0), f"frame {k}")
        assert got[1] == 10 + k
        if k == 2:                                                               # held frames block a resize as queued ones do
            with pytest.raises(rr.TsdfError):
                ctx.resize(64, 36)
        ctx.present_release()
    with pytest.raises(rr.TsdfError):
        ctx.present_acquire(wait=False)                                           # drained
    ctx.resize(20, 12)                                                            # works again, and the ring follows the new size
    ctx.set_framebuffer(*planted(20, 12, seed=3))
    ctx.present(tag=5)
    got, tag, size = take(ctx)
    assert tag == 5 and size == (20, 12) and got.shape == (12, 20, 4)
    # the smallest ring and the largest: 2 * slots + 1 frames, at most `slots` of them in flight, so the head goes round the ring twice
    ctx.resize(w, h)
    for slots in (2, 8):
        ctx.present_config(P.RGBA8, 0, slots)
        n, queued, taken = 2 * slots + 1, 0, 0

        def put():
            nonlocal queued
            ctx.set_framebuffer(*fbs[queued % 5])
            ctx.present(tag=100 * slots + queued)
            queued += 1

        def get():
            nonlocal taken
            got, tag, _ = take(ctx)
            assert tag == 100 * slots + taken, (slots, taken)
            np.testing.assert_array_equal(got, expect(fbs[taken % 5][0], P.RGBA8, 0), f"{slots} slots, frame {taken}")
            taken += 1

        for _ in range(slots):
            put()
        with pytest.raises(rr.TsdfError) as e:
            ctx.present(tag=99)                                                   # every slot is queued
        assert e.value.code == -4
        while queued < n:
            get()
            put()
        while taken < n:
            get()
        with pytest.raises(rr.TsdfError):
            ctx.present_acquire(wait=False)                                       # drained


_plain_runs = {}


def moving_frames(rr):
    import torch
    mk = dict(n_streams=2, width=160, height=120, lut_res=32, inv_res=32)
    scs = [rr.scene.make_scene(**mk), rr.scene.make_scene(**mk, sphere_c=(0.4, 0.7, -0.3), box_c=(-0.5, 1.5, 0.2)), rr.scene.make_scene(**mk, sphere_c=(-0.3, 1.3, 0.2))]
    raw = [[torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ("depth", "quality", "silhouette", "color")] for sc in scs]
    torch.cuda.synchronize()
    pr = rr.scene.gl_flat(rr.scene.perspective(50.0, 16.0 / 9.0, 0.1, 200.0))
    mvs = [rr.scene.gl_flat(rr.scene.look_at(e, (0.0, 1.1, 0.0))) for e in [(0.0, 1.1, 3.0), (1.6, 1.4, 2.4), (-2.2, 0.6, 1.2)]]
    return scs, raw, mvs, pr


def plain_run(rr, lane_flags, frames):
    """the framebuffer of every frame from a context that never presents (one run per lane setting, shared by the formats)"""
    if lane_flags not in _plain_runs:
        scs, raw, mvs, pr = moving_frames(rr)
        hip = rr.ReconIntegrationHip(scs[0], view=(64, 36), lane_flags=lane_flags, **KW)
        out = []
        for f in range(frames):
            hip.frame_dev(mvs[f % 3], pr, [t.data_ptr() for t in raw[f % 3]])
            out.append(hip.framebuffer()[0])
        hip.close()
        _plain_runs[lane_flags] = out
    return _plain_runs[lane_flags]


@pytest.mark.parametrize("fmt,name", FORMATS)
@pytest.mark.parametrize("one_stream", [False, True])
def test_frames_through_the_lanes_picked_up_two_late(rr, one_stream, fmt, name):
    frames, lag = 8, 2
    lane_flags = rr.LANES_ONE_STREAM if one_stream else 0
    want = plain_run(rr, lane_flags, frames)
    assert any((want[f] != want[f + 1]).any() for f in range(frames - 1))         # the frames do move
    scs, raw, mvs, pr = moving_frames(rr)
    hip = rr.ReconIntegrationHip(scs[0], view=(64, 36), lane_flags=lane_flags, **KW)
    hip.present_config(fmt, P.TOP_DOWN, 3)
    seen = []

    def pick(f):
        got, tag, size = take(hip)
        assert tag == 1000 + f and size == (64, 36)
        np.testing.assert_array_equal(got, expect(want[f], fmt, P.TOP_DOWN), f"{name}, frame {f}")
        seen.append(f)

    for f in range(frames):
        hip.frame_dev(mvs[f % 3], pr, [t.data_ptr() for t in raw[f % 3]])
        hip.present(tag=1000 + f)
        if f >= lag:
            pick(f - lag)
        if f in (3, frames - 1):                                                 # presenting changes nothing: the same framebuffer, bit for bit
            np.testing.assert_array_equal(hip.framebuffer()[0].view(np.uint32), want[f].view(np.uint32), f"framebuffer, frame {f}")
    for f in range(frames - lag, frames):
        pick(f)
    assert seen == list(range(frames))
    hip.close()
