"""What seeing the frames costs: frames/s of the tsdf_frame_dev loop at bench.py's c2 (512^3, 4 streams, 1280 x 720, a new frame from device memory
every step) in four variants that alternate in one process --
  none      no read-out (what bench.py measures)
  download  tsdf_download_framebuffer every frame: synchronous, fp32 colour + depth, 20 B per pixel (the only read-out before tsdf_present)
  rgba8     tsdf_present every frame into the RGBA8 ring (3 slots), each frame acquired and released two frames late
  dxt1      the same with the DXT1 ring
-- and the device time of the conversion kernel (timer "present") per format.  Prints one JSON line; with an argument, also writes it to that file.
Kernel times of a profiler belong to a run of their own (rocprofv3 --kernel-trace --stats -- python tools/present_timing.py)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch  # noqa: F401  (torch first: the library binds to the HIP runtime torch loaded)
import rgbd_recon_amd as rr
import bench

FRAMES = int(os.environ.get("PRESENT_TIMING_FRAMES", "300"))
ROUNDS = int(os.environ.get("PRESENT_TIMING_ROUNDS", "3"))
LAG = 2
cfg = bench.CONFIGS["c2"]
mk = dict(n_streams=cfg["streams"], width=640, height=480, lut_res=bench.LUT, inv_res=bench.LUT)
scs = [rr.scene.make_scene(**mk), rr.scene.make_scene(**mk, **bench.MOVED)]
ext = scs[0]["bbox_max"] - scs[0]["bbox_min"]
hip = rr.ReconIntegrationHip(scs[0], res=cfg["res"], brick_size=[float(ext[k]) / cfg["res"][k] * 8 for k in range(3)], limit=bench.LIMIT, view=bench.VIEW)
hip.setUseBricks(cfg["use_bricks"]); hip.setSpaceSkip(cfg["skip_space"]); hip.setColorFilling(cfg["fill_holes"])
mv, pr = rr.scene.default_view(*bench.VIEW)
raw = [[torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ("depth", "quality", "silhouette", "color")] for sc in scs]
ptr = [[t.data_ptr() for t in r] for r in raw]
torch.cuda.synchronize()
L, c = hip._L, hip._c
w, h = bench.VIEW
fb_c, fb_d = np.empty((h, w, 4), np.float32), np.empty((h, w), np.float32)
import ctypes as C
p_c, p_d = fb_c.ctypes.data_as(C.POINTER(C.c_float)), fb_d.ctypes.data_as(C.POINTER(C.c_float))
data, nbytes, tag, size = C.c_void_p(), C.c_uint64(), C.c_uint64(), (C.c_uint32 * 2)()
checksum = 0


def pick():
    """acquire (waiting) + release without copying: the consumer reads the pinned buffer in place; one byte is read so that the frame is touched"""
    global checksum
    rc = L.tsdf_present_acquire(c, 1, C.byref(data), C.byref(nbytes), C.byref(tag), size)
    assert rc == 0 and data.value
    checksum += C.cast(data, C.POINTER(C.c_uint8))[nbytes.value - 1]
    assert L.tsdf_present_release(c) == 0


def loop(variant, n):
    if variant in ("rgba8", "dxt1"):
        hip.present_config(rr.PRESENT_DXT1 if variant == "dxt1" else rr.PRESENT_RGBA8, rr.PRESENT_TOP_DOWN, 3)
    hip.sync()
    t0 = time.perf_counter()
    for i in range(n):
        hip.frame_dev(mv, pr, ptr[i & 1])
        if variant == "download":
            assert L.tsdf_download_framebuffer(c, p_c, p_d) == 0
        elif variant != "none":
            hip.present(i)
            if i >= LAG:
                pick()
    if variant in ("rgba8", "dxt1"):
        for _ in range(min(LAG, n)):
            pick()
    hip.sync()
    return n / (time.perf_counter() - t0)


variants = ("none", "download", "rgba8", "dxt1")
for v in variants:
    loop(v, 30)                                                            # warm-up: allocations, the second volume set, the ring
rec = dict(shape="c2", view=f"{w}x{h}", frames=FRAMES, rounds=ROUNDS, lag=LAG)
fps = {v: [] for v in variants}
for _ in range(ROUNDS):
    for v in variants:
        fps[v].append(loop(v, FRAMES))
for v in variants:
    rec[f"fps_{v}"] = [round(x, 1) for x in fps[v]]
    rec[f"fps_{v}_median"] = round(float(np.median(fps[v])), 1)
# device time of the conversion kernel alone (timers on: the calling thread issues the fill lane's calls, so the rates above are taken first)
hip.enable_timers(True)
hip.set_timer_filter(["present"])
for v in ("rgba8", "dxt1"):
    loop(v, 10)
    hip.timer_stats("present")
    loop(v, 100)
    cnt, total = hip.timer_stats("present")
    rec[f"present_{v}_ms"] = round(total / cnt, 5)
    rec[f"bytes_{v}"] = hip.present_size()
hip.enable_timers(False)
rec["bytes_download"] = w * h * 20
rec["checksum"] = int(checksum)
print(json.dumps(rec), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(rec, f, indent=1)
hip.close()
