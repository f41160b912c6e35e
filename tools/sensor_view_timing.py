"""Timing of the GUI's "Show textures" windows (drawSensorTexture): each of the seven types as a 480-wide window (480 x 640 destination pixels) of a
640 x 480 x 4-stream raw frame into a 1280 x 720 view, beside drawTextures -- the bilinear blit of comparable pixel count that is already in
the tree -- in the same process as the yardstick.  Device time per draw from the library's HIP-event timers ("sensortex", "textures"), and
per destination pixel.  Type 6 also runs the on-demand Lab pass in front of its timer; it is reported with the wall time of the whole call
queue.  Prints one JSON line; with an argument, also writes it to that file."""
import sys, os, json, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch  # noqa: F401  (torch first: the library binds to the HIP runtime torch loaded)
import rgbd_recon_amd as rr
VIEW = (1280, 720)
N = 200
NAMES = ["color", "depth", "quality", "normals", "silhouette", "orig_depth", "lab"]


def event_ms(hip, name, fn, n=N):
    for _ in range(10): fn()
    hip.sync()
    hip.timer_stats(name)                                                # (resets the timer's samples)
    for _ in range(n): fn()
    hip.sync()
    cnt, total = hip.timer_stats(name)
    return total / cnt


scene = rr.scene.make_scene(n_streams=4, width=640, height=480, lut_res=128, inv_res=128)
ext = scene["bbox_max"] - scene["bbox_min"]
res = (512,) * 3
hip = rr.ReconIntegrationHip(scene, res=res, brick_size=[float(ext[a]) / res[a] * 8 for a in range(3)], limit=0.01, view=VIEW)
mv, pr = rr.scene.default_view(*VIEW)
hip.upload_raw_frame(scene)
hip.clearOccupiedBricks(); hip.processTextures(); hip.updateOccupiedBricks(); hip.integrate(); hip.drawF(mv, pr)
hip.sync()
hip.enable_timers(True)
hip.set_timer_filter(["sensortex", "textures"])
w, h = hip.sensorViewSize(480.0)
rect = (20.0, 20.0, 20.0 + w, 20.0 + h)
px = 480 * 640
rec = dict(view=f"{VIEW[0]}x{VIEW[1]}", window=f"{w:g}x{h:g}", window_pixels=px, repeats=N)
vw, vh = int(np.float32(int(np.float32(1.5) * np.float32(VIEW[0]))) / np.float32(2)), VIEW[1] // 2
rec["textures_unit15_ms"] = event_ms(hip, "textures", lambda: hip.drawTextures(0))
rec["textures_pixels"] = vw * vh
rec["textures_ns_per_pixel"] = rec["textures_unit15_ms"] * 1e6 / (vw * vh)
for t, name in enumerate(NAMES):
    ms = [event_ms(hip, "sensortex", lambda: hip.drawSensorTexture(t, s, rect)) for s in range(4)]
    rec[name + "_ms"] = float(np.median(ms))
    rec[name + "_ms_per_stream"] = ms
    rec[name + "_ns_per_pixel"] = float(np.median(ms)) * 1e6 / px
hip.enable_timers(False)
hip.sync()
t0 = time.perf_counter()
for _ in range(N): hip.drawSensorTexture(6, 0, rect)
hip.sync()
rec["lab_whole_call_wall_ms"] = (time.perf_counter() - t0) * 1e3 / N
print(json.dumps(rec), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(rec, f, indent=1)
