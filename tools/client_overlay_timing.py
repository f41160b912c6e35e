"""Timing of the client's last two mono draws, drawBBox (the bounding-box wireframe) and drawTextures (the texture view of unit 15, the
hole-filling atlas, and unit 16, the depth-limit image), after one frame (integrate + drawF) at the bench scene's c2 (512^3 culled, hole
filling and space skipping on) and c1 (256^3 dense; the frame is drawn once with both on so that both textures exist, then without).
Device time per draw from the library's HIP-event timers ("bbox", "textures").  Prints one JSON line per shape; with an argument, also
writes the list of them to that file."""
import sys, os, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch  # noqa: F401  (torch first: the library binds to the HIP runtime torch loaded)
import rgbd_recon_amd as rr
VIEW = (1280, 720)
N = 50


def event_ms(hip, name, fn, n=N):
    for _ in range(5): fn()
    hip.sync()
    hip.timer_stats(name)                                                # (resets the timer's samples)
    for _ in range(n): fn()
    hip.sync()
    cnt, total = hip.timer_stats(name)
    return total / cnt


out = []
for shape in ("c2", "c1"):
    scene = rr.scene.make_scene(n_streams=4, width=640, height=480, lut_res=128, inv_res=128)
    ext = scene["bbox_max"] - scene["bbox_min"]
    res = (512,) * 3 if shape == "c2" else (256,) * 3
    hip = rr.ReconIntegrationHip(scene, res=res, brick_size=[float(ext[a]) / res[a] * 8 for a in range(3)], limit=0.01, view=VIEW)
    mv, pr = rr.scene.default_view(*VIEW)
    hip.clearOccupiedBricks(); hip.markBricks(); hip.updateOccupiedBricks(); hip.integrate(); hip.drawF(mv, pr)
    if shape == "c1":
        hip.setUseBricks(False); hip.setSpaceSkip(False); hip.setColorFilling(False)
        hip.integrate(); hip.drawF(mv, pr)
    hip.sync()
    hip.enable_timers(True)
    hip.set_timer_filter(["bbox", "textures"])
    rec = dict(shape=shape, res=list(hip.res), view=f"{VIEW[0]}x{VIEW[1]}")
    rec["bbox_ms"] = event_ms(hip, "bbox", lambda: hip.drawBBox(mv, pr))
    rec["textures_unit15_ms"] = event_ms(hip, "textures", lambda: hip.drawTextures(0))
    rec["textures_unit16_ms"] = event_ms(hip, "textures", lambda: hip.drawTextures(1))
    print(json.dumps(rec), flush=True)
    out.append(rec)
    hip.close()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
