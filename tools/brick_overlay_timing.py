"""Timing of the occupied-brick wireframes (drawOccupiedBricks, timer "brickwire") beside the bounding box (timer "bbox") of the same run,
after one frame (integrate + drawF) at the bench scene's c2 (512^3, 8-voxel bricks) and at the reference's operating point (200 x 221 x
200, 10-voxel bricks, 5 streams; tests/refpoint_scene.py with a small inverse LUT: the brick list does not depend on it), both at
1280 x 720 under the benchmark's view.  The balanced kernel and the plain one-wave-per-segment form (RR_BRICKWIRE_PLAIN, read at every
draw) alternate in one process.  Device time per draw from the library's HIP-event timers.  Prints one JSON line per shape; with an
argument, also writes the list of them to that file."""
import sys, os, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch  # noqa: F401  (torch first: the library binds to the HIP runtime torch loaded)
import rgbd_recon_amd as rr
import refpoint_scene as rp
VIEW = (1280, 720)
N = 50


def event_ms(hip, name, fn, n=N, prep=lambda: None):
    for _ in range(5): prep(); fn()
    hip.sync()
    hip.timer_stats(name)                                                # (resets the timer's samples)
    for _ in range(n): prep(); fn()
    hip.sync()
    cnt, total = hip.timer_stats(name)
    return total / cnt


def plain(on):
    if on: os.environ["RR_BRICKWIRE_PLAIN"] = "1"
    else: os.environ.pop("RR_BRICKWIRE_PLAIN", None)


out = []
for shape in ("c2", "refpoint"):
    if shape == "c2":
        scene = rr.scene.make_scene(n_streams=4, width=640, height=480, lut_res=128, inv_res=128)
        ext = scene["bbox_max"] - scene["bbox_min"]
        hip = rr.ReconIntegrationHip(scene, res=(512,) * 3, brick_size=[float(ext[a]) / 512 * 8 for a in range(3)], limit=0.01, view=VIEW)
    else:
        scene = rp.make_frames(rr, n_frames=1, inv_res=(64, 64, 64))[0]
        hip = rr.ReconIntegrationHip(scene, **rp.KW)
    mv, pr = rr.scene.default_view(*VIEW)
    hip.clearOccupiedBricks(); hip.markBricks(); hip.updateOccupiedBricks(); hip.integrate(); hip.drawF(mv, pr)
    hip.sync()
    fb = hip.framebuffer()
    hip.enable_timers(True)
    hip.set_timer_filter(["bbox", "brickwire"])
    rec = dict(shape=shape, res=list(hip.res), bricks=list(hip.res_bricks), occupied=int(hip.bricks()[1].sum()), view=f"{VIEW[0]}x{VIEW[1]}")

    def wire():
        hip.drawOccupiedBricks(mv, pr)
    for k in range(2):                                                   # two rounds, alternating: order effects would show
        for name, on in (("balanced", False), ("plain", True)):
            plain(on)
            # every sample draws over the frame as drawF left it: over its own wireframes every fragment would fail the depth test
            rec[f"brickwire_{name}_ms_{k}"] = event_ms(hip, "brickwire", wire, n=20, prep=lambda: hip.set_framebuffer(*fb))
    plain(False)
    # the two forms draw the same picture
    hip.set_framebuffer(*fb); wire(); a = hip.framebuffer()
    plain(True); hip.set_framebuffer(*fb); wire(); b = hip.framebuffer(); plain(False)
    rec["forms_identical"] = bool((a[0] == b[0]).all() and (a[1] == b[1]).all())
    rec["wire_pixels"] = int((a[1] != fb[1]).sum())
    hip.set_framebuffer(*fb)
    rec["bbox_ms"] = event_ms(hip, "bbox", lambda: hip.drawBBox(mv, pr))
    print(json.dumps(rec), flush=True)
    out.append(rec)
    hip.close()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
