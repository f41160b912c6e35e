"""Timing of the MVT back-end (drawMVT) beside Trigrid (drawTrigrid) in one process, device-synchronised wall time per draw:
4 x 640x480 into 1280x720 (the bench's frame size) and 5 x 512x424 (the reference's five Kinect V2 sensors).  Prints one JSON line per
shape; with an argument, also writes the list of them to that file."""
import sys, os, time, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch  # noqa: F401  (torch first: the library binds to the HIP runtime torch loaded)
import rgbd_recon_amd as rr
VIEW = (1280, 720)


def timed(fn, n):
    for _ in range(5): fn()
    hip.sync(); t0 = time.perf_counter()
    for _ in range(n): fn()
    hip.sync()
    return (time.perf_counter() - t0) / n * 1e3


out = []
for n_streams, w, h in ((4, 640, 480), (5, 512, 424)):
    scene = rr.scene.make_scene(n_streams=n_streams, width=w, height=h, lut_res=128, inv_res=128)
    hip = rr.ReconIntegrationHip(scene, res=(64, 64, 64), brick_size=0.25, limit=0.04, view=VIEW)
    hip.upload_raw_frame(scene)
    mv, pr = rr.scene.default_view(*VIEW)
    r = dict(shape=f"{n_streams}x{w}x{h}", view=f"{VIEW[0]}x{VIEW[1]}", vertices=n_streams * (w + 1) * (h + 1))
    r["mvt_ms"] = timed(lambda: hip.drawMVT(mv, pr), 200)
    r["mvt_covered"] = int((hip.framebuffer()[1] < 1).sum())
    r["mvt_valid_vertices"] = int((hip.mvt_vertices()[..., 0] > 0).sum())
    r["trigrid_ms"] = timed(lambda: hip.drawTrigrid(mv, pr), 200)
    r["trigrid_covered"] = int((hip.framebuffer()[1] < 1).sum())
    print(json.dumps(r), flush=True)
    out.append(r)
    hip.close()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
