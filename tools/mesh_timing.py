"""Timing of the mesh extraction (tsdf_mesh_extract) beside the read-out it replaces, tsdf_download_volume, after one frame at the bench scene's
c2 (512^3 culled, 4 streams).  Device time per stage from the library's HIP-event timers: "mesh_count" (one launch), "mesh_scan" (three), "mesh_emit"
(vertices + triangles), each for the position-only extract and for the one with normals and colours; the volume download is bracketed by a timer of
this tool's own on the context's stream (tile-major -> linear launch + the 512 MiB copy to pageable host memory).  A record, not a threshold.  Prints
one JSON line; with an argument, also writes it to that file."""
import sys, os, json, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch  # noqa: F401  (torch first: the library binds to the HIP runtime torch loaded)
import rgbd_recon_amd as rr
VIEW = (1280, 720)
N = 10
STAGES = ("mesh_count", "mesh_scan", "mesh_emit")

scene = rr.scene.make_scene(n_streams=4, width=640, height=480, lut_res=128, inv_res=128)
ext = scene["bbox_max"] - scene["bbox_min"]
res = (512,) * 3
hip = rr.ReconIntegrationHip(scene, res=res, brick_size=[float(ext[a]) / res[a] * 8 for a in range(3)], limit=0.01, view=VIEW)
mv, pr = rr.scene.default_view(*VIEW)
hip.clearOccupiedBricks(); hip.markBricks(); hip.updateOccupiedBricks(); hip.integrate(); hip.drawF(mv, pr)
hip.sync()
hip.enable_timers(True)
hip.set_timer_filter(list(STAGES) + ["volume_download"])
rec = dict(shape="c2", res=list(hip.res), streams=4)
for label, kw in (("positions", dict(normals=False, colours=False)), ("all_attributes", dict(normals=True, colours=True))):
    for _ in range(2):
        mesh = hip.extract_mesh(**kw)
    for s in STAGES:
        hip.timer_stats(s)                                               # (resets the timer's samples)
    t0 = time.perf_counter()
    for _ in range(N):
        hip.extract_mesh(**kw)
    wall = (time.perf_counter() - t0) / N * 1e3
    r = {s + "_ms": (lambda ct: ct[1] / ct[0])(hip.timer_stats(s)) for s in STAGES}
    r["device_ms"] = sum(r.values())
    r["call_and_download_wall_ms"] = wall                                # extract + tsdf_mesh_download into numpy arrays
    rec[label] = r
st = hip.mesh_stats()
rec.update(vertices=len(mesh["position"]), triangles=len(mesh["triangles"]), mesh_bytes=st["bytes"], tiles=st["tiles"], tiles_skipped=st["tiles_skipped"],
           tiles_with_surface=st["tiles_with_surface"])
hip.tsdf()
hip.timer_stats("volume_download")
t0 = time.perf_counter()
for _ in range(3):
    hip.timer_begin("volume_download"); vol = hip.tsdf(); hip.timer_end("volume_download")
rec["volume_download_wall_ms"] = (time.perf_counter() - t0) / 3 * 1e3
cnt, total = hip.timer_stats("volume_download")
rec["volume_download_ms"] = total / cnt
rec["volume_bytes"] = int(vol.nbytes)
print(json.dumps(rec), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(rec, f, indent=1)
hip.close()
