"""Timing of the client's overlays, drawCalibVis ("Draw TSDF") and drawFrustums ("Draw frustums"), after one frame (integrate + drawF) at
three shapes: the bench scene c2 (512^3 culled, 128^3 inverse LUT grid), c1 (256^3 dense) and the reference client's default operating point
(voxel 0.01 m -> 200 x 220 x 200, 5 streams, stream 0's inverse LUT from tsdf_invert_calibration at 0.007 m -> 286 x 315 x 286 points).
Device time per draw from the library's HIP-event timers ("calibvis", "frustums"), plus the fraction of grid points the empty-space test
removed.  Prints one JSON line per shape; with an argument, also writes the list of them to that file."""
import sys, os, json
import ctypes as C
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
for shape in ("c2", "c1", "ref"):
    n_streams = 5 if shape == "ref" else 4
    scene = rr.scene.make_scene(n_streams=n_streams, width=640, height=480, lut_res=128, inv_res=128)
    ext = scene["bbox_max"] - scene["bbox_min"]
    if shape == "ref":
        hip = rr.ReconIntegrationHip(scene, voxel_size=0.01, brick_size=0.1, limit=0.01, view=VIEW)
        res_inv = rr.inverse_volume_resolution(scene["bbox_min"], scene["bbox_max"], 0.007)
        r = scene["lut_res"]
        xyz = np.asarray(scene["cv_xyz"][0], np.float32).reshape(int(r[2]), int(r[1]), int(r[0]), 3)
        inv, _ = rr.invert_calibration(xyz, scene["bbox_min"], scene["bbox_max"], res_inv)
        rl = (C.c_uint32 * 3)(*[int(x) for x in r])
        hip._ck(hip._L.tsdf_set_calibration(hip._c, 0, rr.binding._fp(inv), (C.c_uint32 * 3)(*[int(x) for x in res_inv]),
                                            rr.binding._fp(np.ascontiguousarray(scene["cv_uv"][0], np.float32)), rl, rr.binding._fp(xyz), rl))
        del inv
    else:
        res = (512,) * 3 if shape == "c2" else (256,) * 3
        hip = rr.ReconIntegrationHip(scene, res=res, brick_size=[float(ext[a]) / res[a] * 8 for a in range(3)], limit=0.01, view=VIEW)
        if shape == "c1":
            hip.setUseBricks(False); hip.setSpaceSkip(False); hip.setColorFilling(False)
    mv, pr = rr.scene.default_view(*VIEW)
    hip.clearOccupiedBricks(); hip.markBricks(); hip.updateOccupiedBricks(); hip.integrate(); hip.drawF(mv, pr)
    hip.sync()
    hip.enable_timers(True)
    hip.set_timer_filter(["calibvis", "frustums"])
    rec = dict(shape=shape, res=list(hip.res), streams=n_streams, view=f"{VIEW[0]}x{VIEW[1]}")
    rec["calibvis_ms"] = event_ms(hip, "calibvis", lambda: hip.drawCalibVis(mv, pr))
    points, skipped = hip.calibvis_stats()
    rec.update(grid_points=points, skipped_points=skipped, skipped_fraction=skipped / points)
    rec["frustums_ms"] = event_ms(hip, "frustums", lambda: hip.drawFrustums(mv, pr))
    print(json.dumps(rec), flush=True)
    out.append(rec)
    hip.close()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
