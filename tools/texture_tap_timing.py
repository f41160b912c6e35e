"""Timing of the texture taps (tsdf_texture_taps / tsdf_mesh_texture_taps) after one frame at the bench scene's c2 (512^3 culled, 4 streams).  Device
time from the library's HIP-event timer "texture_taps" (summed over the launches of a call), mean of N calls, for
  (a) the level-0 mesh and (b) the level-2 mesh of the fused surface (tsdf_mesh_texture_taps: over the mesh's position array on the device), without and
      with sensor records;
  (c) 1 M random points of the bounding box (tsdf_texture_taps, world coordinates);
each with tsdf_texture_tap_stats.  Beside (a) and (b) the yardstick: what TSDF_MESH_COLOURS adds to tsdf_mesh_extract on the same mesh, "mesh_emit" with
the flag minus "mesh_emit" without it -- that colour pass performs the same LUT and image fetches plus the colour taps, in blend_colors()' 128-register
waves.  A record, not a threshold.  Prints one JSON line; with a file argument, also writes it to that file."""
import sys, os, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch  # noqa: F401  (torch first: the library binds to the HIP runtime torch loaded)
import rgbd_recon_amd as rr
VIEW = (1280, 720)
N = 10
OUT = [a for a in sys.argv[1:] if not a.startswith("--")]

scene = rr.scene.make_scene(n_streams=4, width=640, height=480, lut_res=128, inv_res=128)
lo, hi = np.asarray(scene["bbox_min"], np.float64), np.asarray(scene["bbox_max"], np.float64)
ext = hi - lo
res = (512,) * 3
hip = rr.ReconIntegrationHip(scene, res=res, brick_size=[float(ext[a]) / res[a] * 8 for a in range(3)], limit=0.01, view=VIEW)
mv, pr = rr.scene.default_view(*VIEW)
hip.clearOccupiedBricks(); hip.markBricks(); hip.updateOccupiedBricks(); hip.integrate(); hip.drawF(mv, pr)
hip.sync()
hip.enable_timers(True)
hip.set_timer_filter(["texture_taps", "mesh_emit"])
rec = dict(shape="c2", res=list(hip.res), streams=4, calls=N)


def per_call(name, calls):
    cnt, total = hip.timer_stats(name)                                   # (resets the timer)
    return total / calls if cnt else 0.0


def emit_ms(colours, level):
    for _ in range(2):
        hip.extract_mesh(normals=False, colours=colours, level=level)
    per_call("mesh_emit", 1)
    for _ in range(N):
        hip.extract_mesh(normals=False, colours=colours, level=level)
    return per_call("mesh_emit", N)


for level in (0, 2):
    out = {}
    with_colours = emit_ms(True, level)
    plain = emit_ms(False, level)                                        # (leaves the mesh the taps are taken of)
    out.update(mesh_emit_ms=plain, mesh_emit_with_colours_ms=with_colours, mesh_colours_add_ms=with_colours - plain)
    for label, sensor in (("taps_ms", False), ("taps_with_sensor_ms", True)):
        for _ in range(2):
            nv, ns = hip.mesh_texture_taps(sensor=sensor, download=False)
        per_call("texture_taps", 1)
        for _ in range(N):
            hip.mesh_texture_taps(sensor=sensor, download=False)
        out[label] = per_call("texture_taps", N)
    out.update(vertices=nv, stats=hip.texture_tap_stats(), taps_bytes=nv * ns * 16, launches=(nv + (1 << 18) - 1) >> 18)
    rec[f"mesh_level_{level}"] = out

# (c) random points of the bounding box
rng = np.random.default_rng(20221019)
n = 1 << 20
pts = (lo + rng.uniform(0.0, 1.0, (n, 3)) * ext).astype(np.float32)
out = {}
for label, sensor in (("taps_ms", False), ("taps_with_sensor_ms", True)):
    for _ in range(2):
        hip.texture_taps(pts, sensor=sensor)
    per_call("texture_taps", 1)
    for _ in range(N):
        hip.texture_taps(pts, sensor=sensor)
    out[label] = per_call("texture_taps", N)
out.update(points=n, stats=hip.texture_tap_stats(), launches=n >> 18)
rec["random_points"] = out

print(json.dumps(rec), flush=True)
if OUT:
    with open(OUT[0], "w") as f:
        json.dump(rec, f, indent=1)
hip.close()
