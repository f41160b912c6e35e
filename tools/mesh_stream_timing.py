"""Timing of mesh streaming (tsdf_mesh_stream) beside the one-shot extraction (tsdf_mesh_extract) at the bench scene's c2 (512^3 culled, 4 streams).
1. Device time per stage from the library's HIP-event timers, streamed ("mesh_stream_count", "mesh_stream_scan" = the three scan launches + the header
   launch, "mesh_stream_emit" = packed vertices + triangles) and extracted ("mesh_count", "mesh_scan", "mesh_emit") on the same volume, each for
   positions alone, for normals alone, for colours alone and for all attributes.
2. Frames per second of the tsdf_frame_dev loop (timers off, a host clock around FRAMES frames that ends in a synchronise) in three forms: plain; with
   mesh_stream every frame (3-slot ring, frames picked up two late and copied out of the pinned buffer); with a synchronous extract + download
   every frame.  Bytes per frame to the host for both forms.
A record, not a threshold.  Prints one JSON line; with a file argument, also writes it to that file; --stages-only leaves part 2 out."""
import sys, os, json, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch  # noqa: F401  (torch first: the library binds to the HIP runtime torch loaded)
import rgbd_recon_amd as rr
VIEW = (1280, 720)
N = 10
FRAMES = 300
EXTRACT_FRAMES = 30
STAGES_ONLY = "--stages-only" in sys.argv
OUT = [a for a in sys.argv[1:] if not a.startswith("--")]
VARIANTS = (("positions", dict(normals=False, colours=False)), ("normals", dict(normals=True, colours=False)), ("colours", dict(normals=False, colours=True)),
            ("all_attributes", dict(normals=True, colours=True)))
STREAM_STAGES = ("mesh_stream_count", "mesh_stream_scan", "mesh_stream_emit")
EXTRACT_STAGES = ("mesh_count", "mesh_scan", "mesh_emit")

scene = rr.scene.make_scene(n_streams=4, width=640, height=480, lut_res=128, inv_res=128)
ext = scene["bbox_max"] - scene["bbox_min"]
res = (512,) * 3
hip = rr.ReconIntegrationHip(scene, res=res, brick_size=[float(ext[a]) / res[a] * 8 for a in range(3)], limit=0.01, view=VIEW)
mv, pr = rr.scene.default_view(*VIEW)
dev = [torch.from_numpy(np.ascontiguousarray(scene[k])).cuda() for k in ("depth", "quality", "silhouette", "color")]
torch.cuda.synchronize()
ptrs = [t.data_ptr() for t in dev]
for _ in range(4):                                                       # both volume sets hold the frame
    hip.frame_dev(mv, pr, ptrs)
hip.sync()
mesh = hip.extract_mesh(normals=False, colours=False)
st = hip.mesh_stats()
nv, nt, ns = len(mesh["position"]), len(mesh["triangles"]), st["tiles_with_surface"]
caps = dict(max_vertices=nv + nv // 4, max_triangles=nt + nt // 4, max_surface_tiles=ns + ns // 4)
rec = dict(shape="c2", res=list(hip.res), streams=4, vertices=nv, triangles=nt, tiles=st["tiles"], tiles_skipped=st["tiles_skipped"], tiles_with_surface=ns,
           capacities=caps)

# 1. device time per stage
hip.enable_timers(True)
hip.set_timer_filter(list(STREAM_STAGES + EXTRACT_STAGES))
for label, kw in VARIANTS:
    hip.mesh_stream_config(slots=3, **kw, **caps)
    for _ in range(2):
        hip.mesh_stream(0); got = hip.mesh_stream_take()
        hip.extract_mesh(**kw)
    assert got[2]["overflow"] == 0 and got[2]["n_vertices"] == nv and got[2]["n_triangles"] == nt
    for s in STREAM_STAGES + EXTRACT_STAGES:
        hip.timer_stats(s)                                               # (resets the timer's samples)
    for _ in range(N):                                                   # alternating: both forms see the same machine
        hip.mesh_stream(0); hip.mesh_stream_take()
        hip.extract_mesh(**kw)
    r = {}
    for name, stages in (("stream", STREAM_STAGES), ("extract", EXTRACT_STAGES)):
        t = {s + "_ms": (lambda ct: ct[1] / ct[0])(hip.timer_stats(s)) for s in stages}
        t["device_ms"] = sum(t.values())
        r[name] = t
    stride = 16 if (kw["normals"] or kw["colours"]) else 8
    r["stream_bytes_per_frame"] = nv * stride + nt * 12 + 64            # payload + header
    r["extract_bytes_per_frame"] = nv * (12 + (12 if kw["normals"] else 0) + (16 if kw["colours"] else 0)) + nt * 12
    rec[label] = r
hip.enable_timers(False)

# 2. the frame loop
def loop(n, per_frame, drain):
    for f in range(10):
        hip.frame_dev(mv, pr, ptrs); per_frame(f)
    drain(); hip.sync()
    t0 = time.perf_counter()
    for f in range(n):
        hip.frame_dev(mv, pr, ptrs); per_frame(f)
    drain(); hip.sync()
    return n / (time.perf_counter() - t0)

def streamed(f):
    hip.mesh_stream(f)
    if hip.mesh_stream_stats()["frames"] - streamed.taken > 2:
        hip.mesh_stream_take(); streamed.taken += 1
def drain_stream():
    while hip.mesh_stream_stats()["frames"] > streamed.taken:
        hip.mesh_stream_take(); streamed.taken += 1

nothing = lambda: None
fps = {}
for rep in range(0 if STAGES_ONLY else 3):                              # the three forms in turn, three times: the spread is part of the record
    for label, kw in (("positions", dict(normals=False, colours=False)), ("all_attributes", dict(normals=True, colours=True))):
        hip.mesh_stream_config(slots=3, **kw, **caps)
        streamed.taken = 0
        before = hip.mesh_stream_stats()["payload_bytes"]
        fps.setdefault("stream_" + label, []).append(loop(FRAMES, streamed, drain_stream))
        rec[label]["stream_payload_bytes_measured"] = (hip.mesh_stream_stats()["payload_bytes"] - before) // (FRAMES + 10)
        fps.setdefault("extract_" + label, []).append(loop(EXTRACT_FRAMES, lambda f: hip.extract_mesh(**kw), nothing))
    fps.setdefault("plain", []).append(loop(FRAMES, lambda f: None, nothing))
if fps:
    rec["frames_per_s"] = {k: dict(runs=[round(x, 1) for x in v], median=round(float(np.median(v)), 1)) for k, v in fps.items()}
print(json.dumps(rec), flush=True)
if OUT:
    with open(OUT[0], "w") as f:
        json.dump(rec, f, indent=1)
hip.close()
