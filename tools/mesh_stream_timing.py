"""Timing of mesh streaming (tsdf_mesh_stream) beside the one-shot extraction (tsdf_mesh_extract) at the bench scene's c2 (512^3 culled, 4 streams).
1. Device time per stage from the library's HIP-event timers, streamed ("mesh_stream_count", "mesh_stream_scan" = the three scan launches + the header
   launch, "mesh_stream_emit" = packed vertices + triangles) and extracted ("mesh_count", "mesh_scan", "mesh_emit") on the same volume, each for
   positions alone, for normals alone, for colours alone and for all attributes.
2. Frames per second of the tsdf_frame_dev loop (timers off, a host clock around FRAMES frames that ends in a synchronise) in three forms: plain; with
   mesh_stream every frame (3-slot ring, frames picked up two late and copied out of the pinned buffer); with a synchronous extract + download
   every frame.  Bytes per frame to the host for both forms.
A record, not a threshold.  Prints one JSON line; with a file argument, also writes it to that file; --stages-only leaves part 2 out.
--level L[,L..] (0, 1, 2; default 0): the levels of detail to time (tsdf_mesh_stream_config_lod / tsdf_mesh_extract_lod).  In part 1 the levels alternate
call by call in this one process (the ring is configured anew for each call, outside the timers), in part 2 loop by loop; the record then has a "levels"
entry with each level's counts, capacities, stages (and the spread of the streamed device time over the N calls) and bytes per frame, and the frame
rates carry the level in their names.  The top-level entries stay those of the first level named.
--min-triangles N (default 0: no filter): the ring drops the components of fewer than N triangles on the device (tsdf_mesh_stream_config_filter).  The
streamed stages then include "mesh_stream_filter" (everything between the emit and the final header), every variant reports the filtered counts, the
four filter words and the payload bytes of the filtered and of the unfiltered frame, and the streamed loops are the filtered ring's.
--variants NAME[,NAME..] (positions, normals, colours, all_attributes; default all four): the attribute variants part 1 times.
--compact: instead of parts 1 and 2, the uint32 ring against the ring of 6-byte tile-local triangles (tsdf_mesh_stream_config_compact) in this one
process, per level and for positions / all attributes, the two formats alternating call by call: the stage timers, the payload bytes per frame (measured
from tsdf_mesh_stream_stats, and what the format's arithmetic gives), the host time from tsdf_mesh_stream on an idle device to the frame complete on the
host ("latency_ms"), the copy's share of it (latency - device stages) and the bandwidth that gives, and the frames per second of the streamed loop.
--slabs K: instead of parts 1 and 2, K Z-slab contexts of the same volume on this one device (recomputed halos), each with a part ring
(tsdf_mesh_stream_config_part), beside the whole-volume context's compact ring, at the first level named, for positions and all attributes: the stage
timers of every slab's part (count + scan + emit; the slowest slab is what a frame waits for when every slab has a device of its own) and of the
whole-volume ring, in WINDOWS windows of N calls with the two alternating call by call; and whether the joined parts equal the whole-volume frame.
--taps: instead of parts 1 and 2, the ring with packed texture taps in the frame (tsdf_mesh_stream_config_taps) against the same ring without, per level
(and with --min-triangles the filtered ring), alternating call by call: the stage timers and "mesh_stream_taps", the bytes per frame with and without
the block; beside them the two yardsticks on the same mesh -- "texture_taps" of tsdf_mesh_texture_taps (the fp32 form) and what TSDF_MESH_COLOURS
adds to "mesh_stream_emit" -- and the frames per second of the streamed loop with the tap ring on and off."""
import sys, os, json, time
from importlib import import_module
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch  # noqa: F401  (torch first: the library binds to the HIP runtime torch loaded)
import rgbd_recon_amd as rr
VIEW = (1280, 720)
N = 10
FRAMES = 300
EXTRACT_FRAMES = 30
STAGES_ONLY = "--stages-only" in sys.argv
ARGS = sys.argv[1:]
LEVELS = [int(x) for x in ARGS[ARGS.index("--level") + 1].split(",")] if "--level" in ARGS else [0]
MIN_TRIANGLES = int(ARGS[ARGS.index("--min-triangles") + 1]) if "--min-triangles" in ARGS else 0
SLABS = int(ARGS[ARGS.index("--slabs") + 1]) if "--slabs" in ARGS else 0
WINDOWS = 5
OUT = [a for i, a in enumerate(ARGS) if not a.startswith("--") and (i == 0 or ARGS[i - 1] not in ("--level", "--min-triangles", "--variants", "--slabs"))]
VARIANTS = (("positions", dict(normals=False, colours=False)), ("normals", dict(normals=True, colours=False)), ("colours", dict(normals=False, colours=True)),
            ("all_attributes", dict(normals=True, colours=True)))
if "--variants" in ARGS:
    VARIANTS = tuple(v for v in VARIANTS if v[0] in ARGS[ARGS.index("--variants") + 1].split(","))
STREAM_STAGES = ("mesh_stream_count", "mesh_stream_scan", "mesh_stream_emit") + (("mesh_stream_filter",) if MIN_TRIANGLES else ())
EXTRACT_STAGES = ("mesh_count", "mesh_scan", "mesh_emit")

scene = rr.scene.make_scene(n_streams=4, width=640, height=480, lut_res=128, inv_res=128)
ext = scene["bbox_max"] - scene["bbox_min"]
res = (512,) * 3
CTX = dict(res=res, brick_size=[float(ext[a]) / res[a] * 8 for a in range(3)], limit=0.01, view=VIEW)
hip = rr.ReconIntegrationHip(scene, **CTX)
mv, pr = rr.scene.default_view(*VIEW)
dev = [torch.from_numpy(np.ascontiguousarray(scene[k])).cuda() for k in ("depth", "quality", "silhouette", "color")]
torch.cuda.synchronize()
ptrs = [t.data_ptr() for t in dev]
for _ in range(4):                                                       # both volume sets hold the frame
    hip.frame_dev(mv, pr, ptrs)
hip.sync()
levels = {}
for L in LEVELS:
    mesh = hip.extract_mesh(normals=False, colours=False, level=L)
    st = hip.mesh_stats()
    nv, nt, ns = len(mesh["position"]), len(mesh["triangles"]), st["tiles_with_surface"]
    levels[L] = dict(vertices=nv, triangles=nt, tiles=st["tiles"], tiles_skipped=st["tiles_skipped"], tiles_with_surface=ns,
                     capacities=dict(max_vertices=nv + nv // 4, max_triangles=nt + nt // 4, max_surface_tiles=ns + ns // 4))
rec = dict(shape="c2", res=list(hip.res), streams=4, level=LEVELS[0], min_triangles=MIN_TRIANGLES, **{k: v for k, v in levels[LEVELS[0]].items()})


def compact_record():
    """--compact: format 0 against format 1"""
    out = dict(rec, tool="tools/mesh_stream_timing.py --compact", unit="ms (stages, latency), bytes, GB/s, frames/s", levels={})
    for L in LEVELS:
        out["levels"][str(L)] = dict(vertices=levels[L]["vertices"], triangles=levels[L]["triangles"], tiles_with_surface=levels[L]["tiles_with_surface"])
        for label, kw in [v for v in VARIANTS if v[0] in ("positions", "all_attributes")]:
            stride = 16 if (kw["normals"] or kw["colours"]) else 8
            samples = {fmt: dict(latency=[], bytes=[], **{s: [] for s in STREAM_STAGES}) for fmt in (0, 1)}
            info = {}
            hip.enable_timers(True)
            hip.set_timer_filter(list(STREAM_STAGES))
            for k in range(2 + N):                                       # two warm calls, then N; the formats alternate: both see the same machine
                for fmt in (0, 1):
                    hip.mesh_stream_config(slots=3, level=L, min_triangles=MIN_TRIANGLES, index_format=fmt, **kw, **levels[L]["capacities"])
                    hip.mesh_stream(0); hip.mesh_stream_take()           # (the configuration's first call allocates)
                    for s in STREAM_STAGES:
                        hip.timer_stats(s)
                    hip.sync()
                    before = hip.mesh_stream_stats()["payload_bytes"]
                    t0 = time.perf_counter()
                    hip.mesh_stream(1)
                    got = hip.mesh_stream_acquire(wait=True)
                    t1 = time.perf_counter()
                    info[fmt] = dict(n_vertices=got[2]["n_vertices"], n_triangles=got[2]["n_triangles"], rows=len(got[2]["compact"]["table"]) if fmt else 0)
                    assert got[2]["overflow"] == 0
                    hip.mesh_stream_release()
                    if k >= 2:
                        samples[fmt]["latency"].append((t1 - t0) * 1e3)
                        samples[fmt]["bytes"].append(hip.mesh_stream_stats()["payload_bytes"] - before)
                        for s in STREAM_STAGES:
                            cnt, total = hip.timer_stats(s)
                            samples[fmt][s].append(total / cnt)
            hip.enable_timers(False)
            r = {}
            for fmt in (0, 1):
                S, I = samples[fmt], info[fmt]
                t = {s + "_ms": float(np.mean(S[s])) for s in STREAM_STAGES}
                device = sum(t.values())
                nv, nt, rows = I["n_vertices"], I["n_triangles"], I["rows"]
                expected = ((nv * stride + 15) // 16 * 16 + rows * 16 + nt * 6 if nv else 0) if fmt else nv * stride + nt * 12
                assert set(S["bytes"]) == {expected}, (S["bytes"], expected)
                lat = float(np.median(S["latency"]))
                t.update(device_ms=device, latency_ms=lat, latency_ms_min=float(np.min(S["latency"])), latency_ms_max=float(np.max(S["latency"])),
                         payload_bytes=expected, table_rows=rows, n_vertices=nv, n_triangles=nt,
                         copy_ms=lat - device, copy_GB_per_s=expected / max(lat - device, 1e-6) / 1e6)
                r["format%d" % fmt] = t
            a, b = r["format0"], r["format1"]
            saved = a["payload_bytes"] - b["payload_bytes"]
            r["bytes_saved"] = saved
            r["bytes_saved_fraction"] = saved / max(a["payload_bytes"], 1)
            r["emit_and_filter_extra_ms"] = (b["mesh_stream_emit_ms"] + b.get("mesh_stream_filter_ms", 0.0)) - (a["mesh_stream_emit_ms"] + a.get("mesh_stream_filter_ms", 0.0))
            r["saved_bytes_copy_ms_at_format0_bandwidth"] = saved / max(a["copy_GB_per_s"], 1e-9) / 1e6
            r["latency_saved_ms"] = a["latency_ms"] - b["latency_ms"]
            out["levels"][str(L)][label] = r
    def streamed(f):
        hip.mesh_stream(f)
        if hip.mesh_stream_stats()["frames"] - streamed.taken > 2:
            hip.mesh_stream_take(); streamed.taken += 1
    def drain():
        while hip.mesh_stream_stats()["frames"] > streamed.taken:
            hip.mesh_stream_take(); streamed.taken += 1
    def loop(n):
        for f in range(10):
            hip.frame_dev(mv, pr, ptrs); streamed(f)
        drain(); hip.sync()
        t0 = time.perf_counter()
        for f in range(n):
            hip.frame_dev(mv, pr, ptrs); streamed(f)
        drain(); hip.sync()
        return n / (time.perf_counter() - t0)
    fps = {}
    for rep in range(0 if STAGES_ONLY else 3):
        for L in LEVELS:
            for label, kw in [v for v in VARIANTS if v[0] in ("positions", "all_attributes")]:
                for fmt in (0, 1):
                    hip.mesh_stream_config(slots=3, level=L, min_triangles=MIN_TRIANGLES, index_format=fmt, **kw, **levels[L]["capacities"])
                    streamed.taken = 0
                    fps.setdefault("level%d_%s_format%d" % (L, label, fmt), []).append(loop(FRAMES))
    out["frames_per_s"] = {k: dict(runs=[round(x, 1) for x in v], median=round(float(np.median(v)), 1)) for k, v in fps.items()}
    return out


def slabs_record():
    """--slabs K: the part rings of K slab contexts beside the whole-volume compact ring"""
    mgpu = import_module("rgbd-recon_amd.multigpu")
    L = LEVELS[0]
    out = dict(rec, tool="tools/mesh_stream_timing.py --slabs %d" % SLABS, unit="ms", slabs=SLABS, windows=WINDOWS, calls_per_window=N)
    ctxs = [rr.ReconIntegrationHip(scene, slab=mgpu.slab_range(res[2], k, SLABS), recompute_halo=True, **CTX) for k in range(SLABS)]
    for c in ctxs:
        c.clearOccupiedBricks(); c.markBricks(); c.updateOccupiedBricks(); c.integrate(); c.sync()
    everyone = [hip] + ctxs
    for label, kw in [v for v in VARIANTS if v[0] in ("positions", "all_attributes")]:
        stride = 16 if (kw["normals"] or kw["colours"]) else 8
        hip.mesh_stream_config(slots=3, level=L, index_format=rr.MESH_INDEX_TILE16, **kw, **levels[L]["capacities"])
        for c in ctxs:
            c.mesh_stream_config(slots=3, level=L, part=True, **kw, **levels[L]["capacities"])
        hip.mesh_stream(0); want = hip.mesh_stream_take()                # (the configuration's first call allocates)
        parts, joined = mgpu.mesh_parts_on_one_device(ctxs)
        assert want[2]["overflow"] == 0 and joined is not None
        identical = (joined[0].tobytes() == want[0].tobytes() and joined[1].tobytes() == want[1].tobytes() and
                     joined[2]["compact"]["table"].tobytes() == want[2]["compact"]["table"].tobytes())
        for c in everyone:
            c.enable_timers(True); c.set_timer_filter(list(STREAM_STAGES))
        windows = []
        for w in range(WINDOWS):
            ms = [{s: [] for s in STREAM_STAGES} for _ in everyone]
            for k in range(2 + N):                                       # two warm calls, then N; whole and slabs alternate: all see the same machine
                for i, c in enumerate(everyone):
                    c.mesh_stream(k); c.mesh_stream_take()
                    for s in STREAM_STAGES:
                        cnt, total = c.timer_stats(s)
                        if k >= 2:
                            ms[i][s].append(total / cnt)
            mean = [{s + "_ms": float(np.mean(m[s])) for s in STREAM_STAGES} for m in ms]
            for m in mean:
                m["device_ms"] = sum(m.values())
            slow = max(range(SLABS), key=lambda k: mean[1 + k]["device_ms"])
            windows.append(dict(whole_volume=mean[0], per_slab_device_ms=[m["device_ms"] for m in mean[1:]], slowest_slab=slow, slowest=mean[1 + slow],
                                sum_of_slabs_ms=sum(m["device_ms"] for m in mean[1:])))
        for c in everyone:
            c.enable_timers(False)
        per = [dict(planes=list(mgpu.slab_range(res[2], k, SLABS)), vertices=p[2]["n_vertices"], triangles=p[2]["n_triangles"], surface_tiles=p[2]["needed_tiles"],
                    seam_tiles=p[2]["part"]["seam_tiles"], payload_bytes=(p[2]["n_vertices"] * stride + 15) // 16 * 16 + p[2]["needed_tiles"] * 16 + p[2]["n_triangles"] * 6
                    if p[2]["n_vertices"] else 0) for k, p in enumerate(parts)]
        whole_ms, slow_ms = [w["whole_volume"]["device_ms"] for w in windows], [w["slowest"]["device_ms"] for w in windows]
        out[label] = dict(identical_to_whole_volume=bool(identical), per_slab=per, windows=windows,
                          whole_volume_device_ms=dict(median=float(np.median(whole_ms)), min=min(whole_ms), max=max(whole_ms)),
                          slowest_slab_device_ms=dict(median=float(np.median(slow_ms)), min=min(slow_ms), max=max(slow_ms)),
                          whole_volume_payload_bytes=(want[2]["n_vertices"] * stride + 15) // 16 * 16 + want[2]["needed_tiles"] * 16 + want[2]["n_triangles"] * 6,
                          sum_of_parts_payload_bytes=sum(r["payload_bytes"] for r in per))
    for c in ctxs:
        c.close()
    return out


def taps_record():
    """--taps: the ring with the tap block against the ring without"""
    stages = STREAM_STAGES + ("mesh_stream_taps",)
    out = dict(rec, tool="tools/mesh_stream_timing.py --taps", unit="ms (stages), bytes, frames/s", calls=N, levels={})
    hip.enable_timers(True)
    hip.set_timer_filter(list(stages) + ["texture_taps"])
    for L in LEVELS:
        r = dict(vertices=levels[L]["vertices"], triangles=levels[L]["triangles"])
        rings = dict(plain=dict(normals=False, colours=False, taps=False), taps=dict(normals=False, colours=False, taps=True),
                     colours=dict(normals=False, colours=True, taps=False), colours_taps=dict(normals=False, colours=True, taps=True))
        samples = {k: dict(bytes=[], **{s: [] for s in stages}) for k in rings}
        fp32 = []
        for k in range(2 + N):                                           # two warm calls, then N; the rings alternate: all see the same machine
            for name, kw in rings.items():
                hip.mesh_stream_config(slots=3, level=L, min_triangles=MIN_TRIANGLES, **kw, **levels[L]["capacities"])
                hip.mesh_stream(0); hip.mesh_stream_take()               # (the configuration's first call allocates)
                for s in stages:
                    hip.timer_stats(s)
                before = hip.mesh_stream_stats()["payload_bytes"]
                hip.mesh_stream(1)
                got = hip.mesh_stream_take()
                assert got[2]["overflow"] == 0 and (("taps" in got[2]) == kw["taps"])
                r.setdefault("n_vertices", got[2]["n_vertices"])
                if k >= 2:
                    samples[name]["bytes"].append(hip.mesh_stream_stats()["payload_bytes"] - before)
                    for s in stages:
                        cnt, total = hip.timer_stats(s)
                        samples[name][s].append(total / cnt if cnt else 0.0)
            hip.extract_mesh(normals=False, colours=False, level=L)      # the yardstick: the fp32 taps of the one-shot extract at the same level
            hip.timer_stats("texture_taps")
            hip.mesh_texture_taps(download=False)
            cnt, total = hip.timer_stats("texture_taps")
            if k >= 2:
                fp32.append(total)                                       # (summed over the call's launches)
        for name in rings:
            S = samples[name]
            assert len(set(S["bytes"])) == 1
            r[name] = dict(payload_and_tap_bytes=S["bytes"][0], **{s + "_ms": float(np.mean(S[s])) for s in stages},
                           mesh_stream_taps_ms_min=float(np.min(S["mesh_stream_taps"])), mesh_stream_taps_ms_max=float(np.max(S["mesh_stream_taps"])))
        r["tap_bytes_per_frame"] = r["taps"]["payload_and_tap_bytes"] - r["plain"]["payload_and_tap_bytes"]
        r["fp32_texture_taps_ms"] = float(np.mean(fp32))
        r["colours_add_to_emit_ms"] = r["colours"]["mesh_stream_emit_ms"] - r["plain"]["mesh_stream_emit_ms"]
        out["levels"][str(L)] = r
    hip.enable_timers(False)
    def streamed(f):
        hip.mesh_stream(f)
        if hip.mesh_stream_stats()["frames"] - streamed.taken > 2:
            hip.mesh_stream_take(); streamed.taken += 1
    def loop(n):
        for f in range(10):
            hip.frame_dev(mv, pr, ptrs); streamed(f)
        while hip.mesh_stream_stats()["frames"] > streamed.taken:
            hip.mesh_stream_take(); streamed.taken += 1
        hip.sync()
        t0 = time.perf_counter()
        for f in range(n):
            hip.frame_dev(mv, pr, ptrs); streamed(f)
        while hip.mesh_stream_stats()["frames"] > streamed.taken:
            hip.mesh_stream_take(); streamed.taken += 1
        hip.sync()
        return n / (time.perf_counter() - t0)
    fps = {}
    for rep_ in range(0 if STAGES_ONLY else 3):
        for L in LEVELS:
            for taps in (False, True):
                hip.mesh_stream_config(slots=3, level=L, min_triangles=MIN_TRIANGLES, taps=taps, **levels[L]["capacities"])
                streamed.taken = 0
                fps.setdefault("level%d_positions_%s" % (L, "taps" if taps else "plain"), []).append(loop(FRAMES))
    out["frames_per_s"] = {k: dict(runs=[round(x, 1) for x in v], median=round(float(np.median(v)), 1)) for k, v in fps.items()}
    return out


if SLABS or "--compact" in ARGS or "--taps" in ARGS:
    rec = slabs_record() if SLABS else taps_record() if "--taps" in ARGS else compact_record()
    print(json.dumps(rec), flush=True)
    if OUT:
        with open(OUT[0], "w") as f:
            json.dump(rec, f, indent=1)
    hip.close()
    sys.exit(0)

# 1. device time per stage
hip.enable_timers(True)
hip.set_timer_filter(list(STREAM_STAGES + EXTRACT_STAGES))
def one_call(L, kw):
    """one streamed frame and one extract of level L; with one level the ring keeps its configuration"""
    if len(LEVELS) > 1 or not one_call.configured:
        hip.mesh_stream_config(slots=3, level=L, min_triangles=MIN_TRIANGLES, **kw, **levels[L]["capacities"])
        one_call.configured = True
    hip.mesh_stream(0); got = hip.mesh_stream_take()
    hip.extract_mesh(level=L, **kw)
    return got
for label, kw in VARIANTS:
    one_call.configured = False
    for _ in range(2):
        for L in LEVELS:
            got = one_call(L, kw)
            assert got[2]["overflow"] == 0 and got[2]["needed_vertices"] == levels[L]["vertices"] and got[2]["needed_triangles"] == levels[L]["triangles"]
            if MIN_TRIANGLES:
                f = got[2]["filter"]
                assert got[2]["n_vertices"] == levels[L]["vertices"] - f["vertices_removed"] and got[2]["n_triangles"] == levels[L]["triangles"] - f["triangles_removed"]
                levels[L]["filtered"] = dict(vertices=got[2]["n_vertices"], triangles=got[2]["n_triangles"], **f)
            else:
                assert got[2]["n_vertices"] == levels[L]["vertices"] and got[2]["n_triangles"] == levels[L]["triangles"]
    for s in STREAM_STAGES + EXTRACT_STAGES:
        hip.timer_stats(s)                                               # (resets the timer's samples)
    samples = {L: {s: [] for s in STREAM_STAGES + EXTRACT_STAGES} for L in LEVELS}
    for _ in range(N):                                                   # alternating: both forms, and every level, see the same machine
        for L in LEVELS:
            one_call(L, kw)
            for s in STREAM_STAGES + EXTRACT_STAGES:
                cnt, total = hip.timer_stats(s)
                samples[L][s].append(total / cnt)
    stride = 16 if (kw["normals"] or kw["colours"]) else 8
    for L in LEVELS:
        r = {}
        for name, stages in (("stream", STREAM_STAGES), ("extract", EXTRACT_STAGES)):
            t = {s + "_ms": float(np.mean(samples[L][s])) for s in stages}
            per_call = np.sum([samples[L][s] for s in stages], axis=0)
            t["device_ms"] = sum(t.values())
            t["device_ms_min"], t["device_ms_max"] = float(per_call.min()), float(per_call.max())
            r[name] = t
        nv, nt = levels[L]["vertices"], levels[L]["triangles"]
        r["stream_bytes_per_frame"] = nv * stride + nt * 12 + 64        # payload + header
        if MIN_TRIANGLES:                                                # the unfiltered frame's bytes stay beside what the filtered ring sends
            r["stream_unfiltered_bytes_per_frame"] = r["stream_bytes_per_frame"]
            r["stream_bytes_per_frame"] = levels[L]["filtered"]["vertices"] * stride + levels[L]["filtered"]["triangles"] * 12 + 128   # payload + record + header
        r["extract_bytes_per_frame"] = nv * (12 + (12 if kw["normals"] else 0) + (16 if kw["colours"] else 0)) + nt * 12
        levels[L][label] = r
    rec[label] = levels[LEVELS[0]][label]
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
suffix = (lambda L: "_level%d" % L) if "--level" in ARGS else (lambda L: "")
for rep in range(0 if STAGES_ONLY else 3):                              # the three forms in turn, three times: the spread is part of the record
    for L in LEVELS:
        for label, kw in [v for v in VARIANTS if v[0] in ("positions", "all_attributes")]:
            hip.mesh_stream_config(slots=3, level=L, min_triangles=MIN_TRIANGLES, **kw, **levels[L]["capacities"])
            streamed.taken = 0
            before = hip.mesh_stream_stats()["payload_bytes"]
            fps.setdefault("stream_" + label + suffix(L), []).append(loop(FRAMES, streamed, drain_stream))
            levels[L][label]["stream_payload_bytes_measured"] = (hip.mesh_stream_stats()["payload_bytes"] - before) // (FRAMES + 10)
            fps.setdefault("extract_" + label + suffix(L), []).append(loop(EXTRACT_FRAMES, lambda f: hip.extract_mesh(level=L, **kw), nothing))
    fps.setdefault("plain", []).append(loop(FRAMES, lambda f: None, nothing))
if fps:
    rec["frames_per_s"] = {k: dict(runs=[round(x, 1) for x in v], median=round(float(np.median(v)), 1)) for k, v in fps.items()}
if MIN_TRIANGLES:
    rec["filtered"] = levels[LEVELS[0]]["filtered"]
if "--level" in ARGS:
    rec["levels"] = {str(L): levels[L] for L in LEVELS}
print(json.dumps(rec), flush=True)
if OUT:
    with open(OUT[0], "w") as f:
        json.dump(rec, f, indent=1)
hip.close()
