"""Timing of the mesh extraction (tsdf_mesh_extract) beside the read-out it replaces, tsdf_download_volume, after one frame at the bench scene's
c2 (512^3 culled, 4 streams).  Device time per stage from the library's HIP-event timers: "mesh_count" (one launch), "mesh_scan" (three), "mesh_emit"
(vertices + triangles), each for the position-only extract and for the one with normals and colours; the volume download is bracketed by a timer of
this tool's own on the context's stream (tile-major -> linear launch + the 512 MiB copy to pageable host memory).  A record, not a threshold.  Prints
one JSON line; with a file argument, also writes it to that file.
--level L[,L..] (0, 1, 2; default 0): the levels of detail to time (tsdf_mesh_extract_lod), alternating call by call in this one process so that every
level sees the same machine; the record then has a "levels" entry with each level's stages, the spread of its device time over the N calls, its counts
and its mesh bytes.  The top-level entries stay those of the first level named.
--components: after that, N times extract (every attribute, the first level named) + tsdf_mesh_components, and with --min-triangles M also
tsdf_mesh_filter_components(M): the record gets a "components" entry with the timers "mesh_components" and "mesh_filter" (each the sum of its call's two
samples: the host sizes an allocation between them) beside mesh_count / mesh_scan / mesh_emit of the same extracts, and the counts.
--components --measures: also tsdf_mesh_component_measures after every labelling: "components" gets the timer "mesh_component_measures" (one sample:
three launches) beside "mesh_components" of the same run, and the largest component's area and volume in SI units.  With --min-extent-m X the filter is
tsdf_mesh_filter_components_measured(min_extent = ceil(X / unit)) instead of the triangle count's (not both).
--slabs K: the same volume once more as K Z-slab contexts (recomputed halos) on this one device, each extracting its part of the first level named with
every attribute (tsdf_mesh_slab_extract / _link): the record gets a "slabs" entry with every slab's "mesh_slab_count" / "_scan" / "_emit" / "_link"
device time, its counts and its tiles with surface, whether the joined parts equal the whole-volume extract byte for byte, and the slowest slab's time
and share of the surface tiles beside the whole-volume extract's device time of this run.
--slabs K --components: the linked parts are labelled where they are (tsdf_mesh_slab_components, the host merge merge_mesh_component_seams through the
library, tsdf_mesh_slab_link_components): "slabs" gets a "components" entry with every slab's "mesh_slab_components" / "mesh_slab_components_link" device
time, its list sizes and their bytes, the host merge's wall time (and the numpy twin's, once), whether the joined labels equal the whole-volume
context's byte for byte, and the slowest slab beside "mesh_components" of the whole volume in this run."""
import sys, os, json, time
from importlib import import_module
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch  # noqa: F401  (torch first: the library binds to the HIP runtime torch loaded)
import rgbd_recon_amd as rr
VIEW = (1280, 720)
N = 10
STAGES = ("mesh_count", "mesh_scan", "mesh_emit")
ARGS = sys.argv[1:]
LEVELS = [int(x) for x in ARGS[ARGS.index("--level") + 1].split(",")] if "--level" in ARGS else [0]
COMPONENTS = "--components" in ARGS or "--min-triangles" in ARGS
MEASURES = "--measures" in ARGS or "--min-extent-m" in ARGS
MIN_EXTENT_M = float(ARGS[ARGS.index("--min-extent-m") + 1]) if "--min-extent-m" in ARGS else None
assert not MEASURES or COMPONENTS, "--measures goes with --components"
assert MIN_EXTENT_M is None or "--min-triangles" not in ARGS, "one filter per labelling: --min-triangles or --min-extent-m"
MIN_TRIANGLES = int(ARGS[ARGS.index("--min-triangles") + 1]) if "--min-triangles" in ARGS else None
SLABS = int(ARGS[ARGS.index("--slabs") + 1]) if "--slabs" in ARGS else 0
SLAB_STAGES = ("mesh_slab_count", "mesh_slab_scan", "mesh_slab_emit", "mesh_slab_link")
OUT = [a for i, a in enumerate(ARGS) if not a.startswith("--") and (i == 0 or ARGS[i - 1] not in ("--level", "--min-triangles", "--slabs", "--min-extent-m"))]

scene = rr.scene.make_scene(n_streams=4, width=640, height=480, lut_res=128, inv_res=128)
ext = scene["bbox_max"] - scene["bbox_min"]
res = (512,) * 3
CTX = dict(res=res, brick_size=[float(ext[a]) / res[a] * 8 for a in range(3)], limit=0.01, view=VIEW)
hip = rr.ReconIntegrationHip(scene, **CTX)
mv, pr = rr.scene.default_view(*VIEW)
hip.clearOccupiedBricks(); hip.markBricks(); hip.updateOccupiedBricks(); hip.integrate(); hip.drawF(mv, pr)
hip.sync()
hip.enable_timers(True)
hip.set_timer_filter(list(STAGES) + ["volume_download", "mesh_components", "mesh_filter", "mesh_component_measures"])
rec = dict(shape="c2", res=list(hip.res), streams=4)
levels = {L: {} for L in LEVELS}
for label, kw in (("positions", dict(normals=False, colours=False)), ("all_attributes", dict(normals=True, colours=True))):
    for _ in range(2):
        for L in LEVELS:
            mesh = hip.extract_mesh(level=L, **kw)
            st = hip.mesh_stats()
            levels[L].update(vertices=len(mesh["position"]), triangles=len(mesh["triangles"]), tiles=st["tiles"], tiles_skipped=st["tiles_skipped"],
                             tiles_with_surface=st["tiles_with_surface"])
            levels[L]["mesh_bytes_" + label] = st["bytes"]
    for s in STAGES:
        hip.timer_stats(s)                                               # (resets the timer's samples)
    samples = {L: {s: [] for s in STAGES} for L in LEVELS}
    wall = {L: 0.0 for L in LEVELS}
    for _ in range(N):                                                   # the levels in turn, N times: all of them see the same machine
        for L in LEVELS:
            t0 = time.perf_counter()
            hip.extract_mesh(level=L, **kw)
            wall[L] += time.perf_counter() - t0
            for s in STAGES:
                cnt, total = hip.timer_stats(s)
                samples[L][s].append(total / cnt)
    for L in LEVELS:
        r = {s + "_ms": float(np.mean(samples[L][s])) for s in STAGES}
        per_call = np.sum([samples[L][s] for s in STAGES], axis=0)
        r["device_ms"] = sum(r.values())
        r["device_ms_min"], r["device_ms_max"] = float(per_call.min()), float(per_call.max())
        r["call_and_download_wall_ms"] = wall[L] / N * 1e3               # extract + tsdf_mesh_download into numpy arrays
        levels[L][label] = r
first = levels[LEVELS[0]]
for label in ("positions", "all_attributes"):
    rec[label] = first[label]
rec.update(level=LEVELS[0], vertices=first["vertices"], triangles=first["triangles"], mesh_bytes=first["mesh_bytes_all_attributes"], tiles=first["tiles"],
           tiles_skipped=first["tiles_skipped"], tiles_with_surface=first["tiles_with_surface"])
if "--level" in ARGS:
    rec["levels"] = {str(L): levels[L] for L in LEVELS}
if COMPONENTS:
    names = STAGES + ("mesh_components",) + (("mesh_component_measures",) if MEASURES else ()) + (("mesh_filter",) if MIN_TRIANGLES is not None or MIN_EXTENT_M is not None else ())
    ms = {s: [] for s in names}
    comp = dict(level=LEVELS[0])
    for it in range(N + 1):                                              # (the first turn is a warm-up)
        hip.extract_mesh(level=LEVELS[0], normals=True, colours=True)
        comp["components"] = hip.mesh_components()
        comp.update(largest_triangles=hip.mesh_component_stats()["largest_triangles"])
        if MEASURES:
            grid = hip.mesh_component_measures()
            if not it:
                rows, table = hip.mesh_download_component_measures(), hip.mesh_download_components()["table"]
                big = int(np.argmax(table["n_triangles"]))
                si = rr.mesh_measures_si(rows, grid, table)
                comp.update(measure_unit_m=grid["unit"], largest_area_m2=float(si["area"][big]), largest_volume_m3=float(si["volume"][big]),
                            total_area_m2=float(si["area"].sum()), negative_volume_components=int((si["volume"] < 0).sum()))
        if MIN_EXTENT_M is not None:
            rule = hip.mesh_measure_rule(min_extent_m=MIN_EXTENT_M)
            comp["kept_vertices"], comp["kept_triangles"] = hip.mesh_filter_measured(rule)
            st = hip.mesh_component_stats()
            comp.update(min_extent_m=MIN_EXTENT_M, min_extent=int(rule["min_extent"]), vertices_removed=st["vertices_removed"], triangles_removed=st["triangles_removed"])
        if MIN_TRIANGLES is not None:
            comp["kept_vertices"], comp["kept_triangles"] = hip.mesh_filter(MIN_TRIANGLES)
            st = hip.mesh_component_stats()
            comp.update(min_triangles=MIN_TRIANGLES, vertices_removed=st["vertices_removed"], triangles_removed=st["triangles_removed"])
        for s in names:
            cnt, total = hip.timer_stats(s)                              # (the samples of this turn alone: timer_stats resets them)
            if it:
                ms[s].append(total)
    for s in names:
        comp[s + "_ms"], comp[s + "_ms_min"], comp[s + "_ms_max"] = float(np.mean(ms[s])), float(np.min(ms[s])), float(np.max(ms[s]))
    comp["extract_ms"] = sum(comp[s + "_ms"] for s in STAGES)
    rec["components"] = comp
hip.tsdf()
hip.timer_stats("volume_download")
t0 = time.perf_counter()
for _ in range(3):
    hip.timer_begin("volume_download"); vol = hip.tsdf(); hip.timer_end("volume_download")
rec["volume_download_wall_ms"] = (time.perf_counter() - t0) / 3 * 1e3
cnt, total = hip.timer_stats("volume_download")
rec["volume_download_ms"] = total / cnt
rec["volume_bytes"] = int(vol.nbytes)
del vol
if SLABS:
    mgpu = import_module("rgbd-recon_amd.multigpu")
    L0 = LEVELS[0]
    whole = hip.extract_mesh(level=L0, normals=True, colours=True)
    ctxs = [rr.ReconIntegrationHip(scene, slab=mgpu.slab_range(res[2], k, SLABS), recompute_halo=True, **CTX) for k in range(SLABS)]
    for c in ctxs:
        c.clearOccupiedBricks(); c.markBricks(); c.updateOccupiedBricks(); c.integrate(); c.sync()
        c.enable_timers(True)
        c.set_timer_filter(list(SLAB_STAGES))
    joined = mgpu.mesh_slabs_on_one_device(ctxs, normals=True, colours=True, level=L0)          # (also the warm-up)
    identical = all(joined[k].tobytes() == whole[k].tobytes() for k in ("position", "normal", "colour", "triangles"))
    for c in ctxs:
        for s in SLAB_STAGES:
            c.timer_stats(s)
    ms = [{s: [] for s in SLAB_STAGES} for _ in ctxs]
    for _ in range(N):
        counts = [c.extract_mesh_slab(True, True, L0) for c in ctxs]
        seams = [c.mesh_slab_seam() for c in ctxs]
        base = 0
        for k, c in enumerate(ctxs):
            c.mesh_slab_link(base, seams[k + 1] if k + 1 < SLABS else None)
            base += counts[k][0]
            for s in SLAB_STAGES:
                cnt, total = c.timer_stats(s)
                ms[k][s].append(total / cnt if cnt else 0.0)
    per = []
    for k, c in enumerate(ctxs):
        st = c.mesh_slab_stats()
        r = {s + "_ms": float(np.mean(ms[k][s])) for s in SLAB_STAGES}
        r["device_ms"] = sum(r.values())
        r.update(planes=list(mgpu.slab_range(res[2], k, SLABS)), vertices=counts[k][0], triangles=counts[k][1], tiles=st["tiles"], tiles_skipped=st["tiles_skipped"],
                 tiles_with_surface=st["tiles_with_surface"])
        per.append(r)
    slow = max(per, key=lambda r: r["device_ms"])
    surface = sum(r["tiles_with_surface"] for r in per)
    rec["slabs"] = dict(n=SLABS, level=L0, identical_to_whole_volume=bool(identical), per_slab=per, slowest_slab_ms=slow["device_ms"],
                        slowest_slab_surface_share=slow["tiles_with_surface"] / max(surface, 1), sum_of_slabs_ms=sum(r["device_ms"] for r in per),
                        whole_volume_device_ms=levels[L0]["all_attributes"]["device_ms"])
    if COMPONENTS:                                                       # the parts are linked: label them where they are
        CC = ("mesh_slab_components", "mesh_slab_components_link")
        for c in ctxs:
            c.set_timer_filter(list(SLAB_STAGES) + list(CC))
        hip.extract_mesh(level=L0, normals=True, colours=True)
        hip.mesh_components()
        want = hip.mesh_download_components()
        got = mgpu.mesh_components_on_one_device(ctxs)                   # (also the warm-up)
        same = all(got[k].tobytes() == want[k].tobytes() for k in ("vertex_component", "triangle_component", "table"))
        for c in ctxs:
            for s in CC:
                c.timer_stats(s)
        cms = [{s: [] for s in CC} for _ in ctxs]
        merge_ms = []
        for _ in range(N):
            lists, base = [], 0
            for k, c in enumerate(ctxs):
                n = c.mesh_slab_components()
                lists.append(dict(vertex_base=base, n_vertices=counts[k][0], n_local=n["local_components"], **c.mesh_slab_component_seam()))
                base += counts[k][0]
            t0 = time.perf_counter()
            merged = rr.merge_mesh_component_seams(lists, native=True)   # the library's host function
            merge_ms.append((time.perf_counter() - t0) * 1e3)
            for k, c in enumerate(ctxs):
                c.mesh_slab_link_components(merged["component_base"][k], merged["links"][k])
                for s in CC:
                    cnt, total = c.timer_stats(s)                        # (step 1 is two samples: the host sizes the lists between them)
                    cms[k][s].append(total)
        t0 = time.perf_counter()
        twin = rr.merge_mesh_component_seams(lists)
        twin_ms = (time.perf_counter() - t0) * 1e3
        cper = []
        for k, c in enumerate(ctxs):
            st = c.mesh_slab_component_stats()
            r = {s + "_ms": float(np.mean(cms[k][s])) for s in CC}
            r["device_ms"] = sum(r.values())
            r.update(st, down_records=len(lists[k]["down"]), up_records=len(lists[k]["up"]), root_records=len(lists[k]["roots"]),
                     seam_bytes=8 * (len(lists[k]["down"]) + len(lists[k]["up"])) + 16 * len(lists[k]["roots"]), link_bytes=32 * len(lists[k]["roots"]))
            cper.append(r)
        cslow = max(cper, key=lambda r: r["device_ms"])
        rec["slabs"]["components"] = dict(
            identical_to_whole_volume=bool(same), components=got["n_components"], per_slab=cper, slowest_slab_ms=cslow["device_ms"],
            sum_of_slabs_ms=sum(r["device_ms"] for r in cper), host_merge_ms=float(np.mean(merge_ms)), host_merge_ms_min=float(np.min(merge_ms)),
            host_merge_ms_max=float(np.max(merge_ms)), numpy_twin_merge_ms=twin_ms,
            numpy_twin_identical=all(a.tobytes() == b.tobytes() for a, b in zip(twin["links"], merged["links"])),
            whole_volume_mesh_components_ms=rec["components"]["mesh_components_ms"])
    for c in ctxs:
        c.close()
print(json.dumps(rec), flush=True)
if OUT:
    with open(OUT[0], "w") as f:
        json.dump(rec, f, indent=1)
hip.close()
