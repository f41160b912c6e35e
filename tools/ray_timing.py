"""Timing of the ray queries (tsdf_cast_rays) after one frame at the bench scene's c2 (512^3 culled, 4 streams).  Device time from the library's HIP-event
timers "rays_march" and "rays_surface" (summed over the launch pairs of a cast), mean of N casts, for
  (a) the 1280 x 720 view's own rays (tsdf_view_rays), beside the timers of tsdf_raymarch on the same view with space skipping off and on ("k_march":
      the march launch; "draw": march + shading) -- the yardstick: the same rays through the pixel-grid kernels;
  (b) 1 M random rays from origins on a sphere around the box towards random points in it (world coordinates);
  (c) the rays of (b) sorted by the storage tile they enter the box in.
Each with the fetched / accounted sample ratio (tsdf_ray_stats) and the longest ray.  A record, not a threshold.  Prints one JSON line; with a file
argument, also writes it to that file.
--slabs K: instead, the view's own rays cast on K Z-slab contexts (tsdf_cast_rays_part_dev): the slowest slab's part cast, the merge
(tsdf_merge_ray_parts_dev) and the whole-volume cast of the same rays, with each part's share of samples that are only walked in front of its run."""
import sys, os, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch  # noqa: F401  (torch first: the library binds to the HIP runtime torch loaded)
import rgbd_recon_amd as rr
VIEW = (1280, 720)
N = 10
ARGS = sys.argv[1:]
SLABS = int(ARGS[ARGS.index("--slabs") + 1]) if "--slabs" in ARGS else 0
OUT = [a for k, a in enumerate(ARGS) if not a.startswith("--") and not (k and ARGS[k - 1] == "--slabs")]

scene = rr.scene.make_scene(n_streams=4, width=640, height=480, lut_res=128, inv_res=128)
lo, hi = np.asarray(scene["bbox_min"], np.float64), np.asarray(scene["bbox_max"], np.float64)
ext = hi - lo
res = (512,) * 3


def time_slabs(world):
    """--slabs K: the view's own rays on K slab contexts (recomputed halos, so no exchange is needed) -- per slab the part cast's device time (timers
    "rays_part_march" + "rays_part_surface", normals and colours) and its sample counts, the merge (torch events around tsdf_merge_ray_parts_dev on
    an adopted stream), and the whole-volume cast of the same rays from the same process.  in_front: the additions a slab performs in front of its owned
    run, counted on the host from the merged answer's geometry (chained float32 additions, the header's owner plane); in_front_share = in_front /
    (in_front + owned samples accounted for): the share of a part's samples that are only walked."""
    from importlib import import_module
    m = import_module("rgbd-recon_amd.multigpu")
    kw = dict(res=res, brick_size=[float(ext[a]) / res[a] * 8 for a in range(3)], limit=0.01, view=VIEW)
    mv, pr = rr.scene.default_view(*VIEW)
    whole = rr.ReconIntegrationHip(scene, **kw)
    whole.clearOccupiedBricks(); whole.markBricks(); whole.updateOccupiedBricks(); whole.integrate()
    rays = whole.view_rays(mv, pr)
    n = len(rays)
    whole.enable_timers(True)
    whole.set_timer_filter(["rays_march", "rays_surface"])
    for _ in range(2):
        want = whole.cast_rays(rays, normals=True, colours=True, unit_cube=True)
    whole.timer_stats("rays_march"); whole.timer_stats("rays_surface")
    for _ in range(N):
        whole.cast_rays(rays, normals=True, colours=True, unit_cube=True)
    rec = dict(shape="c2", res=list(res), streams=4, view=list(VIEW), casts=N, slabs=world, rays=n,
               whole=dict(rays_march_ms=whole.timer_stats("rays_march")[1] / N, rays_surface_ms=whole.timer_stats("rays_surface")[1] / N, **whole.ray_stats()))
    whole.close()
    ranges = [m.slab_range(res[2], k, world) for k in range(world)]
    u8 = dict(dtype=torch.uint8, device="cuda")
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(n, 32).copy()).cuda()
    hit_parts, surf_parts = torch.zeros((world, n, 32), **u8), torch.zeros((world, n, 32), **u8)
    hits, surf = torch.zeros((n, 32), **u8), torch.zeros((n, 32), **u8)
    torch.cuda.synchronize()
    # the additions in front of each slab's run: the rays' sample planes on the host
    fronts = _in_front(_setup(rays), ranges)
    parts = []
    for k, zr in enumerate(ranges):
        b = rr.ReconIntegrationHip(scene, slab=zr, recompute_halo=True, **kw)
        b.clearOccupiedBricks(); b.markBricks(); b.updateOccupiedBricks(False); b.integrate()
        b.enable_timers(True)
        b.set_timer_filter(["rays_part_march", "rays_part_surface"])
        for _ in range(2):
            b.cast_rays_part_dev(d_rays.data_ptr(), n, hit_parts[k].data_ptr(), surf_parts[k].data_ptr(), normals=True, colours=True, unit_cube=True)
        b.sync()
        b.timer_stats("rays_part_march"); b.timer_stats("rays_part_surface")
        for _ in range(N):
            b.cast_rays_part_dev(d_rays.data_ptr(), n, hit_parts[k].data_ptr(), surf_parts[k].data_ptr(), normals=True, colours=True, unit_cube=True)
        b.sync()
        st = b.ray_stats()
        front = fronts[k]
        parts.append(dict(planes=list(zr), rays_part_march_ms=b.timer_stats("rays_part_march")[1] / N, rays_part_surface_ms=b.timer_stats("rays_part_surface")[1] / N,
                          hits=st["hits"], samples=st["samples"], fetched=st["fetched"], in_front=front, in_front_share=front / max(front + st["samples"], 1)))
        if k + 1 < world:
            b.close()
    stream = torch.cuda.Stream()                                         # the merge, on the last context (any context merges)
    b.set_stream(stream.cuda_stream)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    with torch.cuda.stream(stream):
        for _ in range(2):
            b.merge_ray_parts_dev(hit_parts.data_ptr(), surf_parts.data_ptr(), world, n, n, hits.data_ptr(), surf.data_ptr())
        ev[0].record(stream)
        for _ in range(N):
            b.merge_ray_parts_dev(hit_parts.data_ptr(), surf_parts.data_ptr(), world, n, n, hits.data_ptr(), surf.data_ptr())
        ev[1].record(stream)
    stream.synchronize()
    b.set_stream(None)
    b.close()
    slow = max(parts, key=lambda p: p["rays_part_march_ms"] + p["rays_part_surface_ms"])
    rec.update(parts=parts, merge_ms=ev[0].elapsed_time(ev[1]) / N, slowest_part_ms=slow["rays_part_march_ms"] + slow["rays_part_surface_ms"],
               slowest_part_planes=slow["planes"], slowest_part_in_front_share=slow["in_front_share"],
               merged_equals_whole=bool(hits.cpu().numpy().tobytes() == want[0].tobytes() and surf.cpu().numpy().tobytes() == want[1].tobytes()))
    return rec


def _setup(rays):
    """start position, step and sample count of unit-cube rays with t_min = 0, t_max = inf (the header's arithmetic in float32)"""
    f32 = np.float32
    o, d = rays["origin"].astype(f32), rays["dir"].astype(f32)
    sd = f32(f32(0.01) * f32(0.5))
    with np.errstate(all="ignore"):
        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).astype(f32)).astype(f32)
        step = ((d * (f32(1.0) / length)[:, None]).astype(f32) * sd).astype(f32)
        inv = (f32(1.0) / step).astype(f32)
        tbot, ttop = (inv * (f32(0.0) - o)).astype(f32), (inv * (f32(1.0) - o)).astype(f32)
        tmn, tmx = np.fmin(ttop, tbot), np.fmax(ttop, tbot)
        t0 = np.fmax(np.fmax(tmn[:, 0], tmn[:, 1]), np.fmax(tmn[:, 0], tmn[:, 2]))
        t1 = np.fmin(np.fmin(tmx[:, 0], tmx[:, 1]), np.fmin(tmx[:, 0], tmx[:, 2]))
        ok = (t0 <= t1) & ~(t1 < 0)
        t_near = np.where(t0 < 0, f32(0.0), t0).astype(f32)
        z = (o[:, 2] + step[:, 2] * t_near).astype(f32)
        max_n = np.where(ok, np.minimum(np.ceil(np.abs(t1 - t_near)), f32(4.0) / f32(0.01) + f32(2.0)), 0).astype(np.int64)
    return dict(z=z, dz=step[:, 2], max_n=max_n)


def _in_front(S, ranges):
    """per slab (voxel planes [z0, z1)): the samples its part cast only walks, summed over the rays -- those in front of the first sample whose owner
    plane lies in tile layers [z0 / 8, (z1 + 7) / 8), and all max_n of a ray that starts behind the slab and never owns a sample.  z is monotonic along
    a ray, so one histogram of the samples' layers per direction of travel answers for every slab."""
    f32 = np.float32
    layers = (res[2] + 7) // 8
    z, left, up = S["z"].copy(), S["max_n"].copy(), S["dz"] >= 0
    hist = np.zeros((2, layers), np.int64)                               # [travelling down / up][layer]

    def layer_of(z):
        with np.errstate(all="ignore"):
            return np.fmin(np.fmax(np.floor((z * f32(res[2])).astype(f32)), f32(0.0)), f32(res[2] - 1)).astype(np.int64) >> 3
    first = layer_of(z)
    for _ in range(int(S["max_n"].max()) if len(z) else 0):
        live = left > 0
        if not live.any():
            break
        layer = layer_of(z)
        hist[1] += np.bincount(layer[live & up], minlength=layers)
        hist[0] += np.bincount(layer[live & ~up], minlength=layers)
        left -= 1
        z = (z + S["dz"]).astype(f32)
    out = []
    for z0, z1 in ranges:
        l0, l1 = z0 // 8, (z1 + 7) // 8
        behind = (up & (first >= l1)) | (~up & (first < l0))             # never owns a sample: the part walks the whole ray
        walked_behind = int(S["max_n"][behind].sum())
        out.append(int(hist[1][:l0].sum() + hist[0][l1:].sum()) + walked_behind)
    return out


if SLABS:
    rec = time_slabs(SLABS)
    print(json.dumps(rec), flush=True)
    if OUT:
        with open(OUT[0], "w") as f:
            json.dump(rec, f, indent=1)
    sys.exit(0)

hip = rr.ReconIntegrationHip(scene, res=res, brick_size=[float(ext[a]) / res[a] * 8 for a in range(3)], limit=0.01, view=VIEW)
mv, pr = rr.scene.default_view(*VIEW)
hip.clearOccupiedBricks(); hip.markBricks(); hip.updateOccupiedBricks(); hip.integrate(); hip.drawF(mv, pr)
hip.sync()
hip.enable_timers(True)
hip.set_timer_filter(["rays_march", "rays_surface", "k_march", "draw"])
rec = dict(shape="c2", res=list(hip.res), streams=4, view=list(VIEW), casts=N)


def per_call(name, calls):
    cnt, total = hip.timer_stats(name)                                   # (resets the timer)
    return total / calls if cnt else 0.0


def time_cast(rays, unit_cube):
    out = {}
    for label, kw in (("march_only", {}), ("normals_and_colours", dict(normals=True, colours=True))):
        for _ in range(2):
            got = hip.cast_rays(rays, unit_cube=unit_cube, **kw)
        per_call("rays_march", 1); per_call("rays_surface", 1)
        for _ in range(N):
            hip.cast_rays(rays, unit_cube=unit_cube, **kw)
        out[label] = dict(rays_march_ms=per_call("rays_march", N), rays_surface_ms=per_call("rays_surface", N))
    hits = got[0]
    s = hip.ray_stats()
    out.update(rays=s["rays"], hits=s["hits"], samples=s["samples"], fetched=s["fetched"], fetched_over_samples=s["fetched"] / max(s["samples"], 1),
               longest_ray=int(hits["n_samples"].max()), mean_samples=float(hits["n_samples"].mean()))
    return out


# (a) the view's own rays, and the draw on the same view
view = hip.view_rays(mv, pr)
rec["view_rays"] = time_cast(view, True)
for skip in (False, True):
    hip.setSpaceSkip(skip)
    for _ in range(2):
        hip.draw(mv, pr)
    hip.sync()
    per_call("k_march", 1); per_call("draw", 1)
    for _ in range(N):
        hip.draw(mv, pr)
    hip.sync()
    rec["raymarch_skip_" + ("on" if skip else "off")] = dict(k_march_ms=per_call("k_march", N), draw_ms=per_call("draw", N))
hip.setSpaceSkip(True)

# (b) random rays: origins on a sphere around the box (unit-cube frame, radius 1.2 about the centre), towards random points in the box
rng = np.random.default_rng(20221019)
n = 1 << 20
u = rng.normal(size=(n, 3))
u /= np.linalg.norm(u, axis=1, keepdims=True)
origin = 0.5 + 1.2 * u
d = rng.uniform(0.0, 1.0, (n, 3)) - origin
rays = rr.make_rays(lo + origin * ext, d * ext)
rec["random_rays"] = time_cast(rays, False)

# (c) the same rays ordered by the storage tile of their entry point (slab test in float64; this only orders them)
with np.errstate(divide="ignore", invalid="ignore"):
    t0 = np.fmax.reduce(np.fmin((0.0 - origin) / d, (1.0 - origin) / d), axis=1)
entry = np.clip(origin + d * np.maximum(t0, 0.0)[:, None], 0.0, 1.0 - 1e-9)
tile = (entry * (np.asarray(res) / 8)).astype(np.int64)
order = np.argsort((tile[:, 2] * 64 + tile[:, 1]) * 64 + tile[:, 0], kind="stable")
rec["random_rays_sorted_by_entry_tile"] = time_cast(rays[order], False)

print(json.dumps(rec), flush=True)
if OUT:
    with open(OUT[0], "w") as f:
        json.dump(rec, f, indent=1)
hip.close()
