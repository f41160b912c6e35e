"""GPU: ray queries (tsdf_cast_rays / tsdf_cast_rays_dev / tsdf_view_rays) against the draw they restate, against tests/ray_reference.py byte for byte,
across dense / culled / sparse storage (skipping empty space changes nothing and happens), through the lanes beside a twin that casts synchronously, and
every error code."""
import numpy as np
import pytest

import main_path_cases as K
import main_path_reference as R
import mesh_lod_reference as L
import mesh_reference as M
import ray_reference as Q

pytestmark = pytest.mark.gpu

LIMIT = 0.04
KW = dict(brick_size=[2.0 / 8, 2.2 / 8, 2.0 / 8], limit=LIMIT, view=(64, 36))
f32 = np.float32


def integrate(hip):
    hip.clearOccupiedBricks()
    hip.markBricks()
    hip.updateOccupiedBricks()
    hip.integrate()


def code(rr, fn):
    with pytest.raises(rr.TsdfError) as e:
        fn()
    return e.value.code


def assert_same(got, want, what):
    ok = Q.same_bytes(got, want)
    bad = np.nonzero(~ok)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(ok)} records differ, e.g. {bad[0]}: device {got[bad[0]]} reference {want[bad[0]]}"


# ---------------------------------------------------------------------------------------------------------------- the draw's rays
def test_view_rays_reproduce_the_draw(rr, small_scene):
    """small_scene at 32^3, 64 x 36, space skipping off, shade mode 0 (which writes blendColors through unchanged): per pixel the cast of the draw's
    own ray has the draw's sample count, hit, depth and colour -- the kernels' and the oracle's."""
    from oracle.oracle import OracleRecon
    kw = dict(res=(32, 32, 32), **KW)
    hip, orc = rr.ReconIntegrationHip(small_scene, **kw), OracleRecon(small_scene, **kw)
    mv, pr = rr.scene.default_view(64, 36)
    for o in (hip, orc):
        o.setSpaceSkip(False)
        integrate(o)
        o.draw(mv, pr)
    rays = hip.view_rays(mv, pr)
    assert rays.shape == (64 * 36,) and (rays["t_min"] == 0).all() and np.isposinf(rays["t_max"]).all()
    assert (rays["origin"] == rays["origin"][0]).all()
    one = hip.view_rays(mv, pr, (17, 9, 3, 2))                           # a rectangle is the same rays, row-major
    assert one.tobytes() == rays.reshape(36, 64)[9:11, 17:20].tobytes()
    hits, surf = hip.cast_rays(rays, colours=True, unit_cube=True)
    hits, surf = hits.reshape(36, 64), surf.reshape(36, 64)
    hit = (hits["status"] & rr.RAY_HIT) != 0
    V = R.View(mv, pr, (64, 36), small_scene["bbox_min"], small_scene["bbox_max"])
    with np.errstate(invalid="ignore"):
        fd = np.where(hit, np.clip(V.frag_depth(hits["pos"].astype(np.float64)), 0.0, 1.0), 1.0)
    assert hit.sum() > 100 and (fd[hit] < 1).all()                      # the view: every hit lies before the far plane (the draw drops fd >= 1)
    tol = K.TABLE["march_depth"]["tol"]
    for name, o in (("kernels", hip), ("oracle", orc)):
        rgba, depth, ns, _ = o.view_images()
        assert (hits["n_samples"] == np.rint(ns.astype(np.float64) / 0.0027)).all(), name
        assert (hit == (depth < 1)).all(), name
        assert np.abs(fd - depth.astype(np.float64)).max() <= tol, name
        assert (surf["rgba"][hit].view(np.uint32) == rgba[hit].view(np.uint32)).all(), name
    p = hip.pick(mv, pr, *[int(v) for v in np.argwhere(hit)[len(np.argwhere(hit)) // 2][::-1]])
    assert p["hit"] and np.isfinite(p["position"]).all() and abs(np.linalg.norm(p["normal"]) - 1) < 1e-5
    assert not hip.pick(mv, pr, 0, 0)["hit"] or hit[0, 0]
    hip.close()


# ---------------------------------------------------------------------------------------------------------------- arbitrary rays
def ray_mix(seed, n, inside_points, bbox_min, bbox_max, world):
    """n rays in the unit cube's frame (mapped to world coordinates when `world`): origins outside aimed into the box, aimed away (a miss), inside the box,
    inside the surface; axis-parallel directions; un-normalised directions; finite t_min / t_max on a quarter; the invalid kinds."""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 16, n)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    origin = 0.5 + u * rng.uniform(0.9, 1.6, (n, 1))                    # on shells around the box ...
    target = rng.uniform(0.05, 0.95, (n, 3))
    d = target - origin
    inside = kind >= 10                                                  # ... 6 of 16 inside the box, any direction
    origin[inside] = rng.uniform(0.0, 1.0, (int(inside.sum()), 3))
    d[inside] = rng.normal(size=(int(inside.sum()), 3))
    solid = kind >= 14                                                   # 2 of 16 start inside the surface
    origin[solid] = inside_points[rng.integers(0, len(inside_points), int(solid.sum()))]
    away = kind == 0                                                     # 1 of 16 misses the box
    d[away] = -d[away]
    axis = (kind == 1) | (kind == 10)                                    # 2 of 16 axis-parallel, from outside and from inside
    a = rng.integers(0, 3, n)
    e = np.zeros((n, 3))
    e[np.arange(n), a] = np.where(origin[np.arange(n), a] > 0.5, -1.0, 1.0)
    origin[kind == 1] = np.where(e[kind == 1] != 0, origin[kind == 1], target[kind == 1])
    d[axis] = e[axis]
    d *= rng.uniform(0.1, 5.0, (n, 1))                                   # un-normalised
    rays = Q.make_rays(origin, d)
    quarter = rng.random(n) < 0.25
    length = np.linalg.norm(d, axis=1)
    rays["t_min"][quarter] = (rng.uniform(-0.2, 1.2, n) / length)[quarter]
    rays["t_max"][quarter] = (rng.uniform(0.3, 2.5, n) / length)[quarter]
    if world:
        lo = np.asarray(bbox_min, np.float64)
        ext = np.asarray(bbox_max, np.float64) - lo
        rays["origin"] = lo + rays["origin"].astype(np.float64) * ext
        rays["dir"] = rays["dir"].astype(np.float64) * ext
    bad = rng.choice(n, 12, replace=False)                               # the invalid kinds, three of each
    rays["dir"][bad[0:3]] = 0.0
    rays["origin"][bad[3:6], 1] = np.nan
    rays["dir"][bad[6:9], 2] = np.inf
    rays["t_min"][bad[9:12]] = np.nan
    rays["origin"][bad[9], 0] = -np.inf
    return rays


def planted_volume():
    """37 x 43 x 35 (padded tiles on every axis): mesh_lod_reference.random_volume -- noise with zeros, -0, NaN, +-inf -- inside a ball, exact -limit
    around it so that rays travel before they hit, and a few of the special values planted in the free space as well"""
    res = (37, 43, 35)
    vol = L.random_volume(res, limit=LIMIT)
    p = R.voxel_positions(res)
    ball = np.linalg.norm(p - (0.5, 0.48, 0.52), axis=-1) < 0.3
    vol = np.where(ball, vol, f32(-LIMIT)).astype(f32)
    rng = np.random.default_rng(7)
    free = np.argwhere(~ball)
    for k, v in enumerate((np.nan, -0.0, 0.0, -np.inf, np.nan, np.inf)):
        z, y, x = free[rng.integers(0, len(free), 40)].T
        if np.isposinf(v):                                               # (a +inf voxel is a hit: a few, so that most rays still reach the ball)
            z, y, x = z[:3], y[:3], x[:3]
        vol[z, y, x] = v
    return res, np.ascontiguousarray(vol)


def check_against_reference(rr, hip, scene, vol, rays, world, colours, what):
    want = Q.cast(vol, LIMIT, scene["bbox_min"], scene["bbox_max"], rays, unit_cube=not world)
    hits, surf = hip.cast_rays(rays, normals=True, colours=colours, unit_cube=not world)
    st = want["hits"]["status"]
    print(f"{what}: {len(rays)} rays, {int((st & 1).sum())} hits, {int((st == 2).sum())} miss the box, {int((st == 4).sum())} invalid, "
          f"{int(want['hits']['n_samples'].sum())} samples, longest {int(want['hits']['n_samples'].max())}; device stats {hip.ray_stats()}")
    assert_same(hits, want["hits"], what + " hits")
    assert_same(surf, Q.surface(vol, scene, LIMIT, scene["bbox_min"], scene["bbox_max"], want, normals=True, colours=colours), what + " surface")
    s = hip.ray_stats()
    assert s["rays"] == len(rays) and s["hits"] == int((st & 1).sum()) and s["samples"] == int(want["hits"]["n_samples"].sum())
    assert s["fetched"] <= s["samples"]
    return want, hits, surf


@pytest.mark.parametrize("world", [False, True], ids=["unit-cube", "world"])
def test_planted_volume_byte_equal(rr, small_scene, world):
    res, vol = planted_volume()
    hip = rr.ReconIntegrationHip(small_scene, res=res, **KW)
    hip.set_tsdf(vol)
    inside = R.voxel_positions(res)[np.nan_to_num(vol, nan=-1.0) > 0]
    rays = ray_mix(11 + world, 4096, inside, small_scene["bbox_min"], small_scene["bbox_max"], world)
    want, hits, _ = check_against_reference(rr, hip, small_scene, vol, rays, world, True, f"planted volume {'world' if world else 'unit cube'}")
    st = want["hits"]["status"]
    assert (st & 1).sum() > 1000 and (st == 2).sum() > 100 and (st == 4).sum() == 12 and (want["hits"]["n_samples"][(st & 1) != 0] == 1).sum() > 100
    assert want["hits"]["n_samples"].max() > 40                         # rays do travel
    s = hip.ray_stats()
    assert s["fetched"] == s["samples"]                                 # an uploaded volume: every class is kTileMixed, nothing may be skipped
    # the attribute flags select: normals alone, colours alone, neither (no surface array at all)
    h1, s1 = hip.cast_rays(rays, normals=True, unit_cube=not world)
    h2, s2 = hip.cast_rays(rays, colours=True, unit_cube=not world)
    h0 = hip.cast_rays(rays, unit_cube=not world)
    assert h0.tobytes() == h1.tobytes() == h2.tobytes() == hits.tobytes()
    assert not s1["rgba"].any() and not s2["normal"].any() and s1["normal"].any() and s2["rgba"].any()
    # ray counts around a wave: 0, 1, 63, 64, 65
    for n in (0, 1, 63, 64, 65):
        part = hip.cast_rays(rays[:n], unit_cube=not world)
        assert part.shape == (n,) and part.tobytes() == hits[:n].tobytes(), n
        assert hip.ray_stats()["rays"] == n
    hip.close()


def storage_contexts(rr, scene, res):
    """the same scene integrated dense with the bricks off, culled, and culled in a sparse pool"""
    out = {}
    for name, kw, bricks in (("dense", {}, False), ("culled", {}, True), ("sparse", dict(sparse_pool_tiles=512), True)):
        hip = rr.ReconIntegrationHip(scene, res=res, **kw, **KW)
        hip.setUseBricks(bricks)
        integrate(hip)
        out[name] = hip
    return out


def test_integrated_scene_byte_equal_and_skipping_changes_nothing(rr, small_scene):
    res = (64, 64, 64)
    ctx = storage_contexts(rr, small_scene, res)
    vols = {k: h.tsdf() for k, h in ctx.items()}
    inside = R.voxel_positions(res)[np.nan_to_num(vols["culled"], nan=-1.0) > 0]
    assert len(inside) > 100
    rays = ray_mix(5, 4096, inside, small_scene["bbox_min"], small_scene["bbox_max"], True)
    got = {}
    for name, hip in ctx.items():                                       # each against the reference on its own volume, normals and colours
        _, got[name], _ = check_against_reference(rr, hip, small_scene, vols[name], rays, True, True, f"small_scene 64^3 {name}")
    # outside the occupied bricks the culled volumes hold the clear value where the dense one holds what integrate() computed: where the three volumes
    # agree along a ray (decided on the reference's samples: the ray's answer is the same on all three), the answers must be identical
    if vols["culled"].tobytes() == vols["sparse"].tobytes():
        assert got["culled"].tobytes() == got["sparse"].tobytes()
    same_vol = (vols["dense"].view(np.uint32) == vols["culled"].view(np.uint32)).all()
    agree = Q.same_bytes(got["dense"], got["culled"])
    print(f"dense and culled volumes identical: {bool(same_vol)}; rays with identical answers: {int(agree.sum())} of {len(rays)}")
    if same_vol:
        assert agree.all()
    # ... and skipping happens: on the culled and the sparse context fewer samples are fetched than accounted for
    for name in ("culled", "sparse"):
        ctx[name].cast_rays(rays)
        s = ctx[name].ray_stats()
        print(name, s)
        assert 0 < s["fetched"] < s["samples"], (name, s)
    for hip in ctx.values():
        hip.close()


# ---------------------------------------------------------------------------------------------------------------- through the lanes
@pytest.mark.parametrize("rings", [False, True], ids=["alone", "beside-mesh-and-present-rings"])
def test_device_form_through_the_lanes(rr, rings):
    """Two scenes alternate for four frames through tsdf_frame_dev with stage overlap on (the volume sets alternate per frame).  tsdf_cast_rays_dev is
    queued behind every frame with no host wait in between; a twin integrates the same frames and casts synchronously.  A smoke check of the arrangement:
    the integrate of frame f + 2 must not reset the set frame f's rays still read (DESIGN.md argues it from the code)."""
    import torch
    mk = dict(n_streams=2, width=160, height=120, lut_res=32, inv_res=32)
    scs = [rr.scene.make_scene(**mk), rr.scene.make_scene(**mk, sphere_c=(0.4, 0.7, -0.3), box_c=(-0.5, 1.5, 0.2))]
    raw = [[torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ("depth", "quality", "silhouette", "color")] for sc in scs]
    mv, pr = rr.scene.default_view(64, 36)
    frames, n = 4, 2048
    inside = np.array([[0.5, 0.5, 0.5]])
    rays = ray_mix(3, n, inside, scs[0]["bbox_min"], scs[0]["bbox_max"], True)
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(n, 32).copy()).cuda()
    d_hits = [torch.zeros((n, 32), dtype=torch.uint8, device="cuda") for _ in range(frames)]
    d_surf = [torch.zeros((n, 32), dtype=torch.uint8, device="cuda") for _ in range(frames)]
    torch.cuda.synchronize()

    hip = rr.ReconIntegrationHip(scs[0], res=(32, 32, 32), **KW)
    if rings:
        hip.mesh_stream_config(normals=True, colours=True, slots=frames, max_vertices=1 << 17, max_triangles=1 << 18, max_surface_tiles=64)
        hip.present_config(rr.PRESENT_RGBA8, 0, frames)
    for f in range(frames):                                             # no host wait inside the loop
        hip.frame_dev(mv, pr, [t.data_ptr() for t in raw[f % 2]])
        if rings:
            hip.present(f)
            hip.mesh_stream(f)
        hip.cast_rays_dev(d_rays.data_ptr(), n, d_hits[f].data_ptr(), d_surf[f].data_ptr(), normals=True, colours=True)
    hip.sync()
    assert hip.ray_stats()["rays"] == n
    hip.close()

    twin = rr.ReconIntegrationHip(scs[0], res=(32, 32, 32), **KW)
    want = []
    for f in range(frames):
        twin.frame_dev(mv, pr, [t.data_ptr() for t in raw[f % 2]])
        want.append(twin.cast_rays(rays, normals=True, colours=True))
    twin.close()
    assert want[0][0].tobytes() != want[1][0].tobytes()                 # the two frames differ
    for f in range(frames):
        hits = d_hits[f].cpu().numpy().reshape(-1).view(rr.RAY_HIT_DTYPE)
        surf = d_surf[f].cpu().numpy().reshape(-1).view(rr.RAY_SURFACE_DTYPE)
        assert ((hits["status"] & 1) != 0).sum() > 200, f
        assert_same(hits, want[f][0], f"frame {f} hits")
        assert_same(surf, want[f][1], f"frame {f} surface")


# ---------------------------------------------------------------------------------------------------------------- errors
def test_error_codes(rr, small_scene):
    import ctypes as C
    mv, pr = rr.scene.default_view(64, 36)
    rays = Q.make_rays([(0.5, 0.5, 1.5)], [(0.0, 0.0, -1.0)])
    hip = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), **KW)
    lib, c = hip._L, hip._c
    assert code(rr, lambda: hip.cast_rays(rays)) == -4                  # before the first integrate / upload_volume
    assert code(rr, lambda: hip.ray_stats()) == -4                      # before any cast
    assert len(hip.view_rays(mv, pr, (0, 0, 2, 2))) == 4                # the view's rays need no volume
    integrate(hip)
    assert hip.cast_rays(rays, unit_cube=True).shape == (1,)
    ray, hit, surf = rr.Ray(), rr.RayHit(), rr.RaySurface()
    cast = lambda r, n, flags, h, s: lib.tsdf_cast_rays(c, r, C.c_uint64(n), C.c_uint32(flags), h, s)
    cast_dev = lambda r, n, flags, h, s: lib.tsdf_cast_rays_dev(c, r, C.c_uint64(n), C.c_uint32(flags), h, s)
    for fn in (cast, cast_dev):
        assert fn(C.byref(ray), 1, 8, C.byref(hit), None) == -1         # an unknown flag
        assert fn(None, 0, 8, None, None) == -1                         # ... with nothing to cast as well
        assert fn(None, 1, 0, C.byref(hit), None) == -1                 # NULL arrays with n > 0
        assert fn(C.byref(ray), 1, 0, None, None) == -1
        assert fn(C.byref(ray), 1, rr.RAY_NORMALS, C.byref(hit), None) == -1      # surface is NULL exactly when neither attribute flag is set
        assert fn(C.byref(ray), 1, 0, C.byref(hit), C.byref(surf)) == -1
        assert fn(None, 0, 0, None, None) == 0                          # n == 0: TSDF_OK, nothing launched
    assert hip.ray_stats() == dict(rays=0, hits=0, samples=0, fetched=0)
    for rect in ((0, 0, 0, 1), (0, 0, 65, 1), (63, 35, 2, 1), (-1, 0, 1, 1), (0, 36, 1, 1)):
        assert code(rr, lambda: hip.view_rays(mv, pr, rect)) == -1, rect
    assert code(rr, lambda: hip.view_rays(np.zeros(16, f32), pr, (0, 0, 1, 1))) == -1       # a singular matrix
    assert lib.tsdf_view_rays(c, None, None, 0, 0, 1, 1, C.byref(ray)) == -1
    hip.close()

    bare = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), upload=False, **KW)          # a volume, but neither calibration nor frame
    bare.set_tsdf(M.sphere_volume((32, 32, 32), limit=LIMIT))
    assert code(rr, lambda: bare.cast_rays(rays, colours=True, unit_cube=True)) == -4
    hits, surf = bare.cast_rays(rays, normals=True, unit_cube=True)
    assert hits["status"][0] == rr.RAY_HIT and abs(hits["pos"][0][2] - 0.8) < 0.01 and np.allclose(surf["normal"][0], (0, 0, 1), atol=1e-3)
    bare.close()

    slab = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), slab=(0, 16), **KW)
    assert code(rr, lambda: slab.cast_rays(rays)) == -4
    slab.close()
