"""GPU: ray queries on Z-slab contexts (tsdf_cast_rays_part / _dev, tsdf_merge_ray_parts_dev) -- every slab casts the same rays, the merged parts against
the whole-volume context's tsdf_cast_rays and tests/ray_part_reference.py, byte for byte: crafted volumes with NaN, infinities, 0 and -0 in every seam's
planes (every single part against the reference's part as well); the integrated scene with exchanged and recomputed halos and in a sparse pool, normals
and colours, world and unit-cube rays, with empty space skipped; the one-slab case; the device forms on one stream without a host wait; more rays than
one launch takes; part stats; two runs; every error code."""
from importlib import import_module

import numpy as np
import pytest

import main_path_reference as R
import mesh_reference as M
import mesh_slab_reference as S
import ray_part_reference as P
import ray_reference as Q
from test_gpu_rays import assert_same, code, integrate, ray_mix
from test_ray_part_reference import CASES, LIMIT, SEED, case

pytestmark = pytest.mark.gpu

KW = dict(brick_size=[2.0 / 8, 2.2 / 8, 2.0 / 8], limit=LIMIT, view=(64, 36))
f32 = np.float32


def mgpu():
    return import_module("rgbd-recon_amd.multigpu")


@pytest.fixture(scope="module")
def scene2(rr):
    return rr.scene.make_scene(n_streams=2, width=160, height=120, lut_res=32, inv_res=32)


def slab_contexts(rr, scene, res, slabs, vol):
    ctxs = [rr.ReconIntegrationHip(scene, res=res, slab=s, **KW) for s in slabs]
    for c in ctxs:
        c.set_tsdf(vol)                                                  # fills the slab's stored layers, halo included
    return ctxs


def close(ctxs):
    for c in ctxs:
        c.close()


# ---------------------------------------------------------------------------------------------------------------- crafted volumes
@pytest.mark.parametrize("res,slabs", CASES)
def test_crafted_volume_parts_merge_byte_for_byte(rr, scene2, res, slabs):
    vol, rays, T = case(res, slabs)
    lo, hi = scene2["bbox_min"], scene2["bbox_max"]
    ref, ref_parts = P.whole(T), P.parts(T, slabs)
    ref_surf = Q.surface(vol, scene2, LIMIT, lo, hi, ref, normals=True, colours=False)
    whole = rr.ReconIntegrationHip(scene2, res=res, **KW)
    whole.set_tsdf(vol)
    w_hits, w_surf = whole.cast_rays(rays, normals=True, unit_cube=True)
    whole.close()
    ctxs = slab_contexts(rr, scene2, res, slabs, vol)
    got = mgpu().rays_slabs_on_one_device(ctxs, rays, normals=True, unit_cube=True)
    close(ctxs)
    n_hits, n_surf = rr.merge_ray_parts(got["parts"])
    print(res, slabs, len(rays), "rays,", int((ref["hits"]["status"] & 1).sum()), "hits; part stats", got["stats"])
    # the device merge, the numpy merge, tsdf_cast_rays on the whole context and the reference: four times the same bytes
    assert_same(w_hits, ref["hits"], "whole context against the reference: hits")
    assert_same(w_surf, ref_surf, "whole context against the reference: surface")
    assert_same(got["hits"], w_hits, "device merge against the whole context: hits")
    assert_same(got["surface"], w_surf, "device merge against the whole context: surface")
    assert_same(n_hits, got["hits"], "numpy merge against the device merge: hits")
    assert_same(n_surf, got["surface"], "numpy merge against the device merge: surface")
    for k, p in enumerate(ref_parts):                                    # ... and every single part is the reference's part
        assert_same(got["parts"][k][0], p["hits"], f"part {k} hits")
        assert_same(got["parts"][k][1], P.part_surface(vol, scene2, LIMIT, lo, hi, p, slabs[k], colours=False), f"part {k} surface")
        assert got["stats"][k]["rays"] == len(rays) and got["stats"][k]["hits"] == int((p["hits"]["status"] & 1).sum()), k   # hits found in THIS part
        assert got["stats"][k]["fetched"] == got["stats"][k]["samples"]  # an uploaded volume: every class is kTileMixed, nothing may be skipped


# ---------------------------------------------------------------------------------------------------------------- the integrated scene
@pytest.fixture(scope="module")
def scene_whole(rr, small_scene):
    """the whole-volume context's answers to the world and the unit-cube rays, normals and colours"""
    hip = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), **KW)
    integrate(hip)
    vol = hip.tsdf()
    inside = R.voxel_positions((32, 32, 32))[np.nan_to_num(vol, nan=-1.0) > 0]
    out = {}
    for world in (True, False):
        rays = ray_mix(21 + world, 2000, inside, small_scene["bbox_min"], small_scene["bbox_max"], world)
        hits, surf = hip.cast_rays(rays, normals=True, colours=True, unit_cube=not world)
        assert ((hits["status"] & 1) != 0).sum() > 300 and surf["rgba"].any() and surf["normal"].any()
        out[world] = (rays, hits, surf)
    hip.close()
    return out


@pytest.mark.parametrize("n_slabs,halo,sparse", [(2, "exchange", 0), (4, "exchange", 0), (2, "recompute", 0), (4, "recompute", 0), (2, "recompute", 512)])
def test_small_scene_slabs_equal_the_whole_volume(rr, small_scene, scene_whole, n_slabs, halo, sparse):
    m = mgpu()
    mv, pr = rr.scene.default_view(*KW["view"])
    ranges = [m.slab_range(32, k, n_slabs) for k in range(n_slabs)]
    slabs = [rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), slab=s, recompute_halo=(halo == "recompute"), sparse_pool_tiles=sparse, **KW) for s in ranges]
    m.frame_slabs_on_one_device(slabs, mv, pr, "cuda:0", halo=halo, composite="compact" if sparse else "dense")   # integrates; the halos are current
    skipped = 0
    for world in (True, False):
        rays, hits, surf = scene_whole[world]
        got = m.rays_slabs_on_one_device(slabs, rays, normals=True, colours=True, unit_cube=not world)
        print(n_slabs, "slabs,", halo, "sparse" if sparse else "dense", "world" if world else "unit cube", got["stats"])
        assert_same(got["hits"], hits, "hits")
        assert_same(got["surface"], surf, "normals and colours")
        assert sum(((p[0]["status"] & 1) != 0).sum() > 0 for p in got["parts"]) >= 2    # more than one slab finds hits
        for s in got["stats"]:
            assert s["fetched"] <= s["samples"]
            skipped += s["samples"] - s["fetched"]
    assert skipped > 0                                                    # skipping happened (fetched < samples in a part's stats) and changed nothing
    close(slabs)


# ---------------------------------------------------------------------------------------------------------------- the one-slab case
def test_whole_volume_context_is_the_one_slab_case(rr, small_scene, scene2):
    res = (37, 43, 35)
    vol = S.crafted_volume(res, [(0, 35)], SEED, LIMIT)
    hip = rr.ReconIntegrationHip(scene2, res=res, **KW)
    hip.set_tsdf(vol)
    inside = R.voxel_positions(res)[np.nan_to_num(vol, nan=-1.0) > 0]
    rays = ray_mix(3, 2000, inside, scene2["bbox_min"], scene2["bbox_max"], True)
    want = hip.cast_rays(rays, normals=True, colours=True)
    stats = hip.ray_stats()
    got = hip.cast_rays_part(rays, normals=True, colours=True)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert hip.ray_stats() == stats                                      # it owns every sample
    assert hip.cast_rays_part(rays).tobytes() == want[0].tobytes()       # no surface array at all
    hip.close()
    hip = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), sparse_pool_tiles=512, **KW)      # ... integrated, in a sparse pool, with skipping
    integrate(hip)
    want = hip.cast_rays(rays, normals=True, colours=True)
    stats = hip.ray_stats()
    got = hip.cast_rays_part(rays, normals=True, colours=True)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert hip.ray_stats() == stats and stats["fetched"] < stats["samples"]
    hip.close()


# ---------------------------------------------------------------------------------------------------------------- the device forms
def test_device_forms_on_one_stream_without_a_host_wait(rr, scene2):
    """cast, gather copy and merge are queued on ONE torch stream the contexts adopt; the host waits once, at the end"""
    import torch
    res, slabs = CASES[2]
    vol, rays, T = case(res, slabs)
    n, world = len(rays), len(slabs)
    ctxs = slab_contexts(rr, scene2, res, slabs, vol)
    u8 = dict(dtype=torch.uint8, device="cuda")
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(n, 32).copy()).cuda()
    own = [(torch.zeros((n, 32), **u8), torch.zeros((n, 32), **u8)) for _ in ctxs]             # each slab's own result arrays
    stride = n + 7                                                        # the gathered parts lie further apart than they are long
    hit_parts, surf_parts = torch.zeros((world, stride, 32), **u8), torch.zeros((world, stride, 32), **u8)
    hits, surf = torch.zeros((n, 32), **u8), torch.zeros((n, 32), **u8)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    for c in ctxs:
        c.set_stream(st.cuda_stream)
    with torch.cuda.stream(st):                                           # no host wait inside
        for k, c in enumerate(ctxs):
            c.cast_rays_part_dev(d_rays.data_ptr(), n, own[k][0].data_ptr(), own[k][1].data_ptr(), normals=True, unit_cube=True)
            hit_parts[k, :n].copy_(own[k][0], non_blocking=True)
            surf_parts[k, :n].copy_(own[k][1], non_blocking=True)
        ctxs[-1].merge_ray_parts_dev(hit_parts.data_ptr(), surf_parts.data_ptr(), world, n, stride, hits.data_ptr(), surf.data_ptr())   # any context merges
    st.synchronize()
    ref = P.whole(T)
    assert_same(hits.cpu().numpy().reshape(-1).view(rr.RAY_HIT_DTYPE), ref["hits"], "hits")
    assert_same(surf.cpu().numpy().reshape(-1).view(rr.RAY_SURFACE_DTYPE),
                Q.surface(vol, scene2, LIMIT, scene2["bbox_min"], scene2["bbox_max"], ref, normals=True, colours=False), "surface")
    for c in ctxs:
        c.set_stream(None)
    close(ctxs)


def test_more_rays_than_one_launch(rr, scene2):
    """kRayChunk + 300 rays on the crafted 32^3 volume: merged parts against the whole context's cast, device against device"""
    import torch
    res, slabs = CASES[0]
    vol, rays, _ = case(res, slabs)
    n = (1 << 18) + 300
    rays = np.ascontiguousarray(np.resize(rays, n))
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(n, 32).copy()).cuda()
    want = torch.zeros((2, n, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    whole = rr.ReconIntegrationHip(scene2, res=res, **KW)
    whole.set_tsdf(vol)
    whole.cast_rays_dev(d_rays.data_ptr(), n, want[0].data_ptr(), want[1].data_ptr(), normals=True, unit_cube=True)
    whole.sync()
    whole.close()
    ctxs = slab_contexts(rr, scene2, res, slabs, vol)
    got = mgpu().rays_slabs_on_one_device(ctxs, rays, normals=True, unit_cube=True)
    close(ctxs)
    want = want.cpu().numpy()
    assert ((want[0].reshape(-1).view(rr.RAY_HIT_DTYPE)["status"][1 << 18:] & 1) != 0).sum() > 50      # the second launch has hits
    assert_same(got["hits"], want[0].reshape(-1).view(rr.RAY_HIT_DTYPE), "hits")
    assert_same(got["surface"], want[1].reshape(-1).view(rr.RAY_SURFACE_DTYPE), "surface")
    assert [s["rays"] for s in got["stats"]] == [n] * len(slabs)


def test_two_runs_give_identical_bytes(rr, scene2):
    res, slabs = CASES[1]
    vol, rays, _ = case(res, slabs)
    ctxs = slab_contexts(rr, scene2, res, slabs, vol)
    runs = [mgpu().rays_slabs_on_one_device(ctxs, rays, normals=True, colours=True, unit_cube=True) for _ in range(2)]
    close(ctxs)
    assert runs[0]["hits"].tobytes() == runs[1]["hits"].tobytes() and runs[0]["surface"].tobytes() == runs[1]["surface"].tobytes()
    for a, b in zip(runs[0]["parts"], runs[1]["parts"]):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert runs[0]["stats"] == runs[1]["stats"]


# ---------------------------------------------------------------------------------------------------------------- errors
def test_error_codes(rr, small_scene):
    import ctypes as C
    import torch
    rays = Q.make_rays([(0.5, 0.5, 1.5)], [(0.0, 0.0, -1.0)])
    slab = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), slab=(0, 16), **KW)
    lib, c = slab._L, slab._c
    assert code(rr, lambda: slab.cast_rays_part(rays)) == -4             # before the first integrate / upload_volume
    buf = torch.zeros((4, 2, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = [buf[k].data_ptr() for k in range(4)]
    assert code(rr, lambda: slab.cast_rays_part_dev(p[0], 1, p[1])) == -4
    merge = lambda hp, sp, parts, n, stride, h, s: lib.tsdf_merge_ray_parts_dev(c, C.c_void_p(hp), C.c_void_p(sp), C.c_uint32(parts), C.c_uint64(n), C.c_uint64(stride),
                                                                                C.c_void_p(h), C.c_void_p(s))
    assert merge(p[0], None, 2, 1, 1, p[2], None) == 0                   # the merge needs no volume
    assert merge(p[0], p[1], 1, 1, 1, p[2], p[3]) == 0
    assert merge(p[0], None, 0, 1, 1, p[2], None) == -1                  # parts == 0
    assert merge(None, None, 0, 0, 0, None, None) == -1
    assert merge(None, None, 2, 1, 1, p[2], None) == -1                  # an array is NULL while n > 0
    assert merge(p[0], None, 2, 1, 1, None, None) == -1
    assert merge(p[0], p[1], 2, 1, 1, p[2], None) == -1                  # exactly one of the two surface arrays
    assert merge(p[0], None, 2, 1, 1, p[2], p[3]) == -1
    assert merge(p[0], None, 2, 2, 1, p[2], None) == -1                  # stride_records < n
    assert merge(None, None, 3, 0, 0, None, None) == 0                   # n == 0: TSDF_OK, nothing launched
    assert lib.tsdf_merge_ray_parts_dev(None, C.c_void_p(p[0]), None, C.c_uint32(1), C.c_uint64(1), C.c_uint64(1), C.c_void_p(p[2]), None) == -1
    integrate(slab)
    assert slab.cast_rays_part(rays, unit_cube=True).shape == (1,)
    with pytest.raises(rr.TsdfError) as e:                               # the whole cast keeps refusing, and says where to go
        slab.cast_rays(rays)
    assert e.value.code == -4 and "tsdf_cast_rays_part" in str(e.value)
    ray, hit, surf = rr.Ray(), rr.RayHit(), rr.RaySurface()
    cast = lambda r, n, flags, h, s: lib.tsdf_cast_rays_part(c, r, C.c_uint64(n), C.c_uint32(flags), h, s)
    cast_dev = lambda r, n, flags, h, s: lib.tsdf_cast_rays_part_dev(c, r, C.c_uint64(n), C.c_uint32(flags), h, s)
    for fn in (cast, cast_dev):
        assert fn(C.byref(ray), 1, 8, C.byref(hit), None) == -1         # an unknown flag
        assert fn(None, 0, 8, None, None) == -1                         # ... with nothing to cast as well
        assert fn(None, 1, 0, C.byref(hit), None) == -1                 # NULL arrays with n > 0
        assert fn(C.byref(ray), 1, 0, None, None) == -1
        assert fn(C.byref(ray), 1, rr.RAY_NORMALS, C.byref(hit), None) == -1      # surface is NULL exactly when neither attribute flag is set
        assert fn(C.byref(ray), 1, 0, C.byref(hit), C.byref(surf)) == -1
        assert fn(None, 0, 0, None, None) == 0                          # n == 0: TSDF_OK, nothing launched
    assert slab.ray_stats() == dict(rays=0, hits=0, samples=0, fetched=0)
    assert lib.tsdf_cast_rays_part(None, C.byref(ray), C.c_uint64(1), C.c_uint32(0), C.byref(hit), None) == -1
    slab.close()

    bare = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), slab=(16, 32), upload=False, **KW)   # a volume, but neither calibration nor frame
    bare.set_tsdf(M.sphere_volume((32, 32, 32), limit=LIMIT))
    assert code(rr, lambda: bare.cast_rays_part(rays, colours=True, unit_cube=True)) == -4
    hits, surf = bare.cast_rays_part(rays, normals=True, unit_cube=True)
    assert hits["status"][0] == rr.RAY_HIT and abs(hits["pos"][0][2] - 0.8) < 0.01 and np.allclose(surf["normal"][0], (0, 0, 1), atol=1e-3)
    bare.close()
