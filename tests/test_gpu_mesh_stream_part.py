"""GPU: mesh streaming on Z-slab contexts (tsdf_mesh_stream_config_part / _frame_part) -- the parts several slab contexts on one device stream, each
against tests/mesh_part_reference.py and their join against the compact ring of a whole-volume context, byte for byte: the crafted volumes of
tests/test_gpu_mesh_slab.py with NaN, infinities, 0 and -0 in every seam's planes, a slab without a vertex, the integrated scene with exchanged and
recomputed halos and in a sparse pool, the capacities to the unit, the one-slab case, errors and states, and the ring's guarantees."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import mesh_compact_reference as MC
import mesh_part_reference as MP
import mesh_slab_reference as S

pytestmark = pytest.mark.gpu

LIMIT = 0.05                                                             # the halo is one tile layer at every resolution used here
KW = dict(brick_size=[2.0 / 8, 2.2 / 8, 2.0 / 8], limit=LIMIT, view=(64, 36))
SEED = 20261019                                                          # tests/test_mesh_part_reference.py checks on the CPU that every seam of every case is crossed
BIG = dict(max_vertices=1 << 18, max_triangles=1 << 19, max_surface_tiles=256)
CRAFTED = [((32, 32, 32), 0, [(0, 16), (16, 32)]),
           ((32, 32, 32), 0, [(0, 8), (8, 16), (16, 24), (24, 32)]),      # the thinnest legal slab: one tile layer, as thick as its halo
           ((20, 12, 28), 0, [(0, 8), (8, 24), (24, 28)]),                 # partial tiles on every axis, a top slab that is not a whole layer
           ((24, 20, 64), 1, [(0, 32), (32, 64)]),
           ((24, 20, 64), 2, [(0, 32), (32, 64)]),
           ((24, 20, 64), 1, [(0, 16), (16, 64)])]


def mgpu():
    return import_module("rgbd-recon_amd.multigpu")


def code(rr, fn):
    with pytest.raises(rr.TsdfError) as e:
        fn()
    return e.value.code


def integrate(hip):
    hip.clearOccupiedBricks()
    hip.markBricks()
    hip.updateOccupiedBricks()
    hip.integrate()


def stream_one(hip, tag=0):
    hip.mesh_stream(tag)
    return hip.mesh_stream_take(wait=True)


def frame_bytes(frame):
    v, codes, info = frame
    return v.tobytes(), info["compact"]["table"].tobytes(), codes.tobytes()


def assert_same_frame(got, want, what=""):
    """vertices, table and codes, byte for byte, and the counts"""
    for name, a, b in zip(("vertices", "table", "codes"), frame_bytes(got), frame_bytes(want)):
        assert a == b, (what, name)
    assert got[0].dtype == want[0].dtype and got[1].dtype == want[1].dtype == np.uint16
    for k in ("n_vertices", "n_triangles", "vertex_stride", "flags", "res"):
        assert got[2][k] == want[2][k], (what, k)
    assert got[2]["compact"]["tiles"] == want[2]["compact"]["tiles"] and got[2]["compact"]["level"] == want[2]["compact"]["level"], what


@pytest.fixture(scope="module")
def scene2(rr):
    return rr.scene.make_scene(n_streams=2, width=160, height=120, lut_res=32, inv_res=32)


def slab_contexts(rr, scene, vol, slabs):
    ctxs = [rr.ReconIntegrationHip(scene, res=vol.shape[::-1], slab=s, **KW) for s in slabs]
    for c in ctxs:
        c.set_tsdf(vol)                                                  # fills the slab's stored layers, halo included
    return ctxs


def whole_and_parts(rr, scene, vol, level, slabs, normals):
    """one frame of the whole-volume context's compact ring, its extract's triangles, and the slab contexts' parts with their join"""
    whole = rr.ReconIntegrationHip(scene, res=vol.shape[::-1], **KW)
    whole.set_tsdf(vol)
    whole.mesh_stream_config(normals=normals, slots=2, level=level, index_format=rr.MESH_INDEX_TILE16, **BIG)
    want = stream_one(whole)
    triangles = whole.extract_mesh(normals=False, colours=False, level=level)["triangles"]
    whole.close()
    ctxs = slab_contexts(rr, scene, vol, slabs)
    for c in ctxs:
        c.mesh_stream_config(normals=normals, slots=2, level=level, part=True, **BIG)
    parts, joined = mgpu().mesh_parts_on_one_device(ctxs, tag=7)
    stats = [c.mesh_stream_stats() for c in ctxs]
    for c in ctxs:
        c.close()
    return want, triangles, parts, joined, stats


@pytest.mark.parametrize("res,level,slabs", CRAFTED)
def test_crafted_volume_parts_equal_the_reference_and_join_to_the_whole_frame(rr, scene2, res, level, slabs):
    vol = S.crafted_volume(res, slabs, SEED, LIMIT)
    ref, ref_parts = MP.parts(vol, LIMIT, scene2["bbox_min"], scene2["bbox_max"], level, slabs)
    want, triangles, parts, joined, stats = whole_and_parts(rr, scene2, vol, level, slabs, normals=False)
    print(res, "level", level, slabs, "whole:", want[2]["n_vertices"], "vertices", want[2]["n_triangles"], "triangles; parts:",
          [(p[2]["n_vertices"], p[2]["n_triangles"], p[2]["needed_tiles"], p[2]["part"]) for p in parts])
    assert want[2]["n_vertices"] > 100 and want[2]["n_triangles"] > 100 and want[2]["overflow"] == 0
    for k, ((v, codes, info), r) in enumerate(zip(parts, ref_parts)):   # each part and the numpy reference
        assert info["overflow"] == 0 and info["tag"] == 7 and info["vertex_stride"] == 8, k
        assert v.dtype == np.uint16 and v.tobytes() == r["vertices"].tobytes(), k
        assert info["compact"]["table"].tobytes() == r["table"].tobytes() and codes.dtype == np.uint16 and codes.tobytes() == r["codes"].tobytes(), k
        assert info["compact"]["tiles"] == r["tiles"] and info["compact"]["level"] == level and info["compact"]["triangles_null"], k
        assert info["part"] == dict(layers=r["layers"], level=level, top=r["top"], seam_tiles=r["seam_tiles"]), k
        assert (info["n_vertices"], info["n_triangles"], info["needed_tiles"]) == (len(r["vertices"]), len(r["codes"]), len(r["table"])), k
        assert (info["needed_vertices"], info["needed_triangles"]) == (info["n_vertices"], info["n_triangles"]), k
        assert stats[k]["payload_bytes"] == MP.payload_bytes(r, 8) and stats[k]["frames"] == 1 and stats[k]["overflowed"] == 0, k
    for r in ref_parts[:-1]:                                              # not vacuous: every seam has codes that name rows of the next part
        assert MP.seam_codes(r) > 0 and r["seam_tiles"] > 0
    assert_same_frame(joined, want)                                       # the join and the whole-volume context's compact ring
    c = joined[2]["compact"]
    assert rr.unpack_mesh_triangles(c["table"], joined[1], c["tiles"]).tobytes() == triangles.tobytes() == ref["triangles"].tobytes()
    assert MC.decode(c["table"], joined[1], c["tiles"]).tobytes() == triangles.tobytes()


@pytest.mark.parametrize("res,level,slabs", [CRAFTED[1], CRAFTED[5]])
def test_crafted_volume_with_normals_joins_to_the_whole_frame(rr, scene2, res, level, slabs):
    vol = S.crafted_volume(res, slabs, SEED, LIMIT)
    want, _, parts, joined, _ = whole_and_parts(rr, scene2, vol, level, slabs, normals=True)
    assert want[2]["vertex_stride"] == 16 and want[2]["n_vertices"] > 100 and all(p[2]["n_vertices"] > 0 for p in parts)
    assert_same_frame(joined, want)


def test_a_slab_without_a_vertex_joins_cleanly(rr, scene2):
    slabs = [(0, 8), (8, 16), (16, 24), (24, 32)]
    vol = S.crafted_volume((32, 32, 32), slabs, SEED, LIMIT)
    vol[16:25] = -LIMIT                                                   # the third slab owns no crossed edge, and no cell of it has one
    want, _, parts, joined, stats = whole_and_parts(rr, scene2, vol, 0, slabs, normals=False)
    info = parts[2][2]
    assert (info["n_vertices"], info["n_triangles"], info["needed_tiles"], info["overflow"]) == (0, 0, 0, 0) and len(info["compact"]["table"]) == 0
    # its seam layer has surface all the same (plane 24 is outside, plane 25 is not: the edges between them are plane 24's), and that is no overflow and
    # no row; the seam layer of the slab below it (planes 16 and 17, both outside) has none
    assert stats[2]["payload_bytes"] == 0 and info["part"]["layers"] == (2, 3) and info["part"]["seam_tiles"] == 16
    assert all(parts[k][2]["n_vertices"] > 0 for k in (0, 1, 3)) and parts[1][2]["part"]["seam_tiles"] == 0
    assert_same_frame(joined, want)


# ---- the integrated scene
@pytest.fixture(scope="module")
def scene_whole(rr, small_scene):
    hip = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), **KW)
    integrate(hip)
    hip.mesh_stream_config(normals=True, colours=True, slots=2, index_format=rr.MESH_INDEX_TILE16, **BIG)
    frame = stream_one(hip)
    hip.close()
    assert frame[2]["n_vertices"] > 200 and frame[2]["n_triangles"] > 200 and frame[2]["vertex_stride"] == 16
    return frame


@pytest.mark.parametrize("halo,sparse", [("exchange", 0), ("recompute", 0), ("recompute", 512)])
def test_small_scene_two_slabs_join_to_the_whole_volume_ring(rr, small_scene, scene_whole, halo, sparse):
    m = mgpu()
    mv, pr = rr.scene.default_view(*KW["view"])
    slabs = [rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), slab=s, recompute_halo=(halo == "recompute"), sparse_pool_tiles=sparse, **KW)
             for s in ((0, 16), (16, 32))]
    m.frame_slabs_on_one_device(slabs, mv, pr, "cuda:0", halo=halo, composite="compact" if sparse else "dense")   # integrates; the halos are current
    for s in slabs:
        s.mesh_stream_config(normals=True, colours=True, slots=2, part=True, **BIG)
    parts, joined = m.mesh_parts_on_one_device(slabs)
    print("small scene,", halo, "sparse" if sparse else "dense", "parts:", [(p[2]["n_vertices"], p[2]["n_triangles"], p[2]["part"]) for p in parts])
    assert parts[0][2]["n_vertices"] > 0 and parts[1][2]["n_vertices"] > 0
    assert ((parts[0][1] >> 14) & 1).any() and parts[0][2]["part"]["seam_tiles"] > 0   # the seam is crossed
    assert_same_frame(joined, scene_whole, (halo, sparse))
    for s in slabs:
        s.close()


# ---- capacities
def test_capacities_to_the_unit(rr, scene2):
    res, slabs = (32, 32, 32), [(0, 16), (16, 32)]
    vol = S.crafted_volume(res, slabs, SEED, LIMIT)
    low = slab_contexts(rr, scene2, vol, slabs[:1])[0]
    low.mesh_stream_config(slots=2, part=True, **BIG)
    v, codes, info = stream_one(low)
    need = dict(max_vertices=info["needed_vertices"], max_triangles=info["needed_triangles"], max_surface_tiles=info["needed_tiles"])
    print("needs of the lower slab:", need, info["part"])
    assert info["part"]["seam_tiles"] > 0 and info["needed_tiles"] == 32  # the seam layer has surface too, and is not counted
    low.mesh_stream_config(slots=2, part=True, **need)                    # need passes, max_surface_tiles = the OWNED surface tiles included
    exact = stream_one(low)
    assert exact[2]["overflow"] == 0 and frame_bytes(exact) == frame_bytes((v, codes, info))
    for bit, key in ((rr.MESH_OVERFLOW_VERTICES, "max_vertices"), (rr.MESH_OVERFLOW_TRIANGLES, "max_triangles"), (rr.MESH_OVERFLOW_TILES, "max_surface_tiles")):
        low.mesh_stream_config(slots=2, part=True, **dict(need, **{key: need[key] - 1}))
        before = low.mesh_stream_stats()["payload_bytes"]
        w, c, i = stream_one(low)
        assert i["overflow"] == bit, key                                  # exactly its bit
        assert (i["n_vertices"], i["n_triangles"], len(w), len(c), len(i["compact"]["table"])) == (0, 0, 0, 0, 0), key
        assert (i["needed_vertices"], i["needed_triangles"], i["needed_tiles"]) == (need["max_vertices"], need["max_triangles"], need["max_surface_tiles"]), key
        st = low.mesh_stream_stats()
        assert st["payload_bytes"] == before == 0 and st["overflowed"] == 1, key
        with pytest.raises(ValueError):
            rr.join_mesh_parts([(w, c, i)])
    low.close()


# ---- the one-slab case
@pytest.mark.parametrize("level", [0, 1, 2])
def test_whole_volume_context_is_the_one_slab_case(rr, scene2, level):
    res = (37, 43, 35)
    vol = S.crafted_volume(res, [(0, 8)], SEED, LIMIT)
    hip = rr.ReconIntegrationHip(scene2, res=res, **KW)
    hip.set_tsdf(vol)
    hip.mesh_stream_config(normals=True, colours=True, slots=2, level=level, index_format=rr.MESH_INDEX_TILE16, **BIG)
    want = stream_one(hip)
    hip.mesh_stream_config(normals=True, colours=True, slots=2, level=level, part=True, **BIG)
    got = stream_one(hip)
    assert want[2]["n_vertices"] > 100 and hip.mesh_stream_index_format() == rr.MESH_INDEX_TILE16 and hip.mesh_stream_level() == level
    assert_same_frame(got, want, level)
    assert {k: x for k, x in got[2].items() if k not in ("compact", "part", "bbox_min", "bbox_max")} == {k: x for k, x in want[2].items() if k not in ("compact", "bbox_min", "bbox_max")}
    tiles = MC.tile_grid(vol.shape, level)
    assert got[2]["part"] == dict(layers=(0, tiles[2]), level=level, top=True, seam_tiles=0)
    assert_same_frame(rr.join_mesh_parts([got]), want, level)
    hip.close()


# ---- errors and states
def test_errors_and_states(rr, scene2):
    lib = rr.load_library()
    res = (24, 20, 64)
    vol = S.crafted_volume(res, [(0, 24)], SEED, LIMIT)
    c = slab_contexts(rr, scene2, vol, [(0, 24)])[0]
    small = dict(max_vertices=1 << 16, max_triangles=1 << 17, max_surface_tiles=64)
    assert code(rr, lambda: c.mesh_stream_config(part=True, level=1, **small)) == -1     # 24 is no multiple of 16 ...
    assert code(rr, lambda: c.mesh_stream_config(part=True, level=2, **small)) == -1     # ... nor of 32: refused at config
    assert code(rr, lambda: c.mesh_stream_config(part=True, level=3, **small)) == -1
    assert code(rr, c.mesh_stream_level) == -4                                           # (a refused config configures nothing)
    c.mesh_stream_config(part=True, level=0, **small)                                    # level 0 always qualifies
    assert code(rr, c.mesh_stream_frame_part) == -4                                      # no frame is held
    c.mesh_stream(1)
    assert code(rr, c.mesh_stream_frame_part) == -4                                      # queued is not held
    got = c.mesh_stream_acquire(wait=True)
    assert got is not None and c.mesh_stream_frame_part() == dict(layers=(0, 3), level=0, top=False, seam_tiles=c.mesh_stream_frame_part()["seam_tiles"])
    assert lib.tsdf_mesh_stream_frame_part(c._c, None) == -1
    c.mesh_stream_release()
    assert code(rr, c.mesh_stream_frame_part) == -4
    # the older config entries keep refusing a slab, each of the four
    for cfg in (dict(), dict(level=1), dict(min_triangles=1), dict(index_format=rr.MESH_INDEX_TILE16)):
        c.mesh_stream_config(**small, **cfg)
        assert code(rr, lambda: c.mesh_stream(0)) == -4, cfg
        assert c.mesh_stream_stats()["frames"] == 0
    # zero capacity, unknown flag, slot count: the checks of the lod entry
    u = C.c_uint32
    assert lib.tsdf_mesh_stream_config_part(c._c, u(0), u(0), u(0), u(1), u(1), u(3)) == -1
    assert lib.tsdf_mesh_stream_config_part(c._c, u(4), u(0), u(1), u(1), u(1), u(3)) == -1
    assert lib.tsdf_mesh_stream_config_part(c._c, u(0), u(0), u(1), u(1), u(1), u(1)) == -1
    with pytest.raises(ValueError):
        c.mesh_stream_config(part=True, min_triangles=2, **small)
    c.close()
    # a ring that is no part ring, with a frame held; and a part ring before the first volume
    whole = rr.ReconIntegrationHip(scene2, res=res, upload=False, **KW)                  # neither calibration nor frame
    whole.mesh_stream_config(part=True, **small)
    assert code(rr, lambda: whole.mesh_stream(0)) == -4                                  # no volume yet
    whole.set_tsdf(vol)
    whole.mesh_stream_config(index_format=rr.MESH_INDEX_TILE16, **small)
    whole.mesh_stream(0)
    assert whole.mesh_stream_acquire(wait=True) is not None and code(rr, whole.mesh_stream_frame_part) == -4
    whole.mesh_stream_release()
    whole.mesh_stream_config(part=True, colours=True, **small)
    assert code(rr, lambda: whole.mesh_stream(0)) == -4                                  # colours without calibration and a frame
    whole.close()


# ---- the ring's guarantees
def test_four_frames_through_a_three_slot_ring_allocate_once_and_repeat(rr, scene2):
    res, slabs = (20, 12, 28), [(0, 8), (8, 24), (24, 28)]
    vol = S.crafted_volume(res, slabs, SEED, LIMIT)
    _, ref_parts = MP.parts(vol, LIMIT, scene2["bbox_min"], scene2["bbox_max"], 0, slabs)
    runs = []
    for _ in range(2):
        ctxs = slab_contexts(rr, scene2, vol, slabs)
        frames = []
        for c in ctxs:
            c.mesh_stream_config(slots=3, part=True, **BIG)
            assert c.mesh_stream_stats()["device_bytes"] == 0
        device_bytes = None
        for f in range(4):                                                # acquire two frames late: with three slots no call waits
            for c in ctxs:
                c.mesh_stream(f)
            now = [c.mesh_stream_stats()["device_bytes"] for c in ctxs]
            device_bytes = device_bytes or now
            assert now == device_bytes and min(now) > 0                   # nothing is allocated after the first call
            if f >= 2:
                frames.append([c.mesh_stream_take(wait=True) for c in ctxs])
        frames += [[c.mesh_stream_take(wait=True) for c in ctxs] for _ in range(2)]
        assert [[p[2]["tag"] for p in fr] for fr in frames] == [[f] * 3 for f in range(4)]
        for k, c in enumerate(ctxs):
            st = c.mesh_stream_stats()
            assert st["frames"] == 4 and st["overflowed"] == 0 and st["device_bytes"] == device_bytes[k]
            assert st["payload_bytes"] == 4 * MP.payload_bytes(ref_parts[k], 8)   # the parts' compact sizes
            c.close()
        runs.append([[frame_bytes(p) for p in fr] for fr in frames])
        assert all(fr == runs[-1][0] for fr in runs[-1])                  # the volume does not change: four identical frames
    assert runs[0] == runs[1]                                             # two runs give identical bytes
