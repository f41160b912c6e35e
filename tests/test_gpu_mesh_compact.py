"""GPU: the mesh ring's tile-local triangle format (tsdf_mesh_stream_config_compact, TSDF_MESH_INDEX_TILE16) against tests/mesh_compact_reference.py and
against a uint32 ring on the same context, byte for byte: the random volume with zeros, -0, NaN and infinities planted, levels 1 and 2, the checkerboard,
an integrated scene dense and in a sparse pool with every attribute combination, the capacities to the unit, the filter, empty and thin volumes, error
codes and states, and four frames through the lanes beside a twin with a uint32 ring."""
import ctypes as C
import functools

import numpy as np
import pytest

import mesh_compact_reference as MC
import mesh_component_reference as K
import mesh_lod_reference as LOD

pytestmark = pytest.mark.gpu

LIMIT = K.LIMIT
KW = dict(brick_size=[2.0 / 8, 2.2 / 8, 2.0 / 8], limit=LIMIT, view=(64, 36))
BIG = dict(max_vertices=1 << 17, max_triangles=1 << 18, max_surface_tiles=256)
COMPACT = 1


@pytest.fixture(scope="module")
def scene2(rr):
    return rr.scene.make_scene(n_streams=2, width=160, height=120, lut_res=32, inv_res=32)


@functools.lru_cache(maxsize=None)
def planted_volume():
    """test_gpu_mesh_stream.py's random volume: ~10 % exact zeros, and -0, NaN, +-inf planted"""
    rng = np.random.default_rng(20221019)
    vol = rng.uniform(-LIMIT, LIMIT, (19, 22, 20)).astype(np.float32)
    vol[rng.random(vol.shape) < 0.10] = 0.0
    special = np.array([-0.0, np.nan, np.inf, -np.inf], np.float32)
    pick = rng.random(vol.shape) < 0.02
    vol[pick] = special[rng.integers(0, 4, int(pick.sum()))]
    vol.setflags(write=False)
    return vol


@functools.lru_cache(maxsize=None)
def big_volume():
    vol = LOD.random_volume((40, 44, 38))
    vol.setflags(write=False)
    return vol


def context(rr, scene, vol, **kw):
    hip = rr.ReconIntegrationHip(scene, res=vol.shape[::-1], **KW, **kw)
    hip.set_tsdf(vol)
    return hip


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


def both_rings(hip, **cfg):
    """one frame through a uint32 ring and one through a tile-local ring of the same context and configuration"""
    hip.mesh_stream_config(**cfg)
    plain = stream_one(hip)
    hip.mesh_stream_config(index_format=COMPACT, **cfg)
    return plain, stream_one(hip)


def assert_decodes_to(rr, compact, plain, what=""):
    """the compact frame carries the uint32 frame: the same vertices, counts and needs, and codes that decode to its triangles"""
    v, codes, info = compact
    c = info["compact"]
    assert codes.dtype == np.uint16 and codes.shape == plain[1].shape and c["triangles_null"], what
    assert v.dtype == plain[0].dtype and v.tobytes() == plain[0].tobytes(), what
    skip = ("compact", "filter", "bbox_min", "bbox_max")
    assert {k: x for k, x in info.items() if k not in skip} == {k: x for k, x in plain[2].items() if k not in skip}, what
    assert rr.unpack_mesh_triangles(c["table"], codes, c["tiles"]).tobytes() == plain[1].tobytes(), what
    assert MC.decode(c["table"], codes, c["tiles"]).tobytes() == plain[1].tobytes(), what
    assert not (codes >> 15).any() and not ((codes >> 12) == 7).any(), what


def assert_equals_encode(compact, want, what=""):
    table, codes, tiles = want[:3]
    c = compact[2]["compact"]
    assert c["tiles"] == tiles and len(c["table"]) == len(table), what
    assert c["table"].tobytes() == table.tobytes() and compact[1].tobytes() == codes.tobytes(), what


def test_random_volume_every_neighbour_code(rr, scene2):
    vol = planted_volume()
    hip = context(rr, scene2, vol)
    cfg = dict(slots=2, **BIG)
    plain, got = both_rings(hip, **cfg)
    assert hip.mesh_stream_index_format() == COMPACT
    v, codes, info = got
    nv, nt = info["n_vertices"], info["n_triangles"]
    print("random volume:", {k: x for k, x in info.items() if k != "compact"}, "rows", len(info["compact"]["table"]))
    assert nv > 10000 and nt > 10000 and info["needed_tiles"] == 27 and info["vertex_stride"] == 8 and info["overflow"] == 0
    want = MC.encode(LOD.extract_lod(vol, LIMIT, scene2["bbox_min"], scene2["bbox_max"], 0), 0, vol.shape)
    assert_equals_encode(got, want)
    assert sorted(np.unique(codes >> 12)) == list(range(7)) and info["compact"]["tiles"] == (3, 3, 3) and info["compact"]["level"] == 0
    assert_decodes_to(rr, got, plain)
    assert plain[1].tobytes() == hip.extract_mesh(normals=False, colours=False)["triangles"].tobytes()
    rows = len(info["compact"]["table"])
    assert rows == 27 and hip.mesh_stream_stats()["payload_bytes"] == (nv * 8 + 15) // 16 * 16 + rows * 16 + nt * 6 == MC.payload_bytes(nv, 8, rows, nt)
    again = stream_one(hip)                                              # a second frame is identical
    assert again[0].tobytes() == v.tobytes() and again[1].tobytes() == codes.tobytes() and again[2]["compact"]["table"].tobytes() == info["compact"]["table"].tobytes()
    # the C frame itself: the uint32 pointer is NULL, the compact pointers lie behind the vertices
    hip.mesh_stream(3)
    f, ready, m = rr.MeshFrame(), C.c_int32(), rr.MeshCompact()
    lib = rr.load_library()
    assert lib.tsdf_mesh_stream_acquire(hip._c, C.c_int32(1), C.byref(f), C.byref(ready)) == 0 and ready.value == 1
    assert not f.triangles and f.n_triangles == nt and lib.tsdf_mesh_stream_frame_compact(hip._c, C.byref(m)) == 0
    assert m.table - f.vertices == (nv * 8 + 15) // 16 * 16 and C.cast(m.triangles, C.c_void_p).value - m.table == rows * 16 and m.n_tile_rows == rows
    if nv & 1:
        assert bytes((C.c_uint8 * 8).from_address(f.vertices + nv * 8)) == bytes(8)        # the padding is zero
    hip.mesh_stream_release()
    hip.close()


@pytest.mark.parametrize("level", [1, 2])
def test_levels_on_the_odd_volume(rr, scene2, level):
    vol = big_volume()
    hip = context(rr, scene2, vol)
    plain, got = both_rings(hip, slots=2, level=level, **BIG)
    assert got[2]["n_triangles"] > 1000 and hip.mesh_stream_level() == level
    want = MC.encode(LOD.extract_lod(vol, 0.04, scene2["bbox_min"], scene2["bbox_max"], level), level, vol.shape)
    assert_equals_encode(got, want, level)
    assert_decodes_to(rr, got, plain, level)
    assert got[2]["compact"]["tiles"] == MC.tile_grid(vol.shape, level) == ((3, 3, 3) if level == 1 else (2, 2, 2)) and got[2]["compact"]["level"] == level
    hip.close()


def test_checkerboard_the_densest_tile(rr, scene2):
    vol = MC.checkerboard()
    hip = context(rr, scene2, vol)
    plain, got = both_rings(hip, slots=2, **BIG)
    want = MC.encode(LOD.extract_lod(vol, LIMIT, scene2["bbox_min"], scene2["bbox_max"], 0), 0, vol.shape)
    assert_equals_encode(got, want)
    assert_decodes_to(rr, got, plain)
    assert got[2]["compact"]["table"]["n_triangles"][0] == 6144
    hip.close()


@pytest.mark.parametrize("sparse", [False, True])
def test_integrated_scene_every_attribute_combination(rr, small_scene, sparse):
    hip = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), sparse_pool_tiles=64 if sparse else 0, **KW)
    integrate(hip)
    for normals, colours in ((False, False), (True, False), (False, True), (True, True)):
        plain, got = both_rings(hip, normals=normals, colours=colours, **BIG)
        assert got[2]["n_vertices"] > 200 and got[2]["vertex_stride"] == (16 if normals or colours else 8)
        assert_decodes_to(rr, got, plain, (normals, colours))
    hip.close()


def test_capacities_to_the_unit(rr, scene2):
    vol = planted_volume()
    hip = context(rr, scene2, vol)
    hip.mesh_stream_config(slots=2, **BIG)
    plain = stream_one(hip)
    nv, nt, ns = plain[2]["n_vertices"], plain[2]["n_triangles"], plain[2]["needed_tiles"]
    exact = dict(max_vertices=nv, max_triangles=nt, max_surface_tiles=ns)
    hip.mesh_stream_config(index_format=COMPACT, **exact)
    assert_decodes_to(rr, stream_one(hip), plain)
    for key, bit in (("max_vertices", rr.MESH_OVERFLOW_VERTICES), ("max_triangles", rr.MESH_OVERFLOW_TRIANGLES), ("max_surface_tiles", rr.MESH_OVERFLOW_TILES)):
        hip.mesh_stream_config(index_format=COMPACT, **dict(exact, **{key: exact[key] - 1}))
        v, codes, info = stream_one(hip, tag=9)
        assert info["overflow"] == bit and info["tag"] == 9, key
        assert info["n_vertices"] == 0 and info["n_triangles"] == 0 and len(v) == 0 and len(codes) == 0 and len(info["compact"]["table"]) == 0
        assert (info["needed_vertices"], info["needed_triangles"], info["needed_tiles"]) == (nv, nt, ns)
        st = hip.mesh_stream_stats()
        assert st["payload_bytes"] == 0 and st["overflowed"] == 1 and st["frames"] == 1
    hip.mesh_stream_config(index_format=COMPACT, **exact)
    assert_decodes_to(rr, stream_one(hip), plain)
    hip.close()


def test_filter_on_the_speckle_volume(rr, scene2):
    vol = K.speckle_volume()
    hip = context(rr, scene2, vol)
    mesh = LOD.extract_lod(vol, LIMIT, scene2["bbox_min"], scene2["bbox_max"], 0)
    for min_triangles in (100, 1, 100000):
        plain, got = both_rings(hip, slots=2, min_triangles=min_triangles, **BIG)
        info = got[2]
        assert info["filter"] == plain[2]["filter"] and info["overflow"] == 0, min_triangles      # tsdf_mesh_stream_frame_filter still answers
        assert_decodes_to(rr, got, plain, min_triangles)
        want = MC.encode_filtered(mesh, 0, vol.shape, min_triangles)
        assert_equals_encode(got, want, min_triangles)
        rows = len(info["compact"]["table"])
        assert hip.mesh_stream_stats()["payload_bytes"] == MC.payload_bytes(info["n_vertices"], 8, rows, info["n_triangles"])
        if min_triangles == 100:
            assert (info["filter"]["kept"], info["n_vertices"], info["n_triangles"]) == (61, 7958, 15180) and rows < info["needed_tiles"] + 1
        elif min_triangles == 1:
            assert info["filter"]["vertices_removed"] == 0 and rows == info["needed_tiles"]
            assert info["compact"]["table"].tobytes() == MC.encode(mesh, 0, vol.shape)[0].tobytes()
        else:                                                            # above every component: an empty frame, no overflow, nothing copied
            assert (info["n_vertices"], info["n_triangles"], rows, info["filter"]["kept"]) == (0, 0, 0, 0) and hip.mesh_stream_stats()["payload_bytes"] == 0
    hip.close()


def test_filter_with_attributes_and_a_level(rr, scene2):
    vol = K.speckle_volume(res=(39, 43, 37))
    hip = context(rr, scene2, vol)
    plain, got = both_rings(hip, slots=2, level=1, normals=True, min_triangles=100, **BIG)
    assert got[2]["vertex_stride"] == 16 and 0 < got[2]["n_vertices"] < got[2]["needed_vertices"]
    assert_decodes_to(rr, got, plain)
    assert_equals_encode(got, MC.encode_filtered(LOD.extract_lod(vol, LIMIT, scene2["bbox_min"], scene2["bbox_max"], 1), 1, vol.shape, 100))
    hip.close()


def test_empty_and_thin(rr, scene2):
    hip = context(rr, scene2, np.full((19, 22, 20), -LIMIT, np.float32))
    for min_triangles in (0, 100):
        hip.mesh_stream_config(index_format=COMPACT, min_triangles=min_triangles, **BIG)
        v, codes, info = stream_one(hip)
        assert (info["n_vertices"], info["n_triangles"], info["needed_tiles"], info["overflow"]) == (0, 0, 0, 0)
        assert len(v) == 0 and codes.shape == (0, 3) and len(info["compact"]["table"]) == 0 and hip.mesh_stream_stats()["payload_bytes"] == 0
    hip.close()
    ext = [float(x) for x in np.asarray(scene2["bbox_max"]) - np.asarray(scene2["bbox_min"])]
    thin = rr.ReconIntegrationHip(scene2, res=(16, 1, 16), brick_size=[ext[0] / 8, ext[1], ext[2] / 8], limit=LIMIT, view=(64, 36))   # one point thick: no cell
    thin.set_tsdf(np.random.default_rng(3).uniform(-LIMIT, LIMIT, (16, 1, 16)).astype(np.float32))
    for min_triangles in (0, 100):
        thin.mesh_stream_config(index_format=COMPACT, min_triangles=min_triangles, **BIG)
        v, codes, info = stream_one(thin)
        assert (info["n_vertices"], info["n_triangles"], info["overflow"]) == (0, 0, 0) and len(info["compact"]["table"]) == 0
        assert info["compact"]["tiles"] == (2, 1, 2)
    thin.close()


def test_errors_states_and_reconfiguring(rr, scene2, small_scene):
    lib = rr.load_library()
    u = C.c_uint32
    vol = planted_volume()
    hip = context(rr, scene2, vol)
    fmt, out = u(), rr.MeshCompact()
    assert lib.tsdf_mesh_stream_index_format(hip._c, C.byref(fmt)) == -4 and lib.tsdf_mesh_stream_frame_compact(hip._c, C.byref(out)) == -4   # before any config
    assert lib.tsdf_mesh_stream_index_format(hip._c, None) == -1 and lib.tsdf_mesh_stream_frame_compact(hip._c, None) == -1
    caps = (u(1 << 17), u(1 << 18), u(256), u(2))
    assert lib.tsdf_mesh_stream_config_compact(hip._c, u(0), u(0), u(0), u(2), *caps) == -1        # index_format 2
    assert lib.tsdf_mesh_stream_config_compact(hip._c, u(4), u(0), u(0), u(1), *caps) == -1        # the other checks are tsdf_mesh_stream_config_filter's
    assert lib.tsdf_mesh_stream_config_compact(hip._c, u(0), u(3), u(0), u(1), *caps) == -1
    assert lib.tsdf_mesh_stream_config_compact(hip._c, u(0), u(0), u(0), u(1), u(1 << 17), u(1 << 18), u(256), u(1)) == -1
    assert lib.tsdf_mesh_stream_config_compact(hip._c, u(0), u(0), u(0), u(1), u(1), u(715827867), u(1), u(2)) == -1   # a slot of 4 GiB + 2 bytes
    # format 0 through the new entry: byte-identical to tsdf_mesh_stream_config_filter's frames, with a uint32 pointer
    assert lib.tsdf_mesh_stream_config_filter(hip._c, u(0), u(0), u(0), *caps) == 0
    old = stream_one(hip)
    assert lib.tsdf_mesh_stream_config_compact(hip._c, u(0), u(0), u(0), u(0), *caps) == 0
    assert hip.mesh_stream_index_format() == 0
    new = stream_one(hip)
    assert new[1].dtype == np.uint32 and len(new[1]) > 10000 and "compact" not in new[2]
    assert new[0].tobytes() == old[0].tobytes() and new[1].tobytes() == old[1].tobytes()
    hip.mesh_stream(1)
    hip.mesh_stream_acquire()
    assert lib.tsdf_mesh_stream_frame_compact(hip._c, C.byref(out)) == -4                         # a frame is held, but the ring has format 0
    # a reconfiguration needs a drained ring, then works in either direction
    assert code(rr, lambda: hip.mesh_stream_config(index_format=COMPACT, **BIG)) == -4
    hip.mesh_stream_release()
    for index_format in (COMPACT, 0, COMPACT):
        hip.mesh_stream_config(slots=2, index_format=index_format, **BIG)
        assert hip.mesh_stream_index_format() == index_format
        got = stream_one(hip)
        if index_format:
            assert_decodes_to(rr, got, old)
        else:
            assert got[1].tobytes() == old[1].tobytes()
    assert lib.tsdf_mesh_stream_frame_compact(hip._c, C.byref(out)) == -4                         # nothing held
    hip.mesh_stream(2)
    assert lib.tsdf_mesh_stream_frame_compact(hip._c, C.byref(out)) == -4                         # queued, not yet acquired
    hip.mesh_stream_acquire()
    assert lib.tsdf_mesh_stream_frame_compact(hip._c, C.byref(out)) == 0 and lib.tsdf_mesh_stream_frame_compact(hip._c, None) == -1
    hip.mesh_stream_release()
    hip.close()
    slab = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), slab=(0, 16), **KW)
    slab.mesh_stream_config(index_format=COMPACT, **BIG)
    assert code(rr, lambda: slab.mesh_stream(0)) == -4
    slab.close()


def test_four_frames_through_the_lanes_beside_a_uint32_twin(rr):
    """Two scenes alternate through tsdf_frame_dev with stage overlap on.  One context streams compact frames, its twin uint32 frames, both from a 3-slot
    ring picked up two frames late with wait = 0 polls only after the loop: mesh_stream itself is never refused and never waits for a frame."""
    import torch
    mk = dict(n_streams=2, width=160, height=120, lut_res=32, inv_res=32)
    scs = [rr.scene.make_scene(**mk), rr.scene.make_scene(**mk, sphere_c=(0.4, 0.7, -0.3), box_c=(-0.5, 1.5, 0.2))]
    raw = [[torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ("depth", "quality", "silhouette", "color")] for sc in scs]
    torch.cuda.synchronize()
    mv, pr = rr.scene.default_view(64, 36)
    frames, lag = 4, 2

    def run(index_format):
        hip = rr.ReconIntegrationHip(scs[0], res=(32, 32, 32), **KW)
        hip.mesh_stream_config(normals=True, colours=True, slots=3, index_format=index_format, **BIG)
        meshes, fbs = [], []
        for f in range(frames):
            hip.frame_dev(mv, pr, [t.data_ptr() for t in raw[f % 2]])
            hip.mesh_stream(f)                                            # (raises if a slot were missing: nothing waits for a frame)
            if f >= lag:
                meshes.append(hip.mesh_stream_take())
            fbs.append(hip.framebuffer()[0])
        for f in range(frames - lag, frames):
            meshes.append(hip.mesh_stream_take())
        vol = hip.tsdf()
        assert hip.mesh_stream_stats()["frames"] == frames
        hip.close()
        return meshes, fbs, vol

    compact, compact_fb, compact_vol = run(COMPACT)
    plain, plain_fb, plain_vol = run(0)
    assert len(plain[0][0]) > 100 and plain[0][1].tobytes() != plain[1][1].tobytes()     # the two scenes differ
    same = lambda a, b: ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()
    for f in range(frames):
        assert compact[f][2]["tag"] == f and plain[f][2]["tag"] == f
        assert_decodes_to(rr, compact[f], plain[f], f)
        assert same(compact_fb[f], plain_fb[f]), f
    assert same(compact_vol, plain_vol)
