"""GPU: the mesh level of detail (tsdf_mesh_extract_lod, tsdf_mesh_stream_config_lod) against tests/mesh_lod_reference.py, bit for bit: a random
volume whose lattices are padded on every axis at every level, with zeros, -0, NaN and infinities planted; a sphere that must stay a closed 2-manifold;
an integrated scene, culled and in a sparse pool, whose class skip works on lattice tiles; normals and colours; the ring at a level -- every flag
combination, the overflow of the lattice-tile capacity, four moving frames through the lanes, a reconfiguration between levels --; errors."""
import ctypes as C

import numpy as np
import pytest

import mesh_lod_reference as L
import mesh_pack_reference as P
import mesh_reference as M

pytestmark = pytest.mark.gpu

LIMIT = 0.04
KW = dict(brick_size=[2.0 / 8, 2.2 / 8, 2.0 / 8], limit=LIMIT, view=(64, 36))
BIG = dict(max_vertices=1 << 18, max_triangles=1 << 19, max_surface_tiles=256)
RANDOM_RES = (37, 43, 35)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def nan_equal(a, b):
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def assert_identical(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def assert_equals_reference(got, want):
    assert got["position"].shape == want["position"].shape and got["triangles"].shape == want["triangles"].shape
    assert got["position"].tobytes() == want["position"].tobytes()
    assert got["triangles"].dtype == np.uint32 and got["triangles"].tobytes() == want["triangles"].tobytes()


def integrate(hip):
    hip.clearOccupiedBricks()
    hip.markBricks()
    hip.updateOccupiedBricks()
    hip.integrate()


def code(rr, fn):
    with pytest.raises(rr.TsdfError) as e:
        fn()
    return e.value.code


def stream_one(hip, tag=0):
    hip.mesh_stream(tag)
    return hip.mesh_stream_take(wait=True)


@pytest.fixture(scope="module")
def scene2(rr):
    return rr.scene.make_scene(n_streams=2, width=160, height=120, lut_res=32, inv_res=32)


@pytest.fixture(scope="module")
def random_case(scene2):
    """the 37 x 43 x 35 volume and its reference at the three levels, computed once"""
    vol = L.random_volume(RANDOM_RES, limit=LIMIT)
    return vol, [L.extract_lod(vol, LIMIT, scene2["bbox_min"], scene2["bbox_max"], level) for level in range(3)]


@pytest.mark.parametrize("level", [0, 1, 2])
def test_random_volume_bit_equal_and_reproducible(rr, scene2, random_case, level):
    """lattices 37 x 43 x 35, 19 x 22 x 18 and 10 x 11 x 9: padded tiles and tile borders on every axis at every level"""
    vol, wants = random_case
    want = wants[level]
    hip = rr.ReconIntegrationHip(scene2, res=RANDOM_RES, **KW)
    hip.set_tsdf(vol)
    nv, nt = C.c_uint64(), C.c_uint64()
    assert rr.load_library().tsdf_mesh_extract_lod(hip._c, C.c_uint32(0), C.c_uint32(level), C.byref(nv), C.byref(nt)) == 0    # the entry itself, level 0 too
    print("level", level, nv.value, "vertices", nt.value, "triangles; reference", len(want["position"]), len(want["triangles"]))
    assert (nv.value, nt.value) == (len(want["position"]), len(want["triangles"])) and nv.value > 1000 and nt.value > 1000
    hip._mesh_counts = (nv.value, nt.value)
    got = hip.download_mesh(normals=False, colours=False)
    assert_equals_reference(got, want)
    st = hip.mesh_stats()
    assert st["tiles"] == want["tiles"] == (150, 27, 8)[level] and st["tiles_skipped"] == 0 and st["tiles_with_surface"] == want["tiles_with_surface"]
    assert st["bytes"] == got["position"].nbytes + got["triangles"].nbytes
    assert_identical(hip.extract_mesh(normals=False, colours=False, level=level), got)      # through the binding, and a second extract
    if level == 0:
        assert_identical(hip.extract_mesh(normals=False, colours=False), got)               # tsdf_mesh_extract
    hip.close()


@pytest.mark.parametrize("level", [1, 2])
def test_sphere_is_a_closed_manifold(rr, scene2, level):
    res = (48, 40, 40)
    vol = M.sphere_volume(res, limit=LIMIT)
    hip = rr.ReconIntegrationHip(scene2, res=res, **KW)
    hip.set_tsdf(vol)
    got = hip.extract_mesh(normals=False, colours=False, level=level)
    hip.close()
    rep = M.manifold_report(got["triangles"], len(got["position"]))
    print("sphere level", level, rep)
    assert rep["faces"] > 500 and rep["vertices_used"] == len(got["position"])
    assert rep["directed_unique"] and rep["edges_shared_by_two"] and rep["opposite"]
    assert rep["euler"] == 2
    assert M.signed_volume(got["position"], got["triangles"]) > 0
    assert_equals_reference(got, L.extract_lod(vol, LIMIT, scene2["bbox_min"], scene2["bbox_max"], level))


@pytest.fixture(scope="module")
def scene_mesh(rr, small_scene):
    """small_scene at 64^3, bricks on, after integrate: the dense context's meshes at levels 1 and 2 (level 1 with every attribute), their stats, the
    volume and the references"""
    from oracle.oracle import OracleRecon
    kw = dict(res=(64, 64, 64), **KW)
    orc = OracleRecon(small_scene, **kw)
    integrate(orc)
    # on the CPU first: the scene leaves lattice tiles of level 1 whose 27 storage tiles hold the clear value only -- what a class skip can take
    empty = L.empty_lattice_tiles(orc.tsdf(), LIMIT, 1)
    print("oracle volume: lattice tiles of level 1 with nothing but -limit in reach:", empty)
    assert empty >= 1
    hip = rr.ReconIntegrationHip(small_scene, **kw)
    integrate(hip)
    got = {1: hip.extract_mesh(normals=True, colours=True, level=1)}
    stats = {1: hip.mesh_stats()}
    got[2] = hip.extract_mesh(normals=False, colours=False, level=2)
    stats[2] = hip.mesh_stats()
    vol = hip.tsdf()
    hip.close()
    want = {level: L.extract_lod(vol, LIMIT, small_scene["bbox_min"], small_scene["bbox_max"], level) for level in (1, 2)}
    return dict(got=got, stats=stats, vol=vol, want=want, empty=empty)


@pytest.mark.parametrize("level", [1, 2])
def test_small_scene_culled_equals_the_unskipped_reference(scene_mesh, level):
    got, want, st = scene_mesh["got"][level], scene_mesh["want"][level], scene_mesh["stats"][level]
    print("small scene level", level, len(got["position"]), "vertices", len(got["triangles"]), "triangles", st)
    assert len(want["position"]) > (200, 50)[level - 1] and len(want["triangles"]) > (200, 50)[level - 1]
    assert_equals_reference(got, want)
    assert st["tiles"] == (64, 8)[level - 1] and st["tiles_with_surface"] == want["tiles_with_surface"]
    assert st["tiles_with_surface"] <= st["tiles"] - st["tiles_skipped"]
    if level == 1:
        assert 0 < st["tiles_skipped"] <= scene_mesh["empty"]


def test_small_scene_sparse_pool_identical_to_dense(rr, small_scene, scene_mesh):
    hip = rr.ReconIntegrationHip(small_scene, res=(64, 64, 64), sparse_pool_tiles=512, **KW)
    integrate(hip)
    got1 = hip.extract_mesh(normals=True, colours=True, level=1)
    st1 = hip.mesh_stats()
    got2 = hip.extract_mesh(normals=False, colours=False, level=2)
    hip.close()
    assert st1["tiles_skipped"] > 0
    assert_identical(got1, scene_mesh["got"][1])
    assert_identical(got2, scene_mesh["got"][2])


def test_normals_and_colours_equal_the_reference(small_scene, scene_mesh):
    """Level 1.  Bit equality, NaN equal to NaN, as tests/test_gpu_mesh.py has it for level 0: the attributes are the full-resolution gradient and
    blendColors at the vertex's unit-cube position, through the same device functions as a frame pixel."""
    got, want, vol = scene_mesh["got"][1], scene_mesh["want"][1], scene_mesh["vol"]
    n = M.normals(vol, LIMIT, small_scene["bbox_min"], small_scene["bbox_max"], want["unit"])
    c = M.colours(small_scene, LIMIT, want["unit"])
    ok_n, ok_c = nan_equal(got["normal"], n), nan_equal(got["colour"], c)
    with np.errstate(invalid="ignore"):
        print("normals: differing", int((~ok_n).sum()), "of", ok_n.size, "NaN", int(np.isnan(n).sum()), "max abs diff", float(np.nanmax(np.abs(got["normal"] - n))) if n.size else 0.0)
        print("colours: differing", int((~ok_c).sum()), "of", ok_c.size, "NaN", int(np.isnan(c).sum()), "valid", int((c[:, 3] > 0).sum()),
              "max abs diff", float(np.nanmax(np.abs(got["colour"] - c))) if c.size else 0.0)
    assert (c[:, 3] > 0).sum() > 100                                     # the scene does colour the surface
    finite = np.isfinite(n).all(axis=1)
    assert finite.sum() > 100 and np.allclose(np.linalg.norm(n[finite], axis=1), 1.0, atol=1e-5)
    assert ok_n.all()
    assert ok_c.all()


# ---- streaming
def pack_extract(hip, scene, normals, colours, level):
    """the packing of this context's own extract at the level: unit-cube positions from the numpy extraction of its volume (whose world positions must be
    the device's bit for bit), normals and colours the device's arrays"""
    got = hip.extract_mesh(normals=normals, colours=colours, level=level)
    want = L.extract_lod(hip.tsdf(), LIMIT, scene["bbox_min"], scene["bbox_max"], level)
    assert got["position"].tobytes() == want["position"].tobytes() and got["triangles"].tobytes() == want["triangles"].tobytes()
    return P.pack(want["unit"], got.get("normal"), got.get("colour")), got["triangles"]


@pytest.mark.parametrize("level", [1, 2])
def test_random_volume_streamed_byte_equal(rr, scene2, random_case, level):
    vol, wants = random_case
    want = wants[level]
    want_v, want_t = P.pack(want["unit"]), want["triangles"]
    nv, nt = len(want_v), len(want_t)
    hip = rr.ReconIntegrationHip(scene2, res=RANDOM_RES, **KW)
    hip.set_tsdf(vol)
    hip.mesh_stream_config(slots=2, level=level, **BIG)
    assert hip.mesh_stream_level() == level
    v, t, info = stream_one(hip, tag=5)
    print("random volume level", level, info)
    assert info["overflow"] == 0 and info["vertex_stride"] == 8 and info["flags"] == 0 and info["tag"] == 5 and info["res"] == RANDOM_RES
    assert (info["n_vertices"], info["n_triangles"], info["needed_vertices"], info["needed_triangles"], info["needed_tiles"]) == (nv, nt, nv, nt, want["tiles_with_surface"])
    assert v.dtype == np.uint16 and v.shape == (nv, 4) and v.tobytes() == want_v.tobytes()
    assert t.dtype == np.uint32 and t.tobytes() == want_t.tobytes()
    assert hip.mesh_stream_stats()["payload_bytes"] == nv * 8 + nt * 12                     # payload bytes to the byte
    v2, t2, _ = stream_one(hip)
    assert v2.tobytes() == v.tobytes() and t2.tobytes() == t.tobytes()
    hip.close()


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("sparse", [False, True])
def test_small_scene_streamed_every_attribute_combination(rr, small_scene, sparse, level):
    hip = rr.ReconIntegrationHip(small_scene, res=(64, 64, 64), sparse_pool_tiles=512 if sparse else 0, **KW)
    integrate(hip)
    want_v, want_t = pack_extract(hip, small_scene, True, True, level)
    nv, nt = len(want_v), len(want_t)
    assert nv > 50 and (want_v[:, 15] == 255).sum() > 20
    for normals, colours in ((True, True), (True, False), (False, True)):
        hip.mesh_stream_config(normals=normals, colours=colours, level=level, **BIG)
        before = hip.mesh_stream_stats()["payload_bytes"]
        v, t, info = stream_one(hip)
        assert info["vertex_stride"] == 16 and info["overflow"] == 0 and info["flags"] == (1 if normals else 0) | (2 if colours else 0)
        assert v.dtype == np.uint8 and v.shape == want_v.shape and t.tobytes() == want_t.tobytes()
        assert v[:, :8].tobytes() == want_v[:, :8].tobytes()
        assert v[:, 8:12].tobytes() == (want_v[:, 8:12].tobytes() if normals else bytes(4 * len(v)))
        assert v[:, 12:].tobytes() == (want_v[:, 12:].tobytes() if colours else bytes(4 * len(v)))
        assert hip.mesh_stream_stats()["payload_bytes"] - before == nv * 16 + nt * 12
    hip.mesh_stream_config(level=level, **BIG)                           # positions alone: stride 8, the same codes
    v, t, info = stream_one(hip)
    assert info["vertex_stride"] == 8 and v.tobytes() == np.ascontiguousarray(want_v[:, :8]).tobytes() and t.tobytes() == want_t.tobytes()
    assert hip.mesh_stream_stats()["payload_bytes"] == nv * 8 + nt * 12
    hip.close()


@pytest.mark.parametrize("level", [1, 2])
def test_overflow_of_the_lattice_tile_capacity(rr, small_scene, level):
    hip = rr.ReconIntegrationHip(small_scene, res=(64, 64, 64), **KW)
    integrate(hip)
    want_v, want_t = pack_extract(hip, small_scene, True, False, level)
    nv, nt, ns = len(want_v), len(want_t), hip.mesh_stats()["tiles_with_surface"]
    assert ns >= 2
    exact = dict(max_vertices=nv, max_triangles=nt, max_surface_tiles=ns)
    hip.mesh_stream_config(normals=True, level=level, **exact)
    v, t, info = stream_one(hip)
    assert info["overflow"] == 0 and v.tobytes() == want_v.tobytes() and t.tobytes() == want_t.tobytes()
    hip.mesh_stream_config(normals=True, level=level, **dict(exact, max_surface_tiles=ns - 1))
    v, t, info = stream_one(hip, tag=9)
    assert info["overflow"] == rr.MESH_OVERFLOW_TILES == 4 and info["tag"] == 9
    assert info["n_vertices"] == 0 and info["n_triangles"] == 0 and len(v) == 0 and len(t) == 0
    assert (info["needed_vertices"], info["needed_triangles"], info["needed_tiles"]) == (nv, nt, ns)
    st = hip.mesh_stream_stats()
    assert st["payload_bytes"] == 0 and st["overflowed"] == 1 and st["frames"] == 1
    hip.close()


@pytest.mark.parametrize("level", [1, 2])
def test_moving_frames_through_the_lanes(rr, level):
    """Two scenes alternate for 4 frames through tsdf_frame_dev with stage overlap on; the streaming context queues mesh_stream(tag = f) behind every frame
    and picks frames up two late from a 3-slot ring, its twin extracts at the same level after every frame (a host wait each)."""
    import torch
    mk = dict(n_streams=2, width=160, height=120, lut_res=32, inv_res=32)
    scs = [rr.scene.make_scene(**mk), rr.scene.make_scene(**mk, sphere_c=(0.4, 0.7, -0.3), box_c=(-0.5, 1.5, 0.2))]
    raw = [[torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ("depth", "quality", "silhouette", "color")] for sc in scs]
    torch.cuda.synchronize()
    mv, pr = rr.scene.default_view(64, 36)
    frames, lag = 4, 2

    def run(mode):
        hip = rr.ReconIntegrationHip(scs[0], res=(64, 64, 64), **KW)
        meshes = []
        if mode == "stream":
            hip.mesh_stream_config(normals=True, colours=True, slots=3, level=level, **BIG)
        for f in range(frames):
            hip.frame_dev(mv, pr, [t.data_ptr() for t in raw[f % 2]])
            if mode == "stream":
                hip.mesh_stream(f)
                if f >= lag:
                    meshes.append(hip.mesh_stream_take())
            else:
                meshes.append(pack_extract(hip, scs[0], True, True, level))
        for f in range(frames - lag, frames):
            if mode == "stream":
                meshes.append(hip.mesh_stream_take())
        hip.close()
        return meshes

    streamed, twin = run("stream"), run("extract")
    assert len(twin[0][0]) > 50 and twin[0][0].tobytes() != twin[1][0].tobytes()          # the two frames differ
    for f in range(frames):
        v, t, info = streamed[f]
        assert info["tag"] == f and info["overflow"] == 0 and info["vertex_stride"] == 16, f
        assert v.tobytes() == twin[f][0].tobytes() and t.tobytes() == twin[f][1].tobytes(), f


def test_reconfiguring_between_levels_while_idle(rr, scene2, random_case):
    vol, wants = random_case
    hip = rr.ReconIntegrationHip(scene2, res=RANDOM_RES, **KW)
    hip.set_tsdf(vol)
    assert code(rr, hip.mesh_stream_level) == -4                         # before any config
    for level in (2, 0, 2):
        hip.mesh_stream_config(level=level, **BIG)
        assert hip.mesh_stream_level() == level
        v, t, info = stream_one(hip)
        assert info["overflow"] == 0 and info["needed_tiles"] == wants[level]["tiles_with_surface"]
        assert v.tobytes() == P.pack(wants[level]["unit"]).tobytes() and t.tobytes() == wants[level]["triangles"].tobytes(), level
    hip.mesh_stream_config(**BIG)                                        # tsdf_mesh_stream_config is level 0
    assert hip.mesh_stream_level() == 0
    hip.close()


def test_errors(rr, small_scene):
    lib = rr.load_library()
    hip = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), **KW)
    assert code(rr, lambda: hip.extract_mesh(normals=False, colours=False, level=1)) == -4          # before any integrate / volume upload
    assert code(rr, lambda: hip.extract_mesh(normals=False, colours=False, level=3)) == -1
    assert code(rr, lambda: hip.mesh_stream_config(level=3, **BIG)) == -1
    assert lib.tsdf_mesh_stream_level(hip._c, None) == -1
    assert lib.tsdf_mesh_extract_lod(hip._c, C.c_uint32(4), C.c_uint32(1), None, None) == -1       # an unknown flag
    integrate(hip)
    assert code(rr, lambda: hip.extract_mesh(normals=False, colours=False, level=3)) == -1
    hip.extract_mesh(normals=False, colours=False, level=2)
    assert code(rr, lambda: hip.download_mesh(normals=True, colours=False)) == -4                    # attributes the extract did not produce
    hip.mesh_stream_config(level=1, slots=2, **BIG)
    hip.mesh_stream(1)
    assert code(rr, lambda: hip.mesh_stream_config(level=2, **BIG)) == -4                            # a frame is queued: the ring is busy
    assert hip.mesh_stream_level() == 1
    hip.mesh_stream_take()
    hip.mesh_stream_config(level=2, **BIG)
    hip.close()

    bare = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), upload=False, **KW)                  # a volume, but neither calibration nor frame
    bare.set_tsdf(M.sphere_volume((32, 32, 32), limit=LIMIT))
    assert code(rr, lambda: bare.extract_mesh(normals=False, colours=True, level=1)) == -4
    assert len(bare.extract_mesh(normals=True, colours=False, level=1)["position"]) > 50
    bare.close()

    slab = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), slab=(0, 16), **KW)
    assert code(rr, lambda: slab.extract_mesh(normals=False, colours=False, level=1)) == -4
    slab.mesh_stream_config(level=1, **BIG)
    assert code(rr, lambda: slab.mesh_stream(0)) == -4
    slab.close()



def test_a_thin_lattice_yields_zero_counts(rr, scene2):
    """4 x 20 x 20: one lattice point along x at level 2 -- no cell, nothing is launched; two at level 1"""
    ext = [float(x) for x in np.asarray(scene2["bbox_max"]) - np.asarray(scene2["bbox_min"])]
    res = (4, 20, 20)
    vol = np.random.default_rng(3).uniform(-LIMIT, LIMIT, res[::-1]).astype(np.float32)
    thin = rr.ReconIntegrationHip(scene2, res=res, brick_size=[ext[0] / 2, ext[1] / 10, ext[2] / 10], limit=LIMIT, view=(64, 36))
    thin.set_tsdf(vol)
    got = thin.extract_mesh(normals=False, colours=False, level=2)
    st = thin.mesh_stats()
    assert len(got["position"]) == 0 and len(got["triangles"]) == 0 and (st["tiles"], st["tiles_skipped"], st["tiles_with_surface"], st["bytes"]) == (1, 0, 0, 0)
    thin.mesh_stream_config(level=2, **BIG)
    v, t, info = stream_one(thin)
    assert (info["n_vertices"], info["n_triangles"], info["overflow"], info["res"]) == (0, 0, 0, res)
    want = L.extract_lod(vol, LIMIT, scene2["bbox_min"], scene2["bbox_max"], 1)
    assert len(want["position"]) > 100
    assert_equals_reference(thin.extract_mesh(normals=False, colours=False, level=1), want)
    thin.close()
