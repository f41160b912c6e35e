"""GPU: mesh streaming (tsdf_mesh_stream) against tests/mesh_pack_reference.py and against the same context's tsdf_mesh_extract, byte for byte: the random
volume of test_gpu_mesh.py with zeros, -0, NaN and infinities planted; an integrated scene, culled and in a sparse pool, with every attribute
combination; the capacities to the unit; the ring's order and error codes; eight frames through the lanes beside a twin that extracts and a third context
that never meshes."""
import numpy as np
import pytest

import mesh_pack_reference as P
import mesh_reference as M
import present_reference

pytestmark = pytest.mark.gpu

LIMIT = 0.04
KW = dict(brick_size=[2.0 / 8, 2.2 / 8, 2.0 / 8], limit=LIMIT, view=(64, 36))
BIG = dict(max_vertices=1 << 17, max_triangles=1 << 18, max_surface_tiles=64)


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


def pack_extract(hip, scene, normals, colours):
    """the packing of this context's own tsdf_mesh_extract: unit-cube positions from the numpy extraction of its volume (whose world positions must be
    the device's bit for bit), normals and colours the device's arrays"""
    got = hip.extract_mesh(normals=normals, colours=colours)
    want = M.extract(hip.tsdf(), LIMIT, scene["bbox_min"], scene["bbox_max"])
    assert got["position"].tobytes() == want["position"].tobytes() and got["triangles"].tobytes() == want["triangles"].tobytes()
    return P.pack(want["unit"], got.get("normal"), got.get("colour")), got["triangles"]


@pytest.fixture(scope="module")
def scene2(rr):
    return rr.scene.make_scene(n_streams=2, width=160, height=120, lut_res=32, inv_res=32)


def test_random_volume_byte_equal_reproducible_and_copied_to_the_byte(rr, scene2):
    """20 x 22 x 19: padded tiles and tile borders on every axis; ~10 % exact zeros, and -0, NaN, +-inf (outside, outside, -limit, -limit)"""
    res = (20, 22, 19)
    rng = np.random.default_rng(20221019)
    vol = rng.uniform(-LIMIT, LIMIT, res[::-1]).astype(np.float32)
    vol[rng.random(vol.shape) < 0.10] = 0.0
    special = np.array([-0.0, np.nan, np.inf, -np.inf], np.float32)
    pick = rng.random(vol.shape) < 0.02
    vol[pick] = special[rng.integers(0, 4, int(pick.sum()))]
    hip = rr.ReconIntegrationHip(scene2, res=res, **KW)
    hip.set_tsdf(vol)
    want_v, want_t, m = P.pack_volume(vol, LIMIT, scene2["bbox_min"], scene2["bbox_max"])
    nv, nt = len(want_v), len(want_t)
    assert nv > 10000 and nt > 10000
    hip.mesh_stream_config(slots=2, **BIG)
    v, t, info = stream_one(hip, tag=5)
    print("random volume:", info)
    assert info["overflow"] == 0 and info["vertex_stride"] == 8 and info["flags"] == 0 and info["tag"] == 5
    assert (info["n_vertices"], info["n_triangles"], info["needed_vertices"], info["needed_triangles"], info["needed_tiles"]) == (nv, nt, nv, nt, 27)
    assert info["res"] == res and info["bbox_min"].tobytes() == np.asarray(scene2["bbox_min"], np.float32).tobytes()
    assert info["bbox_max"].tobytes() == np.asarray(scene2["bbox_max"], np.float32).tobytes()
    assert v.dtype == np.uint16 and v.shape == (nv, 4) and v.tobytes() == want_v.tobytes()
    assert t.dtype == np.uint32 and t.tobytes() == want_t.tobytes()
    assert t.tobytes() == hip.extract_mesh(normals=False, colours=False)["triangles"].tobytes()
    assert hip.mesh_stream_stats()["payload_bytes"] == nv * 8 + nt * 12
    v2, t2, _ = stream_one(hip)
    assert v2.tobytes() == v.tobytes() and t2.tobytes() == t.tobytes()
    st = hip.mesh_stream_stats()
    assert st["frames"] == 2 and st["overflowed"] == 0 and st["payload_bytes"] == 2 * (nv * 8 + nt * 12) and st["device_bytes"] > 2 * (BIG["max_vertices"] * 8)
    hip.close()


@pytest.mark.parametrize("sparse", [False, True])
def test_small_scene_every_attribute_combination(rr, small_scene, sparse):
    hip = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), sparse_pool_tiles=64 if sparse else 0, **KW)
    integrate(hip)
    want_v, want_t = pack_extract(hip, small_scene, True, True)
    assert len(want_v) > 200 and hip.mesh_stats()["tiles_skipped"] > 0
    nan_normals = int((want_v[:, 8:12].copy().view(np.int16) == -32768).all(axis=1).sum())
    print("small scene:", len(want_v), "vertices,", nan_normals, "NaN normal codes,", int((want_v[:, 15] == 255).sum()), "valid colours")
    assert (want_v[:, 15] == 255).sum() > 100
    for normals, colours in ((True, True), (True, False), (False, True)):
        hip.mesh_stream_config(normals=normals, colours=colours, **BIG)
        v, t, info = stream_one(hip)
        assert info["vertex_stride"] == 16 and info["overflow"] == 0 and info["flags"] == (1 if normals else 0) | (2 if colours else 0)
        assert v.dtype == np.uint8 and v.shape == want_v.shape and t.tobytes() == want_t.tobytes()
        assert v[:, :8].tobytes() == want_v[:, :8].tobytes()
        assert v[:, 8:12].tobytes() == (want_v[:, 8:12].tobytes() if normals else bytes(4 * len(v)))
        assert v[:, 12:].tobytes() == (want_v[:, 12:].tobytes() if colours else bytes(4 * len(v)))
        un = rr.unpack_mesh_vertices(v)
        assert un["position"].shape == (len(v), 3) and un["normal"].dtype == np.int16 and un["colour"].shape == (len(v), 4)
    hip.mesh_stream_config(**BIG)                                        # positions alone: stride 8, the same codes
    v, t, info = stream_one(hip)
    assert info["vertex_stride"] == 8 and v.tobytes() == np.ascontiguousarray(want_v[:, :8]).tobytes() and t.tobytes() == want_t.tobytes()
    hip.close()


def test_overflow_is_decided_to_the_unit(rr, small_scene):
    hip = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), **KW)
    integrate(hip)
    want_v, want_t = pack_extract(hip, small_scene, True, False)
    nv, nt, ns = len(want_v), len(want_t), hip.mesh_stats()["tiles_with_surface"]
    exact = dict(max_vertices=nv, max_triangles=nt, max_surface_tiles=ns)
    hip.mesh_stream_config(normals=True, **exact)
    v, t, info = stream_one(hip)
    assert info["overflow"] == 0 and v.tobytes() == want_v.tobytes() and t.tobytes() == want_t.tobytes()
    assert hip.mesh_stream_stats()["payload_bytes"] == nv * 16 + nt * 12
    for key, bit in (("max_vertices", rr.MESH_OVERFLOW_VERTICES), ("max_triangles", rr.MESH_OVERFLOW_TRIANGLES), ("max_surface_tiles", rr.MESH_OVERFLOW_TILES)):
        hip.mesh_stream_config(normals=True, **dict(exact, **{key: exact[key] - 1}))
        v, t, info = stream_one(hip, tag=9)
        assert info["overflow"] == bit and info["tag"] == 9, key
        assert info["n_vertices"] == 0 and info["n_triangles"] == 0 and len(v) == 0 and len(t) == 0
        assert (info["needed_vertices"], info["needed_triangles"], info["needed_tiles"]) == (nv, nt, ns)
        st = hip.mesh_stream_stats()
        assert st["payload_bytes"] == 0 and st["overflowed"] == 1 and st["frames"] == 1
    hip.mesh_stream_config(normals=True, **BIG)
    v, t, info = stream_one(hip)
    assert info["overflow"] == 0 and v.tobytes() == want_v.tobytes() and t.tobytes() == want_t.tobytes()
    hip.close()


def test_ring_order_states_and_empty_volume(rr, small_scene, scene2):
    hip = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), **KW)
    assert code(rr, lambda: hip.mesh_stream(0)) == -4                    # before any config
    for bad in (dict(slots=1), dict(slots=9), dict(max_vertices=0), dict(max_triangles=0), dict(max_surface_tiles=0)):
        assert code(rr, lambda: hip.mesh_stream_config(**dict(BIG, **bad))) == -1
    lib = rr.load_library()
    import ctypes as C
    assert lib.tsdf_mesh_stream_config(hip._c, C.c_uint32(4), C.c_uint32(1), C.c_uint32(1), C.c_uint32(1), C.c_uint32(3)) == -1   # an unknown flag
    hip.mesh_stream_config(slots=3, **BIG)
    assert code(rr, lambda: hip.mesh_stream(0)) == -4                    # before any volume exists
    assert code(rr, lambda: hip.mesh_stream_acquire()) == -4             # nothing queued
    assert code(rr, hip.mesh_stream_release) == -4                       # nothing held
    integrate(hip)
    want_v, want_t = pack_extract(hip, small_scene, False, False)
    for tag in (10, 11, 12):
        hip.mesh_stream(tag)
    assert code(rr, lambda: hip.mesh_stream(13)) == -4                   # every slot is taken; nothing was queued
    assert code(rr, lambda: hip.mesh_stream_config(**BIG)) == -4 and code(rr, lambda: hip.setVoxelSize(0.1)) == -4
    polls = 0
    for tag in (10, 11, 12, 13):
        got = None
        while got is None:                                               # wait = 0: nothing, or the complete frame
            got = hip.mesh_stream_acquire(wait=False)
            polls += 1
            assert polls < 10_000_000
        v, t, info = got
        assert info["tag"] == tag and info["overflow"] == 0
        assert v.tobytes() == np.ascontiguousarray(want_v).tobytes() and t.tobytes() == want_t.tobytes()
        assert code(rr, lambda: hip.mesh_stream_acquire()) == -4         # a frame is held already
        assert code(rr, lambda: hip.setVoxelSize(0.1)) == -4
        hip.mesh_stream_release()
        if tag == 10:
            hip.mesh_stream(13)                                          # the freed slot
    assert hip.mesh_stream_stats()["frames"] == 4
    assert code(rr, lambda: hip.mesh_stream_acquire()) == -4
    # Drained with the head at slot 1 of three.  A ring of another size starts at its slot 0 whatever the old head was: exactly two frames are taken, they come
    # out in order with the bytes as before, and the third frame is written where the first one was -- once round a ring of two.
    hip.mesh_stream_config(slots=2, **BIG)
    hip.mesh_stream(20)
    hip.mesh_stream(21)
    assert code(rr, lambda: hip.mesh_stream(22)) == -4                   # both slots are taken
    where = []
    for tag in (20, 21, 22):
        v, t, info = hip.mesh_stream_acquire(wait=True)
        assert info["tag"] == tag and info["overflow"] == 0
        assert v.tobytes() == np.ascontiguousarray(want_v).tobytes() and t.tobytes() == want_t.tobytes()
        where.append(v.ctypes.data)
        hip.mesh_stream_release()
        if tag == 20:
            hip.mesh_stream(22)
    assert where[2] == where[0] and where[1] != where[0]
    assert hip.mesh_stream_stats()["frames"] == 3                        # (counted from the config)
    assert code(rr, lambda: hip.mesh_stream_acquire()) == -4
    hip.close()

    hip = rr.ReconIntegrationHip(scene2, res=(20, 22, 19), **KW)         # every voxel -limit: no surface
    hip.set_tsdf(np.full((19, 22, 20), -LIMIT, np.float32))
    hip.mesh_stream_config(normals=True, **BIG)
    v, t, info = stream_one(hip)
    assert info["overflow"] == 0 and (info["n_vertices"], info["n_triangles"], info["needed_vertices"], info["needed_tiles"]) == (0, 0, 0, 0)
    assert len(v) == 0 and len(t) == 0 and hip.mesh_stream_stats()["payload_bytes"] == 0
    hip.close()

    bare = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), upload=False, **KW)     # a volume, but neither calibration nor frame
    bare.set_tsdf(M.sphere_volume((32, 32, 32), limit=LIMIT))
    bare.mesh_stream_config(colours=True, **BIG)
    assert code(rr, lambda: bare.mesh_stream(0)) == -4
    bare.mesh_stream_config(normals=True, **BIG)
    assert stream_one(bare)[2]["n_vertices"] > 100
    bare.close()

    slab = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), slab=(0, 16), **KW)
    slab.mesh_stream_config(**BIG)
    assert code(rr, lambda: slab.mesh_stream(0)) == -4
    slab.close()

    ext = [float(x) for x in np.asarray(scene2["bbox_max"]) - np.asarray(scene2["bbox_min"])]
    thin = rr.ReconIntegrationHip(scene2, res=(16, 1, 16), brick_size=[ext[0] / 8, ext[1], ext[2] / 8], limit=LIMIT, view=(64, 36))   # one point thick: no cell
    thin.set_tsdf(np.random.default_rng(3).uniform(-LIMIT, LIMIT, (16, 1, 16)).astype(np.float32))
    thin.mesh_stream_config(**BIG)
    v, t, info = stream_one(thin)
    assert (info["n_vertices"], info["n_triangles"], info["overflow"], info["res"]) == (0, 0, 0, (16, 1, 16))
    thin.close()


@pytest.mark.parametrize("with_present", [False, True])
def test_sequence_through_the_lanes(rr, with_present):
    """Two scenes alternate for 8 frames through tsdf_frame_dev with stage overlap on (the volume sets alternate per frame).  The streaming context queues
    mesh_stream(tag = f) behind every frame and picks frames up two late from a 3-slot ring; its twin extracts every frame (a host wait each); a third
    context never meshes; the streaming context runs twice, once downloading its framebuffer every frame like the others and once free-running (no host wait
    inside the loop; with the present ring its pictures come through that).  Every streamed frame is the packing of the twin's mesh of the same frame -- the integrate of frame f + 2 must not reset the set
    frame f's mesh kernels still read --, and all three draw the same pictures."""
    import torch
    mk = dict(n_streams=2, width=160, height=120, lut_res=32, inv_res=32)
    scs = [rr.scene.make_scene(**mk), rr.scene.make_scene(**mk, sphere_c=(0.4, 0.7, -0.3), box_c=(-0.5, 1.5, 0.2))]
    raw = [[torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ("depth", "quality", "silhouette", "color")] for sc in scs]
    torch.cuda.synchronize()
    mv, pr = rr.scene.default_view(64, 36)
    frames, lag = 8, 2

    def run(mode, download=True):
        hip = rr.ReconIntegrationHip(scs[0], res=(32, 32, 32), **KW)
        meshes, fbs, shown = [], [], []
        if mode == "stream":
            hip.mesh_stream_config(normals=True, colours=True, slots=3, **BIG)
            if with_present:
                hip.present_config(rr.PRESENT_RGBA8, 0, 3)
        for f in range(frames):
            hip.frame_dev(mv, pr, [t.data_ptr() for t in raw[f % 2]])
            if mode == "stream":
                if with_present:
                    hip.present(f)
                hip.mesh_stream(f)
                if f >= lag:
                    meshes.append(hip.mesh_stream_take())
                    if with_present:
                        shown.append(hip.present_acquire()); hip.present_release()
            elif mode == "extract":
                got = hip.extract_mesh(normals=True, colours=True)
                want = M.extract(hip.tsdf(), LIMIT, scs[0]["bbox_min"], scs[0]["bbox_max"])
                assert got["position"].tobytes() == want["position"].tobytes()
                meshes.append((P.pack(want["unit"], got["normal"], got["colour"]), got["triangles"]))
            if download:
                fbs.append(hip.framebuffer()[0])                         # (a host wait: the free-running variant below does without)
        for f in range(frames - lag, frames):
            if mode == "stream":
                meshes.append(hip.mesh_stream_take())
                if with_present:
                    shown.append(hip.present_acquire()); hip.present_release()
        hip.close()
        return meshes, fbs, shown

    free, _, shown = run("stream", download=False)                    # the host never waits inside the loop: the lanes run ahead as in a client
    streamed, stream_fb, _ = run("stream")
    twin, twin_fb, _ = run("extract")
    _, plain_fb, _ = run("plain")
    assert len(twin[0][0]) > 100 and twin[0][0].tobytes() != twin[1][0].tobytes()        # the two frames differ
    same = lambda a, b: ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()
    for f in range(frames):
        for v, t, info in (free[f], streamed[f]):
            assert info["tag"] == f and info["overflow"] == 0 and info["vertex_stride"] == 16, f
            assert v.tobytes() == twin[f][0].tobytes() and t.tobytes() == twin[f][1].tobytes(), f
        assert same(stream_fb[f], plain_fb[f]) and same(twin_fb[f], plain_fb[f]), f
        if with_present:
            assert shown[f][1] == f and shown[f][0].tobytes() == present_reference.to_rgba8(plain_fb[f]).tobytes(), f
