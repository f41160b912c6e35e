"""GPU: the filtered mesh stream (tsdf_mesh_stream_config_filter, min_triangles >= 1) against tests/mesh_stream_filter_reference.py, byte for byte: the
components' test volumes (a speckle of blobs, the random volume, two tubes through every tile, nested shells), a level of detail on an odd resolution,
an integrated scene with normals and colours against the same context's one-shot extract -> components -> filter, the capacities to the unit, the ring's
order, reconfiguring, error codes, and six frames through the lanes beside a twin that filters one-shot and a third context that never meshes."""
import ctypes as C
import functools

import numpy as np
import pytest

import mesh_component_reference as K
import mesh_pack_reference as P
import mesh_reference as M
import mesh_stream_filter_reference as F

pytestmark = pytest.mark.gpu

LIMIT = K.LIMIT
KW = dict(brick_size=[2.0 / 8, 2.2 / 8, 2.0 / 8], limit=LIMIT, view=(64, 36))
BIG = dict(max_vertices=1 << 17, max_triangles=1 << 18, max_surface_tiles=256)
VOLUMES = dict(speckle=(K.speckle_volume, (20, 22, 19)), random=(K.random_volume, (20, 22, 19)), snakes=(K.snakes_volume, (40, 24, 24)),
               shells=(K.shells_volume, (40, 24, 24)), speckle_odd=(lambda: K.speckle_volume(res=(39, 43, 37)), (39, 43, 37)))


@pytest.fixture(scope="module")
def scene2(rr):
    return rr.scene.make_scene(n_streams=2, width=160, height=120, lut_res=32, inv_res=32)


@functools.lru_cache(maxsize=None)
def volume(name):
    vol = VOLUMES[name][0]()
    vol.setflags(write=False)
    return vol


@pytest.fixture(scope="module")
def reference(scene2):
    """(name, min_triangles, level) -> (packed vertices, triangles, words), computed once"""
    @functools.lru_cache(maxsize=None)
    def ref(name, min_triangles, level=0):
        return F.filtered_frame(volume(name), LIMIT, scene2["bbox_min"], scene2["bbox_max"], min_triangles, level=level)
    return ref


def context(rr, scene, name, **kw):
    hip = rr.ReconIntegrationHip(scene, res=VOLUMES[name][1], **KW, **kw)
    hip.set_tsdf(volume(name))
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


def words_of(info):
    f = info["filter"]
    return (f["components"], f["kept"], f["vertices_removed"], f["triangles_removed"])


def assert_frame(got, want, what=""):
    v, t, info = got
    assert v.dtype == want[0].dtype and v.shape == want[0].shape and v.tobytes() == want[0].tobytes(), what
    assert t.dtype == np.uint32 and t.shape == want[1].shape and t.tobytes() == want[1].tobytes(), what
    assert (info["n_vertices"], info["n_triangles"]) == (len(want[0]), len(want[1])) and info["overflow"] == 0, what
    assert words_of(info) == tuple(want[2]), what


def test_speckle_min_100_positions_only(rr, scene2, reference):
    hip = context(rr, scene2, "speckle")
    hip.extract_mesh(normals=False, colours=False)
    tiles = hip.mesh_stats()["tiles_with_surface"]
    hip.mesh_stream_config(slots=2, min_triangles=100, **BIG)
    assert hip.mesh_stream_min_triangles() == 100
    got = stream_one(hip, tag=5)
    v, t, info = got
    print("speckle, min 100:", info)
    want = reference("speckle", 100)
    assert_frame(got, want)
    assert (info["n_vertices"], info["n_triangles"]) == (7958, 15180)
    assert (info["needed_vertices"], info["needed_triangles"], info["needed_tiles"]) == (13532, 24420, tiles)
    assert words_of(info) == (343, 61, 5574, 9240)
    assert info["vertex_stride"] == 8 and info["flags"] == 0 and info["tag"] == 5 and info["res"] == (20, 22, 19)
    assert info["bbox_min"].tobytes() == np.asarray(scene2["bbox_min"], np.float32).tobytes()
    assert info["bbox_max"].tobytes() == np.asarray(scene2["bbox_max"], np.float32).tobytes()
    assert hip.mesh_stream_stats()["payload_bytes"] == 7958 * 8 + 15180 * 12
    v2, t2, info2 = stream_one(hip)
    assert v2.tobytes() == v.tobytes() and t2.tobytes() == t.tobytes() and words_of(info2) == words_of(info)
    st = hip.mesh_stream_stats()
    assert st["frames"] == 2 and st["overflowed"] == 0 and st["payload_bytes"] == 2 * (7958 * 8 + 15180 * 12)
    assert st["device_bytes"] > 3 * (BIG["max_vertices"] * 8 + BIG["max_triangles"] * 12)      # two slots and the raw buffer
    hip.close()


def test_min_1_keeps_everything_through_the_filter(rr, scene2, reference):
    hip = context(rr, scene2, "random")
    hip.mesh_stream_config(slots=2, **BIG)
    assert hip.mesh_stream_min_triangles() == 0
    plain = stream_one(hip)
    assert "filter" not in plain[2]
    hip.mesh_stream_config(slots=2, min_triangles=1, **BIG)
    got = stream_one(hip)
    assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes()
    assert {k: v for k, v in got[2].items() if k not in ("filter", "bbox_min", "bbox_max")} == {k: v for k, v in plain[2].items() if k not in ("bbox_min", "bbox_max")}
    assert words_of(got[2]) == (8, 8, 0, 0)
    assert_frame(got, reference("random", 1))
    hip.close()


def test_random_volume_min_100(rr, scene2, reference):
    hip = context(rr, scene2, "random")
    hip.mesh_stream_config(slots=2, min_triangles=100, **BIG)
    got = stream_one(hip)
    assert_frame(got, reference("random", 100))
    assert (got[2]["n_vertices"], got[2]["n_triangles"]) == (26222, 52574) and words_of(got[2])[:2] == (8, 2)
    hip.close()


def test_snakes_the_smallest_label_travels_through_every_tile(rr, scene2, reference):
    hip = context(rr, scene2, "snakes")
    hip.mesh_stream_config(slots=2, min_triangles=12796, **BIG)
    got = stream_one(hip)
    assert_frame(got, reference("snakes", 12796))
    assert (got[2]["n_vertices"], got[2]["n_triangles"]) == (12800, 25592) and words_of(got[2]) == (2, 2, 0, 0)
    hip.mesh_stream_config(slots=2, min_triangles=12797, **BIG)
    got = stream_one(hip)
    assert_frame(got, reference("snakes", 12797))
    assert (got[2]["n_vertices"], got[2]["n_triangles"]) == (0, 0) and words_of(got[2]) == (2, 0, 12800, 25592)
    hip.close()


def test_shells_remapped_across_the_gap_and_the_empty_frame(rr, scene2, reference):
    hip = context(rr, scene2, "shells")
    for min_triangles, counts, kept in ((2000, (10584, 21160), 2), (5969, None, 1), (15193, (0, 0), 0)):
        hip.mesh_stream_config(slots=2, min_triangles=min_triangles, **BIG)
        got = stream_one(hip, tag=min_triangles)
        want = reference("shells", min_triangles)
        assert_frame(got, want, min_triangles)
        v, t, info = got
        assert words_of(info)[:2] == (3, kept) and info["tag"] == min_triangles
        assert (info["needed_vertices"], info["needed_triangles"]) == (11246, 22480)
        if counts is not None:
            assert (info["n_vertices"], info["n_triangles"]) == counts
        if min_triangles == 5969:
            assert info["n_triangles"] == 15192
        if len(t):
            assert int(t.max()) == len(v) - 1                            # the inner ball (vertices 317 ..) is gone: the indices are dense again
        assert hip.mesh_stream_stats()["payload_bytes"] == len(v) * 8 + len(t) * 12
    assert hip.mesh_stream_stats()["overflowed"] == 0                   # the empty frame: acquired, nothing copied, no overflow
    hip.close()


def test_level_1_on_an_odd_resolution(rr, scene2, reference):
    hip = context(rr, scene2, "speckle_odd")
    hip.mesh_stream_config(slots=2, level=1, min_triangles=100, **BIG)
    assert hip.mesh_stream_level() == 1 and hip.mesh_stream_min_triangles() == 100
    got = stream_one(hip)
    assert_frame(got, reference("speckle_odd", 100, 1))
    assert (got[2]["n_vertices"], got[2]["n_triangles"]) == (8046, 15458) and words_of(got[2])[:2] == (333, 51)
    assert (got[2]["needed_vertices"], got[2]["needed_triangles"]) == (13616, 24550)
    hip.close()


def oneshot_filtered(hip, scene, min_triangles, normals, colours):
    """this context's extract -> components -> filter -> download, packed: (vertices, triangles, words, the table before the filter).  Unit-cube positions
    come from the numpy extraction of the context's volume, whose world positions must be the device's bit for bit."""
    full = hip.extract_mesh(normals=normals, colours=colours)
    want = M.extract(hip.tsdf(), LIMIT, scene["bbox_min"], scene["bbox_max"])
    assert full["position"].tobytes() == want["position"].tobytes() and full["triangles"].tobytes() == want["triangles"].tobytes()
    n = hip.mesh_components()
    comps = hip.mesh_download_components()
    flags = comps["table"]["n_triangles"] >= min_triangles
    kv = flags[comps["vertex_component"]] if n else np.zeros(0, bool)
    nv, nt = hip.mesh_filter(min_triangles)
    got = hip.download_mesh(normals=normals, colours=colours)
    assert got["position"].tobytes() == want["position"][kv].tobytes()
    words = (n, int(flags.sum()), len(full["position"]) - nv, len(full["triangles"]) - nt)
    return P.pack(want["unit"][kv], got.get("normal"), got.get("colour")), got["triangles"], words, comps["table"]


@pytest.mark.parametrize("sparse", [False, True])
def test_integrated_scene_equals_the_one_shot_filter(rr, small_scene, sparse):
    hip = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), sparse_pool_tiles=64 if sparse else 0, **KW)
    integrate(hip)
    hip.extract_mesh(normals=False, colours=False)
    hip.mesh_components()
    n_triangles = np.sort(hip.mesh_download_components()["table"]["n_triangles"])
    print("integrated scene, components:", n_triangles.tolist())
    assert len(n_triangles) >= 2 and n_triangles[0] < n_triangles[-1]
    min_triangles = int(n_triangles[-1])                                # the largest stays, a smaller one goes
    want = oneshot_filtered(hip, small_scene, min_triangles, True, True)
    assert 1 <= want[2][1] < want[2][0] and want[2][2] > 0 and len(want[0]) > 100
    hip.mesh_stream_config(normals=True, colours=True, min_triangles=min_triangles, **BIG)
    got = stream_one(hip)
    assert got[2]["vertex_stride"] == 16 and got[2]["flags"] == 3
    assert_frame(got, want[:3])
    assert (want[0][:, 15] == 255).sum() > 50                            # the scene does colour what is kept
    hip.close()


def test_capacities_bound_the_unfiltered_mesh_to_the_unit(rr, scene2, reference):
    hip = context(rr, scene2, "speckle")
    hip.extract_mesh(normals=False, colours=False)
    tiles = hip.mesh_stats()["tiles_with_surface"]
    exact = dict(max_vertices=13532, max_triangles=24420, max_surface_tiles=tiles)
    hip.mesh_stream_config(min_triangles=100, **exact)
    assert_frame(stream_one(hip), reference("speckle", 100))
    for key, bit in (("max_vertices", rr.MESH_OVERFLOW_VERTICES), ("max_triangles", rr.MESH_OVERFLOW_TRIANGLES), ("max_surface_tiles", rr.MESH_OVERFLOW_TILES)):
        hip.mesh_stream_config(min_triangles=100, **dict(exact, **{key: exact[key] - 1}))   # the filtered mesh (7958, 15180) would fit: it overflows all the same
        v, t, info = stream_one(hip, tag=9)
        assert info["overflow"] == bit and info["tag"] == 9, key
        assert info["n_vertices"] == 0 and info["n_triangles"] == 0 and len(v) == 0 and len(t) == 0
        assert (info["needed_vertices"], info["needed_triangles"], info["needed_tiles"]) == (13532, 24420, tiles)
        assert words_of(info) == (0, 0, 0, 0)
        st = hip.mesh_stream_stats()
        assert st["payload_bytes"] == 0 and st["overflowed"] == 1 and st["frames"] == 1
    hip.mesh_stream_config(min_triangles=100, **exact)
    assert_frame(stream_one(hip), reference("speckle", 100))
    hip.close()


def test_ring_of_three_alternating_speckle_and_shells(rr, scene2):
    """one ring, one resolution: a speckle at the shells' 40 x 24 x 24 and the shells are uploaded alternately, three frames in flight"""
    res = (40, 24, 24)
    vols = (K.speckle_volume(res=res), volume("shells"))
    want = [F.filtered_frame(vol, LIMIT, scene2["bbox_min"], scene2["bbox_max"], 100) for vol in vols]
    assert 0 < want[0][2][1] < want[0][2][0] and want[1][2] == (3, 3, 0, 0)
    hip = rr.ReconIntegrationHip(scene2, res=res, **KW)
    hip.mesh_stream_config(slots=3, min_triangles=100, **BIG)
    polls = 0

    def take(k):
        nonlocal polls
        got = None
        while got is None:                                               # wait = 0: nothing, or the complete frame
            got = hip.mesh_stream_acquire(wait=False)
            polls += 1
            assert polls < 10_000_000
        v, t, info = got
        assert info["tag"] == 100 + k and info["overflow"] == 0, k
        assert (info["n_vertices"], info["n_triangles"]) == (len(want[k % 2][0]), len(want[k % 2][1])), k
        assert v.tobytes() == want[k % 2][0].tobytes() and t.tobytes() == want[k % 2][1].tobytes(), k
        f = hip.mesh_stream_frame_filter()
        assert (f["components"], f["kept"], f["vertices_removed"], f["triangles_removed"]) == tuple(want[k % 2][2]), k
        assert code(rr, lambda: hip.mesh_stream_acquire()) == -4         # a frame is held already
        hip.mesh_stream_release()

    frames, taken = 7, 0
    for k in range(frames):
        hip.set_tsdf(vols[k % 2])
        hip.mesh_stream(100 + k)
        if k + 1 - taken == 3:
            assert code(rr, lambda: hip.mesh_stream(999)) == -4          # every slot is taken; nothing was queued
            assert code(rr, lambda: hip.mesh_stream_config(**BIG)) == -4
            take(taken)
            taken += 1
    while taken < frames:
        take(taken)
        taken += 1
    assert hip.mesh_stream_stats()["frames"] == frames
    assert code(rr, lambda: hip.mesh_stream_acquire()) == -4
    hip.close()


def test_reconfiguring_filter_no_filter_and_back(rr, scene2, reference):
    hip = context(rr, scene2, "speckle")
    plain_v, plain_t, _ = P.pack_volume(volume("speckle"), LIMIT, scene2["bbox_min"], scene2["bbox_max"])
    for min_triangles in (100, 0, 100, 2000, 0):
        hip.mesh_stream_config(slots=2, min_triangles=min_triangles, **BIG)
        assert hip.mesh_stream_min_triangles() == min_triangles
        got = stream_one(hip)
        if min_triangles:
            assert_frame(got, reference("speckle", min_triangles), min_triangles)
        else:
            assert "filter" not in got[2] and got[0].tobytes() == plain_v.tobytes() and got[1].tobytes() == plain_t.tobytes()
            hip.mesh_stream(1)
            hip.mesh_stream_acquire()
            assert code(rr, hip.mesh_stream_frame_filter) == -4          # a frame is held, but the ring has no filter
            hip.mesh_stream_release()
    hip.close()


def test_error_codes(rr, scene2, small_scene):
    lib = rr.load_library()
    u = C.c_uint32
    hip = context(rr, scene2, "speckle")
    n, out = u(), (C.c_uint64 * 4)()
    assert lib.tsdf_mesh_stream_min_triangles(hip._c, C.byref(n)) == -4 and lib.tsdf_mesh_stream_frame_filter(hip._c, out) == -4    # before any config
    assert lib.tsdf_mesh_stream_min_triangles(hip._c, None) == -1 and lib.tsdf_mesh_stream_frame_filter(hip._c, None) == -1
    # the argument checks of tsdf_mesh_stream_config_lod
    assert lib.tsdf_mesh_stream_config_filter(hip._c, u(4), u(0), u(100), u(1), u(1), u(1), u(3)) == -1      # an unknown flag
    assert lib.tsdf_mesh_stream_config_filter(hip._c, u(0), u(3), u(100), u(1), u(1), u(1), u(3)) == -1      # level 3
    for bad in (dict(slots=1), dict(slots=9), dict(max_vertices=0), dict(max_triangles=0), dict(max_surface_tiles=0)):
        assert code(rr, lambda: hip.mesh_stream_config(min_triangles=100, **dict(BIG, **bad))) == -1
    assert lib.tsdf_mesh_stream_config_filter(hip._c, u(0), u(0), u(0), u(1 << 17), u(1 << 18), u(256), u(2)) == 0     # min_triangles 0: the plain ring
    assert hip.mesh_stream_min_triangles() == 0
    hip.mesh_stream_config(slots=2, min_triangles=100, **BIG)
    assert code(rr, hip.mesh_stream_frame_filter) == -4                  # nothing held: nothing queued ...
    hip.mesh_stream(1)
    assert code(rr, hip.mesh_stream_frame_filter) == -4                  # ... queued, not yet acquired
    hip.mesh_stream(2)
    assert code(rr, lambda: hip.mesh_stream(3)) == -4                    # a full ring
    hip.mesh_stream_acquire()
    assert hip.mesh_stream_frame_filter()["components"] == 343
    assert lib.tsdf_mesh_stream_frame_filter(hip._c, None) == -1
    hip.mesh_stream_release()
    assert code(rr, hip.mesh_stream_frame_filter) == -4                  # released
    assert hip.mesh_stream_take()[2]["tag"] == 2
    hip.close()
    slab = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), slab=(0, 16), **KW)
    slab.mesh_stream_config(min_triangles=100, **BIG)
    assert code(rr, lambda: slab.mesh_stream(0)) == -4
    slab.close()


def test_no_surface_and_a_lattice_without_cells(rr, scene2):
    hip = rr.ReconIntegrationHip(scene2, res=(20, 22, 19), **KW)         # every voxel -limit: no surface, the filter's workgroups all return
    hip.set_tsdf(np.full((19, 22, 20), -LIMIT, np.float32))
    hip.mesh_stream_config(normals=True, min_triangles=100, **BIG)
    v, t, info = stream_one(hip)
    assert info["overflow"] == 0 and (info["n_vertices"], info["n_triangles"], info["needed_vertices"], info["needed_tiles"]) == (0, 0, 0, 0)
    assert len(v) == 0 and len(t) == 0 and words_of(info) == (0, 0, 0, 0) and hip.mesh_stream_stats()["payload_bytes"] == 0
    hip.close()
    ext = [float(x) for x in np.asarray(scene2["bbox_max"]) - np.asarray(scene2["bbox_min"])]
    thin = rr.ReconIntegrationHip(scene2, res=(16, 1, 16), brick_size=[ext[0] / 8, ext[1], ext[2] / 8], limit=LIMIT, view=(64, 36))   # one point thick: no cell, no launch
    thin.set_tsdf(np.random.default_rng(3).uniform(-LIMIT, LIMIT, (16, 1, 16)).astype(np.float32))
    thin.mesh_stream_config(min_triangles=100, **BIG)
    v, t, info = stream_one(thin)
    assert (info["n_vertices"], info["n_triangles"], info["overflow"], info["res"]) == (0, 0, 0, (16, 1, 16)) and words_of(info) == (0, 0, 0, 0)
    thin.close()


def test_six_frames_through_the_lanes(rr):
    """Two scenes alternate through tsdf_frame_dev with stage overlap on.  The streaming context queues a filtered mesh_stream behind every frame and picks
    frames up two late from a 3-slot ring; its twin extracts, labels and filters one-shot every frame; a third context never meshes.  Every streamed frame
    is the packing of the twin's filtered mesh of the same frame, and the streaming context draws the third's pictures."""
    import torch
    mk = dict(n_streams=2, width=160, height=120, lut_res=32, inv_res=32)
    scs = [rr.scene.make_scene(**mk), rr.scene.make_scene(**mk, sphere_c=(0.4, 0.7, -0.3), box_c=(-0.5, 1.5, 0.2))]
    raw = [[torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ("depth", "quality", "silhouette", "color")] for sc in scs]
    torch.cuda.synchronize()
    mv, pr = rr.scene.default_view(64, 36)
    frames, lag, min_triangles = 6, 2, 200

    def run(mode):
        hip = rr.ReconIntegrationHip(scs[0], res=(32, 32, 32), **KW)
        meshes, fbs = [], []
        if mode == "stream":
            hip.mesh_stream_config(normals=True, colours=True, slots=3, min_triangles=min_triangles, **BIG)
        for f in range(frames):
            hip.frame_dev(mv, pr, [t.data_ptr() for t in raw[f % 2]])
            if mode == "stream":
                hip.mesh_stream(f)
                if f >= lag:
                    meshes.append(hip.mesh_stream_take())
            elif mode == "extract":
                meshes.append(oneshot_filtered(hip, scs[0], min_triangles, True, True))
            fbs.append(hip.framebuffer()[0])
        for f in range(frames - lag, frames):
            if mode == "stream":
                meshes.append(hip.mesh_stream_take())
        hip.close()
        return meshes, fbs

    streamed, stream_fb = run("stream")
    twin, _ = run("extract")
    _, plain_fb = run("plain")
    print("lanes:", [(m[2], len(m[0]), len(m[1])) for m in twin[:2]])
    assert len(twin[0][0]) > 100 and twin[0][0].tobytes() != twin[1][0].tobytes()        # the two frames differ
    assert any(m[2][1] < m[2][0] for m in twin) and all(m[2][1] >= 1 for m in twin)      # something is dropped, something kept
    same = lambda a, b: ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()
    for f in range(frames):
        assert streamed[f][2]["tag"] == f and streamed[f][2]["vertex_stride"] == 16, f
        assert_frame(streamed[f], twin[f][:3], f)
        assert same(stream_fb[f], plain_fb[f]), f
