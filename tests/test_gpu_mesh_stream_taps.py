"""GPU: texture taps in the streamed frame (tsdf_mesh_stream_config_taps / _frame_taps) against tests/mesh_tap_pack_reference.py, byte for byte: the tap
block of every form of the ring -- uint32 indices at both strides, a level of detail, filtered, tile-local compact, slab parts and their join -- taken
at the frame's OWN vertex codes, the frame itself byte-identical to a twin ring without taps; coordinates outside [0, 1] and a NaN; one stream with the
smallest vertex counts; an overflowing frame and the slot after it; the statistics; four frames through the lanes beside a twin context without a mesh
ring; the link to the receiver's rule; every error code; device memory over context cycles."""
import copy
from importlib import import_module

import numpy as np
import pytest

import main_path_reference as R
import mesh_component_reference as K
import mesh_reference as M
import mesh_tap_pack_reference as TP
import texture_tap_reference as T

pytestmark = pytest.mark.gpu

LIMIT = 0.04
KW = dict(brick_size=[2.0 / 8, 2.2 / 8, 2.0 / 8], limit=LIMIT, view=(64, 36))
RES = (37, 43, 35)                                                       # padded tiles on every axis
BIG = dict(max_vertices=1 << 15, max_triangles=1 << 16, max_surface_tiles=256)
f32 = np.float32
SCENES = {"3-streams": dict(n_streams=3, lut_res=24, inv_res=32), "5-streams": dict(n_streams=5, lut_res=32, inv_res=24)}
COLOUR_BOUND = 0.5 / 255.0                                               # tests/test_mesh_tap_pack_reference.py: measured 0.187 / 255 and 0.148 / 255


def code(rr, fn):
    with pytest.raises(rr.TsdfError) as e:
        fn()
    return e.value.code


def stream_one(hip, tag=0):
    hip.mesh_stream(tag)
    return hip.mesh_stream_take(wait=True)


_CASES = {}


def case(rr, name):
    """per scene, computed once and left unchanged: the scene and the float32 reference's integrated volume at RES"""
    if name not in _CASES:
        scene = rr.scene.make_scene(color_width=96, color_height=80, **SCENES[name])
        vol, _ = R.integrate(scene, RES, f32(LIMIT))
        vol.setflags(write=False)
        _CASES[name] = dict(scene=scene, vol=vol, refs={})
    return _CASES[name]


def reference(K_, vertices, limit=LIMIT):
    """frame_taps of a frame's own vertices, once per distinct set of position codes"""
    key = (TP.vertex_codes(vertices).tobytes(), float(limit))
    if key not in K_["refs"]:
        K_["refs"][key] = TP.frame_taps(K_["scene"], limit, vertices)
    return K_["refs"][key]


def assert_taps(frame, want, n_streams, what=""):
    taps = frame[2]["taps"]
    assert taps.dtype == TP.PACKED_TAP_DTYPE and taps.shape == (frame[2]["n_vertices"], n_streams) == want.shape, what
    bad = np.nonzero((taps.reshape(-1).view(np.uint64) != want.reshape(-1).view(np.uint64)))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {taps.size} packed taps differ, e.g. pair {bad[0]}: device {taps.reshape(-1)[bad[0]]} reference {want.reshape(-1)[bad[0]]}"


def payload_of(frame):
    """the bytes of a frame's payload arrays: vertices, table (compact), triangles / codes"""
    v, t, info = frame
    return v.tobytes(), (info["compact"]["table"].tobytes() if "compact" in info else b""), t.tobytes()


def twin_and_taps(rr, hip, K_, what, limit=LIMIT, **cfg):
    """one frame of the ring without taps, one with: the frame byte-identical, the tap block the reference's, the stats to the byte"""
    N = K_["scene"]["n"]
    hip.mesh_stream_config(slots=2, **cfg)
    assert hip.mesh_stream_tap_flags() == 0
    plain = stream_one(hip, tag=3)
    assert "taps" not in plain[2]
    plain_bytes = hip.mesh_stream_stats()["payload_bytes"]
    hip.mesh_stream_config(slots=2, taps=True, **cfg)
    assert hip.mesh_stream_tap_flags() == rr.MESH_STREAM_TAPS
    got = stream_one(hip, tag=3)
    assert payload_of(got) == payload_of(plain), what
    for k in ("n_vertices", "n_triangles", "needed_vertices", "needed_triangles", "needed_tiles", "tag", "flags", "vertex_stride", "overflow", "res"):
        assert got[2][k] == plain[2][k], (what, k)
    nv = got[2]["n_vertices"]
    want = reference(K_, got[0], limit) if nv else np.zeros((0, N), TP.PACKED_TAP_DTYPE)
    assert_taps(got, want, N, what)
    st = hip.mesh_stream_stats()
    assert st["payload_bytes"] == plain_bytes + nv * N * 8 and st["frames"] == 1, what
    return got, want


# ---------------------------------------------------------------------------------------------------------------- every form of the ring
@pytest.mark.parametrize("name", list(SCENES))
def test_whole_volume_rings_carry_the_reference_taps_and_leave_the_frame_alone(rr, name):
    K_ = case(rr, name)
    scene, N = K_["scene"], K_["scene"]["n"]
    hip = rr.ReconIntegrationHip(scene, res=RES, **KW)
    hip.set_tsdf(K_["vol"])
    got, want = twin_and_taps(rr, hip, K_, "plain, stride 8", **BIG)
    nv = got[2]["n_vertices"]
    f = TP.unpack_taps(want)
    sub = int((((want["dist_h"] & 0x7C00) == 0) & ((want["dist_h"] & 0x3FF) != 0)).sum() + (((want["quality_h"] & 0x7C00) == 0) & ((want["quality_h"] & 0x3FF) != 0)).sum())
    fallback = int((T.combine(scene, f)[:, 3] < 0).sum())
    print(f"{name}: {nv} vertices, pairs with quality {(f['quality'] > 0).mean():.2f}, fallback vertices {fallback}, binary16-subnormal fields {sub}")
    assert got[2]["vertex_stride"] == 8 and nv > 4000 and nv % 64 != 0 and nv > 256          # more than one workgroup, no multiple of a wave
    assert (f["quality"] > 0).mean() > 0.2 and fallback > 50 and sub > 50                      # both branches and the subnormals occur
    wide, want16 = twin_and_taps(rr, hip, K_, "normals + colours, stride 16", normals=True, colours=True, **BIG)
    assert wide[2]["vertex_stride"] == 16 and wide[2]["taps"].tobytes() == got[2]["taps"].tobytes()   # the same codes at the other stride
    lod, _ = twin_and_taps(rr, hip, K_, "level 2", level=2, **BIG)
    assert 50 < lod[2]["n_vertices"] < nv // 4
    compact, _ = twin_and_taps(rr, hip, K_, "tile-local compact", index_format=rr.MESH_INDEX_TILE16, **BIG)
    assert compact[2]["taps"].tobytes() == got[2]["taps"].tobytes() and compact[2]["compact"]["triangles_null"]
    # the view of the held frame: into the pinned slot, behind the payload's capacity; valid until the release
    hip.mesh_stream(9)
    v, t, info = hip.mesh_stream_acquire(wait=True)
    view = hip.mesh_stream_frame_taps()
    assert view.shape == (nv, N) and view.tobytes() == got[2]["taps"].tobytes()
    layout_offset = (BIG["max_vertices"] * 8 + 15) // 16 * 16 + BIG["max_surface_tiles"] * 16 + BIG["max_triangles"] * 6
    assert view.ctypes.data - v.ctypes.data == (layout_offset + 15) // 16 * 16
    hip.mesh_stream_release()
    hip.close()


def test_filtered_ring_taps_follow_the_filtered_vertices(rr):
    K_ = case(rr, "3-streams")
    vol = K.speckle_volume()
    hip = rr.ReconIntegrationHip(K_["scene"], res=(20, 22, 19), **dict(KW, limit=K.LIMIT))
    hip.set_tsdf(vol)
    cfg = dict(max_vertices=1 << 17, max_triangles=1 << 18, max_surface_tiles=256)
    got, want = twin_and_taps(rr, hip, K_, "speckle, min 100", limit=K.LIMIT, min_triangles=100, **cfg)
    assert (got[2]["n_vertices"], got[2]["n_triangles"], got[2]["needed_vertices"]) == (7958, 15180, 13532)   # (test_gpu_mesh_stream_filter.py's counts)
    unfiltered, _ = twin_and_taps(rr, hip, K_, "speckle, no filter", limit=K.LIMIT, **cfg)
    assert unfiltered[2]["n_vertices"] == 13532 and unfiltered[2]["taps"][:7958].tobytes() != got[2]["taps"].tobytes()   # not the raw frame's first rows
    both, _ = twin_and_taps(rr, hip, K_, "speckle, min 100, compact", limit=K.LIMIT, min_triangles=100, index_format=rr.MESH_INDEX_TILE16, **cfg)
    assert both[2]["taps"].tobytes() == got[2]["taps"].tobytes()
    emptied, _ = twin_and_taps(rr, hip, K_, "a frame the filter empties", limit=K.LIMIT, min_triangles=1 << 20, **cfg)
    assert emptied[2]["n_vertices"] == 0 and emptied[2]["needed_vertices"] == 13532 and emptied[2]["taps"].shape == (0, 3)
    assert hip.mesh_stream_stats()["payload_bytes"] == 0
    again = stream_one(hip)                                              # ... and the slot after it
    assert again[2]["n_vertices"] == 0 and again[2]["taps"].shape == (0, 3)
    hip.close()


@pytest.mark.parametrize("slabs", [[(0, 16), (16, 35)], [(0, 8), (8, 24), (24, 35)]], ids=["two-slabs", "three-slabs"])
def test_part_rings_taps_join_to_the_whole_volume_rings_block(rr, slabs):
    K_ = case(rr, "3-streams")
    scene, N = K_["scene"], 3
    whole = rr.ReconIntegrationHip(scene, res=RES, **KW)
    whole.set_tsdf(K_["vol"])
    whole.mesh_stream_config(slots=2, index_format=rr.MESH_INDEX_TILE16, taps=True, **BIG)
    want = stream_one(whole)
    whole.close()
    ctxs = [rr.ReconIntegrationHip(scene, res=RES, slab=s, **KW) for s in slabs]
    plain_parts = []
    for c in ctxs:
        c.set_tsdf(K_["vol"])                                             # fills the slab's stored layers, halo included
        c.mesh_stream_config(slots=2, part=True, **BIG)
        plain_parts.append(stream_one(c))
        c.mesh_stream_config(slots=2, part=True, taps=True, **BIG)
    parts, joined = import_module("rgbd-recon_amd.multigpu").mesh_parts_on_one_device(ctxs, tag=7)
    for k, (p, q) in enumerate(zip(parts, plain_parts)):
        assert payload_of(p) == payload_of(q) and p[2]["part"] == q[2]["part"], k
        assert_taps(p, reference(K_, p[0]) if len(p[0]) else np.zeros((0, N), TP.PACKED_TAP_DTYPE), N, f"part {k}")
        assert ctxs[k].mesh_stream_stats()["payload_bytes"] == len(b"".join(payload_of(p))) + (-p[2]["n_vertices"] * 8 % 16) + p[2]["n_vertices"] * N * 8, k
    for c in ctxs:
        c.close()
    assert sum(p[2]["n_vertices"] > 0 for p in parts) >= 2               # (the lowest of three slabs holds no surface: a part without a tap)
    assert payload_of(joined) == payload_of(want)
    assert joined[2]["taps"].dtype == TP.PACKED_TAP_DTYPE and joined[2]["taps"].shape == want[2]["taps"].shape
    assert joined[2]["taps"].tobytes() == want[2]["taps"].tobytes()
    assert_taps(want, reference(K_, want[0]), N, "whole volume")


# ---------------------------------------------------------------------------------------------------------------- clamped coordinates and a NaN
def test_coordinates_outside_the_unit_square_are_clamped_and_a_nan_packs_as_zero(rr):
    K_ = case(rr, "3-streams")
    scene = copy.copy(K_["scene"])
    rl = [int(x) for x in scene["lut_res"]]
    # cv_uv of every stream stretched about 0.5 by 1.6: a coordinate of 0.19 becomes 0.004, one of 0.1 leaves the unit square; and one NaN texel in stream 1
    uv = [((np.asarray(a, f32) - f32(0.5)) * f32(1.6) + f32(0.5)).astype(f32).reshape(rl[2], rl[1], rl[0], 2).copy() for a in scene["cv_uv"]]
    hip0 = rr.ReconIntegrationHip(K_["scene"], res=RES, **KW)
    hip0.set_tsdf(K_["vol"])
    hip0.mesh_stream_config(slots=2, **BIG)
    vertices = stream_one(hip0)[0]
    hip0.close()
    pc = T.sensor(K_["scene"], LIMIT, TP.unit_of_codes(TP.vertex_codes(vertices)), unit_cube=True)[len(vertices) // 2, 1]   # where a vertex reads stream 1's cv_uv
    tx, ty, tz = (min(max(int(np.floor(float(c) * r)), 0), r - 1) for c, r in zip((pc["x"], pc["y"], pc["z"]), rl))
    uv[1][tz, ty, tx, 0] = np.nan
    scene["cv_uv"] = np.ascontiguousarray(np.stack(uv).reshape(np.asarray(K_["scene"]["cv_uv"]).shape), f32)
    K2 = dict(scene=scene, refs={})
    fp = TP.frame_taps_f32(scene, LIMIT, vertices)
    with np.errstate(invalid="ignore"):
        outside = ((fp["u"] < 0) | (fp["u"] > 1) | (fp["v"] < 0) | (fp["v"] > 1))
    nan = np.isnan(fp["u"]) | np.isnan(fp["v"])
    print(f"rescaled cv_uv: {outside.mean():.3f} of the pairs have a coordinate outside [0, 1], {int(nan.sum())} pairs a NaN coordinate")
    assert outside.mean() > 0.02 and nan.sum() >= 1                       # the reference alone shows that both kinds occur
    want = TP.pack_taps(fp)
    assert ((want["u"] == 0) | (want["u"] == 65535) | (want["v"] == 0) | (want["v"] == 65535))[outside].all() and (want["u"][np.isnan(fp["u"])] == 0).all()
    hip = rr.ReconIntegrationHip(scene, res=RES, **KW)
    hip.set_tsdf(K_["vol"])
    hip.mesh_stream_config(slots=2, taps=True, **BIG)
    got = stream_one(hip)
    assert got[0].tobytes() == vertices.tobytes()
    K2["refs"][(TP.vertex_codes(vertices).tobytes(), float(LIMIT))] = want
    assert_taps(got, want, 3, "rescaled cv_uv")
    hip.close()


# ---------------------------------------------------------------------------------------------------------------- the smallest counts, one stream
def small_volume(voxels, res=(32, 32, 32)):
    """everything outside but the listed voxels (x, y, z): isolated inside voxels, each crossing every lattice edge it has"""
    vol = np.full(res[::-1], -LIMIT, f32)
    for x, y, z in voxels:
        vol[z, y, x] = f32(0.5 * LIMIT)
    return vol


def test_one_stream_with_0_1_4_63_64_and_65_vertices(rr):
    """A lattice point has 14 edges inside the volume, 7 at the corners (0, 0, 0) and (31, 31, 31), 4 at the six other corners: isolated inside voxels
    give 63 = 4 * 14 + 7, 64 = 4 * 14 + 2 * 4, 65 = 3 * 14 + 7 + 4 * 4 vertices.  No whole volume has fewer than 4 (every lattice point has at least 4
    edges); ONE vertex is what the part of slab z = [0, 8) holds when the only inside voxel is (0, 0, 8): of its edges only the one from (0, 0, 7) is owned
    below the seam."""
    scene = rr.scene.make_scene(n_streams=1, width=160, height=120, lut_res=16, inv_res=24)
    K1 = dict(scene=scene, refs={})
    inner = [(5, 9, 13), (20, 6, 25), (11, 22, 4), (26, 27, 17)]
    corners4 = [(31, 0, 0), (0, 31, 0), (0, 0, 31), (31, 31, 0)]
    volumes = {0: [], 4: [(31, 0, 0)], 63: inner + [(0, 0, 0)], 64: inner + corners4[:2], 65: inner[:3] + [(31, 31, 31)] + corners4}
    hip = rr.ReconIntegrationHip(scene, res=(32, 32, 32), **KW)
    for n, voxels in volumes.items():
        vol = small_volume(voxels)
        assert len(M.extract(vol, LIMIT, scene["bbox_min"], scene["bbox_max"])["unit"]) == n
        hip.set_tsdf(vol)
        got, _ = twin_and_taps(rr, hip, K1, f"{n} vertices", max_vertices=65, max_triangles=400, max_surface_tiles=64)
        assert got[2]["n_vertices"] == n and got[2]["overflow"] == 0
    hip.close()
    slab = rr.ReconIntegrationHip(scene, res=(32, 32, 32), slab=(0, 8), **KW)
    slab.set_tsdf(small_volume([(0, 0, 8)]))
    got, _ = twin_and_taps(rr, slab, K1, "1 vertex", part=True, max_vertices=65, max_triangles=400, max_surface_tiles=64)
    assert got[2]["n_vertices"] == 1 and got[2]["taps"].shape == (1, 1)
    slab.close()


# ---------------------------------------------------------------------------------------------------------------- overflow, the slot after it, the stats
def test_an_overflowing_frame_has_no_tap_bytes_and_the_next_frame_on_its_slot_is_intact(rr):
    K_ = case(rr, "3-streams")
    N = 3
    hip = rr.ReconIntegrationHip(K_["scene"], res=RES, **KW)
    hip.set_tsdf(K_["vol"])
    hip.mesh_stream_config(slots=2, **BIG)
    first = stream_one(hip)
    nv, nt = first[2]["n_vertices"], first[2]["n_triangles"]
    more = np.array(K_["vol"])
    more[20:24, 10:14, 3:7] = f32(0.5 * LIMIT)                           # a block of inside voxels in empty space: more vertices
    more[21:23, 11:13, 4:6] = f32(-LIMIT)
    assert len(M.extract(more, LIMIT, K_["scene"]["bbox_min"], K_["scene"]["bbox_max"])["unit"]) > nv
    hip.mesh_stream_config(slots=2, taps=True, max_vertices=nv, max_triangles=1 << 16, max_surface_tiles=256)
    per_frame = nv * 8 + nt * 12 + nv * N * 8
    want = reference(K_, first[0])
    frames = []
    for f, vol in enumerate((K_["vol"], more, K_["vol"], K_["vol"])):    # slots 0, 1 (overflows), 0, 1
        hip.set_tsdf(vol)
        before = hip.mesh_stream_stats()["payload_bytes"]
        frames.append(stream_one(hip, tag=f))
        grew = hip.mesh_stream_stats()["payload_bytes"] - before
        assert grew == (0 if f == 1 else per_frame), f                   # exactly payload + n_vertices * N * 8; an overflowed frame copies nothing
    over = frames[1]
    assert over[2]["overflow"] == rr.MESH_OVERFLOW_VERTICES and over[2]["n_vertices"] == 0 and over[2]["needed_vertices"] > nv
    assert over[2]["taps"].shape == (0, N)
    for f in (0, 2, 3):
        assert frames[f][2]["overflow"] == 0 and payload_of(frames[f]) == payload_of(first), f
        assert_taps(frames[f], want, N, f"frame {f}")
    st = hip.mesh_stream_stats()
    assert st["frames"] == 4 and st["overflowed"] == 1 and st["payload_bytes"] == 3 * per_frame
    hip.close()


# ---------------------------------------------------------------------------------------------------------------- through the lanes
def test_four_frames_through_the_lanes_taken_two_late_beside_a_twin_without_a_ring(rr):
    """Two scenes alternate for four frames through tsdf_frame_dev.  The streaming context queues mesh_stream(f) with taps behind every frame and takes
    frames two late from a ring of three slots; its twin has no mesh ring.  The taps of frame f are the reference's for THAT frame's images, the pictures
    and the final volume are the twin's, and after the first call nothing is allocated."""
    import torch
    mk = dict(n_streams=2, width=160, height=120, lut_res=32, inv_res=32)
    scs = [rr.scene.make_scene(**mk), rr.scene.make_scene(**mk, sphere_c=(0.4, 0.7, -0.3), box_c=(-0.5, 1.5, 0.2))]
    raw = [[torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ("depth", "quality", "silhouette", "color")] for sc in scs]
    torch.cuda.synchronize()
    mv, pr = rr.scene.default_view(64, 36)
    frames, lag = 4, 2

    def run(stream, download):
        hip = rr.ReconIntegrationHip(scs[0], res=(32, 32, 32), **KW)
        taken, fbs, device_bytes, free = [], [], None, None
        if stream:
            hip.mesh_stream_config(normals=True, colours=True, slots=3, taps=True, **BIG)
        for f in range(frames):
            hip.frame_dev(mv, pr, [t.data_ptr() for t in raw[f % 2]])
            if stream:
                hip.mesh_stream(f)
                now = hip.mesh_stream_stats()["device_bytes"]
                device_bytes = device_bytes or now
                assert now == device_bytes > 3 * BIG["max_vertices"] * (16 + 2 * 8)          # three slots with their blocks; nothing after the first call
                if f >= lag:
                    taken.append(hip.mesh_stream_take())
            if download:
                fbs.append(hip.framebuffer()[0])                         # (a host wait: the free-running run does without)
            if f == 0:
                free = torch.cuda.mem_get_info()[0]
        lost = free - torch.cuda.mem_get_info()[0]                       # what the frames after the first took from the device (the lanes settle in frame 2)
        if stream:
            taken += [hip.mesh_stream_take() for _ in range(lag)]
        last, vol = hip.framebuffer()[0], hip.tsdf()
        hip.close()
        return taken, fbs, last, vol, lost

    free_run = run(True, False)
    streamed = run(True, True)
    twin, twin_free = run(False, True), run(False, False)
    # hipMemGetInfo: beyond what the same frames take without a ring, not a slot's worth (1.8 MiB with its block) after the first call
    assert free_run[4] - twin_free[4] < (1 << 20) and streamed[4] - twin[4] < (1 << 20), (free_run[4], twin_free[4], streamed[4], twin[4])
    same = lambda a, b: ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()
    assert same(free_run[2], twin[2]) and same(streamed[2], twin[2]) and same(free_run[3], twin[3]) and same(streamed[3], twin[3])
    Ks = [dict(scene=sc, refs={}) for sc in scs]
    for f in range(frames):
        assert same(streamed[1][f], twin[1][f]), f
        for got in (free_run[0][f], streamed[0][f]):
            assert got[2]["tag"] == f and got[2]["overflow"] == 0 and got[2]["n_vertices"] > 100, f
            assert_taps(got, reference(Ks[f % 2], got[0]), 2, f"frame {f}")
    assert free_run[0][0][2]["taps"].tobytes() != free_run[0][1][2]["taps"].tobytes()       # the two frames differ


# ---------------------------------------------------------------------------------------------------------------- the receiver
@pytest.mark.parametrize("name", list(SCENES))
def test_the_receivers_rule_on_the_unpacked_taps_is_within_half_an_8_bit_step(rr, name):
    K_ = case(rr, name)
    scene = K_["scene"]
    hip = rr.ReconIntegrationHip(scene, res=RES, **KW)
    hip.set_tsdf(K_["vol"])
    hip.mesh_stream_config(slots=2, taps=True, **BIG)
    v, _, info = stream_one(hip)
    hip.close()
    un = rr.unpack_mesh_taps(info["taps"])
    assert un.dtype == rr.TEXTURE_TAP_DTYPE and un.tobytes() == TP.unpack_taps(info["taps"]).tobytes()
    exact = rr.blend_from_taps(TP.frame_taps_f32(scene, LIMIT, v), scene["color"])
    got = rr.blend_from_taps(un, scene["color"])
    diff = np.abs(exact[:, :3].astype(np.float64) - got[:, :3].astype(np.float64))
    print(f"{name}: receiver's colour from the device's packed taps against the fp32 reference taps: max {diff.max() * 255:.3f} / 255, mean {diff.mean() * 255:.3f} / 255")
    assert (exact[:, 3] == got[:, 3]).all() and not np.isnan(diff).any()
    assert diff.max() <= COLOUR_BOUND


# ---------------------------------------------------------------------------------------------------------------- errors, states, memory
def test_every_error_code_and_the_reset_by_a_config(rr, small_scene):
    import ctypes as C
    lib = rr.load_library()
    hip = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), **KW)
    assert code(rr, lambda: hip.mesh_stream_config_taps(True)) == -4      # before a config
    assert code(rr, hip.mesh_stream_tap_flags) == -4
    assert code(rr, hip.mesh_stream_frame_taps) == -4
    hip.mesh_stream_config(slots=2, **BIG)
    assert hip.mesh_stream_tap_flags() == 0
    for bad in (2, 3, 0x80000000):
        assert code(rr, lambda: hip.mesh_stream_config_taps(bad)) == -1   # an unknown bit
    assert hip.mesh_stream_tap_flags() == 0
    assert lib.tsdf_mesh_stream_tap_flags(hip._c, None) == -1 and lib.tsdf_mesh_stream_frame_taps(hip._c, None) == -1
    assert lib.tsdf_mesh_stream_config_taps(None, C.c_uint32(1)) == -1 and lib.tsdf_mesh_stream_frame_taps(None, None) == -1
    hip.set_tsdf(M.sphere_volume((32, 32, 32), limit=LIMIT))
    hip.mesh_stream(0)
    assert code(rr, lambda: hip.mesh_stream_config_taps(True)) == -4      # a frame is queued
    assert code(rr, hip.mesh_stream_frame_taps) == -4                     # a ring without taps (and nothing held)
    hip.mesh_stream_acquire(wait=True)
    assert code(rr, lambda: hip.mesh_stream_config_taps(True)) == -4      # a frame is held
    assert code(rr, hip.mesh_stream_frame_taps) == -4                     # held, but the ring has no taps
    hip.mesh_stream_release()
    hip.mesh_stream_config_taps(True)
    assert hip.mesh_stream_tap_flags() == 1 and hip.mesh_stream_stats()["device_bytes"] == 0   # the slots were dropped: the next call allocates
    assert code(rr, hip.mesh_stream_frame_taps) == -4                     # taps, but no frame is held
    hip.mesh_stream(1)
    assert code(rr, lambda: hip.mesh_stream_config_taps(False)) == -4
    v, t, info = hip.mesh_stream_take()
    assert info["taps"].shape == (info["n_vertices"], 4) and info["n_vertices"] > 100
    with_block = hip.mesh_stream_stats()["device_bytes"]
    hip.mesh_stream_config_taps(True)                                     # no change: the slots stay
    assert hip.mesh_stream_stats()["device_bytes"] == with_block
    hip.mesh_stream_config_taps(False)
    assert hip.mesh_stream_tap_flags() == 0 and hip.mesh_stream_stats()["device_bytes"] == 0
    assert "taps" not in stream_one(hip)[2]
    assert with_block - hip.mesh_stream_stats()["device_bytes"] == 2 * BIG["max_vertices"] * 4 * 8   # out[3] counts the larger slots: two blocks
    # every config entry resets the flag
    for cfg in (dict(), dict(level=1), dict(min_triangles=5), dict(index_format=rr.MESH_INDEX_TILE16), dict(part=True)):
        hip.mesh_stream_config_taps(True)
        assert hip.mesh_stream_tap_flags() == 1
        hip.mesh_stream_config(slots=2, **BIG, **cfg)
        assert hip.mesh_stream_tap_flags() == 0, cfg
    # 4 GiB: the uint32 payload alone fits (1 + 1.5 GiB), with the block of 4 streams (4 GiB) the slot does not; the flag stays as it was
    huge = dict(max_vertices=1 << 27, max_triangles=1 << 27, max_surface_tiles=256)
    hip.mesh_stream_config(slots=2, **huge)
    assert code(rr, lambda: hip.mesh_stream_config_taps(True)) == -1 and hip.mesh_stream_tap_flags() == 0
    assert code(rr, lambda: hip.mesh_stream_config(slots=2, taps=True, **huge)) == -1
    hip.mesh_stream_config(slots=2, taps=True, **BIG)
    hip.mesh_stream_config_taps(True)
    assert hip.mesh_stream_tap_flags() == 1 and stream_one(hip)[2]["taps"].shape[1] == 4
    hip.close()

    bare = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), upload=False, **KW)      # a volume, but neither calibration nor frame
    bare.set_tsdf(M.sphere_volume((32, 32, 32), limit=LIMIT))
    bare.mesh_stream_config(slots=2, taps=True, **BIG)
    assert code(rr, lambda: bare.mesh_stream(0)) == -4 and bare.mesh_stream_stats()["frames"] == 0
    assert code(rr, bare.mesh_stream_acquire) == -4                       # nothing was queued
    bare.mesh_stream_config(slots=2, normals=True, **BIG)                 # without taps the same ring streams
    assert stream_one(bare)[2]["n_vertices"] > 100
    bare.close()


def test_device_memory_over_context_cycles(rr, small_scene):
    import torch
    vol = M.sphere_volume((32, 32, 32), limit=LIMIT)

    def cycle():
        h = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), **KW)
        h.set_tsdf(vol)
        h.mesh_stream_config(slots=3, taps=True, min_triangles=1, **BIG)
        for f in range(3):
            h.mesh_stream(f)
        assert h.mesh_stream_take()[2]["taps"].shape[0] > 100
        h.close()                                                         # two frames still queued: destroy drains the ring

    cycle()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(6):
        cycle()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < (8 << 20), f"{(free0 - free1) >> 20} MiB of device memory lost over 6 context cycles"
