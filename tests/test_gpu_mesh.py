"""GPU: the mesh extraction (tsdf_mesh_extract) against tests/mesh_reference.py, bit for bit: a random volume whose size is no multiple of the
storage tile, with zeros, -0, NaN and infinities planted; a sphere whose mesh must be a closed 2-manifold; an integrated scene, culled and in
a sparse pool; normals and colours; the lanes (the right volume set and frame slot are read, and nothing is disturbed); the PLY file; errors."""
import numpy as np
import pytest

import mesh_reference as M

pytestmark = pytest.mark.gpu

LIMIT = 0.04
KW = dict(brick_size=[2.0 / 8, 2.2 / 8, 2.0 / 8], limit=LIMIT, view=(64, 36))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def nan_equal(a, b):
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def assert_same_geometry(got, want):
    assert got["position"].shape == want["position"].shape and got["triangles"].shape == want["triangles"].shape
    assert (bits(got["position"]) == bits(want["position"])).all()
    assert got["triangles"].dtype == np.uint32
    assert (M.canonical(got["triangles"]) == M.canonical(want["triangles"])).all()       # smallest index first: keeps the winding


def assert_identical(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


@pytest.fixture(scope="module")
def scene2(rr):
    return rr.scene.make_scene(n_streams=2, width=160, height=120, lut_res=32, inv_res=32)


def integrate(hip):
    hip.clearOccupiedBricks()
    hip.markBricks()
    hip.updateOccupiedBricks()
    hip.integrate()


def test_random_volume_bit_equal_and_reproducible(rr, scene2):
    """20 x 22 x 19: padded tiles and tile borders on every axis; ~10 % exact zeros, and -0, NaN, +-inf (outside, outside, -limit, -limit)"""
    res = (20, 22, 19)
    rng = np.random.default_rng(20221019)
    vol = rng.uniform(-LIMIT, LIMIT, res[::-1]).astype(np.float32)
    vol[rng.random(vol.shape) < 0.10] = 0.0
    special = np.array([-0.0, np.nan, np.inf, -np.inf], np.float32)
    pick = rng.random(vol.shape) < 0.02
    vol[pick] = special[rng.integers(0, 4, int(pick.sum()))]
    assert (vol == 0).mean() > 0.08 and np.isnan(vol).sum() > 5 and np.isinf(vol).sum() > 5 and (np.signbit(vol) & (vol == 0)).sum() > 5
    hip = rr.ReconIntegrationHip(scene2, res=res, **KW)
    hip.set_tsdf(vol)
    got = hip.extract_mesh(normals=False, colours=False)
    want = M.extract(vol, LIMIT, scene2["bbox_min"], scene2["bbox_max"])
    print("random volume:", len(got["position"]), "vertices", len(got["triangles"]), "triangles; reference", len(want["position"]), len(want["triangles"]))
    assert len(want["position"]) > 10000 and np.isfinite(want["position"]).all()
    assert_same_geometry(got, want)
    assert (got["triangles"] == want["triangles"]).all()                # (the winding convention is the same on both sides)
    st = hip.mesh_stats()
    assert st["tiles"] == 3 * 3 * 3 and st["tiles_skipped"] == 0 and st["tiles_with_surface"] == 27
    assert st["bytes"] == got["position"].nbytes + got["triangles"].nbytes
    assert_identical(hip.extract_mesh(normals=False, colours=False), got)
    hip.close()


def test_sphere_is_a_closed_manifold(rr, scene2):
    res = (24, 16, 16)
    vol = M.sphere_volume(res, limit=LIMIT)
    hip = rr.ReconIntegrationHip(scene2, res=res, **KW)
    hip.set_tsdf(vol)
    got = hip.extract_mesh(normals=False, colours=False)
    hip.close()
    rep = M.manifold_report(got["triangles"], len(got["position"]))
    print("sphere:", rep)
    assert rep["faces"] > 1000 and rep["vertices_used"] == len(got["position"])
    assert rep["directed_unique"] and rep["edges_shared_by_two"] and rep["opposite"]
    assert rep["euler"] == 2
    assert M.signed_volume(got["position"], got["triangles"]) > 0
    assert_same_geometry(got, M.extract(vol, LIMIT, scene2["bbox_min"], scene2["bbox_max"]))


@pytest.fixture(scope="module")
def scene_mesh(rr, small_scene):
    """small_scene at 32^3, bricks on, after integrate: the dense context's mesh with every attribute, its volume, its stats, and the reference"""
    hip = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), **KW)
    integrate(hip)
    got = hip.extract_mesh(normals=True, colours=True)
    stats = hip.mesh_stats()
    vol = hip.tsdf()
    hip.close()
    want = M.extract(vol, LIMIT, small_scene["bbox_min"], small_scene["bbox_max"])
    return dict(got=got, stats=stats, vol=vol, want=want)


def test_small_scene_culled_equals_the_unskipped_reference(scene_mesh):
    got, want, st = scene_mesh["got"], scene_mesh["want"], scene_mesh["stats"]
    print("small scene:", len(got["position"]), "vertices", len(got["triangles"]), "triangles", st)
    assert len(want["position"]) > 200 and len(want["triangles"]) > 200
    assert_same_geometry(got, want)
    assert st["tiles"] == 64 and st["tiles_skipped"] > 0 and 0 < st["tiles_with_surface"] <= 64 - st["tiles_skipped"]


def test_small_scene_sparse_pool_identical_to_dense(rr, small_scene, scene_mesh):
    hip = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), sparse_pool_tiles=64, **KW)
    integrate(hip)
    got = hip.extract_mesh(normals=True, colours=True)
    st = hip.mesh_stats()
    hip.close()
    assert st["tiles_skipped"] > 0
    assert_identical(got, scene_mesh["got"])


def test_normals_and_colours_equal_the_reference(small_scene, scene_mesh):
    """Bit equality, NaN equal to NaN: normals and colours go through the same device functions as a frame pixel (get_gradient, blendColors), and
    the frame tests get bit equality for those against the same oracle primitives."""
    got, want, vol = scene_mesh["got"], scene_mesh["want"], scene_mesh["vol"]
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


def test_lanes_read_the_right_volume_set_and_disturb_nothing(rr):
    """two different frames alternating through tsdf_frame_dev: an extract after frame k equals the extract of a one-stream context after the same
    frames, and every drawn frame equals the one drawn without any extract in between"""
    import torch
    mk = dict(n_streams=2, width=160, height=120, lut_res=32, inv_res=32)
    scs = [rr.scene.make_scene(**mk), rr.scene.make_scene(**mk, sphere_c=(0.4, 0.7, -0.3), box_c=(-0.5, 1.5, 0.2))]
    raw = [[torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ("depth", "quality", "silhouette", "color")] for sc in scs]
    torch.cuda.synchronize()
    mv, pr = rr.scene.default_view(64, 36)
    frames = 5

    def run(lane_flags, extract):
        hip = rr.ReconIntegrationHip(scs[0], res=(32, 32, 32), lane_flags=lane_flags, **KW)
        meshes, fbs = [], []
        for f in range(frames):
            hip.frame_dev(mv, pr, [t.data_ptr() for t in raw[f % 2]])
            if extract:
                meshes.append(hip.extract_mesh(normals=True, colours=True))
            fbs.append(hip.framebuffer()[0])
        hip.close()
        return meshes, fbs

    lanes, lanes_fb = run(0, True)
    one, _ = run(rr.LANES_ONE_STREAM, True)
    _, plain_fb = run(0, False)
    assert len(lanes[0]["position"]) > 100 and lanes[0]["position"].tobytes() != lanes[1]["position"].tobytes()   # the two frames differ
    for f in range(frames):
        assert_identical(lanes[f], one[f])
        assert nan_equal(lanes_fb[f], plain_fb[f]).all(), f


def read_ply(path):
    """binary little-endian PLY with float vertex properties and uchar / int faces -> (names, vertex rows [V][n], faces [T][3])"""
    raw = open(path, "rb").read()
    head, body = raw[:raw.index(b"end_header\n")].decode().split("\n"), raw[raw.index(b"end_header\n") + 11:]
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    nv = int([l for l in head if l.startswith("element vertex")][0].split()[2])
    nt = int([l for l in head if l.startswith("element face")][0].split()[2])
    names = [l.split()[2] for l in head if l.startswith("property float")]
    assert "property list uchar int vertex_indices" in head
    verts = np.frombuffer(body, "<f4", nv * len(names)).reshape(nv, len(names))
    faces = np.frombuffer(body, np.dtype([("n", "u1"), ("i", "<i4", 3)]), nt, offset=verts.nbytes)
    assert verts.nbytes + faces.nbytes == len(body) and (faces["n"] == 3).all()
    return names, verts, faces["i"]


def test_ply_file_equals_the_downloads(rr, small_scene, tmp_path):
    hip = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), **KW)
    integrate(hip)
    for normals, colours in ((True, True), (False, False), (False, True)):
        mesh = hip.extract_mesh(normals=normals, colours=colours)
        path = tmp_path / f"mesh_{int(normals)}{int(colours)}.ply"
        hip.write_ply(path)
        names, verts, faces = read_ply(path)
        want_names = ["x", "y", "z"] + (["nx", "ny", "nz"] if normals else []) + (["red", "green", "blue", "alpha"] if colours else [])
        assert names == want_names
        want = np.concatenate([mesh["position"]] + ([mesh["normal"]] if normals else []) + ([mesh["colour"]] if colours else []), axis=1)
        assert len(verts) > 200 and bits(verts).tobytes() == bits(want).tobytes()
        assert (faces.astype(np.uint32) == mesh["triangles"]).all()
    hip.close()


def test_errors(rr, small_scene):
    def code(fn):
        with pytest.raises(rr.TsdfError) as e:
            fn()
        return e.value.code

    hip = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), **KW)
    assert code(lambda: hip.extract_mesh(normals=False, colours=False)) == -4          # before any integrate / volume upload
    assert code(hip.mesh_stats) == -4 and code(lambda: hip.write_ply("/nonexistent/x.ply")) == -4
    integrate(hip)
    hip.extract_mesh(normals=False, colours=False)
    assert code(lambda: hip.download_mesh(normals=True, colours=False)) == -4           # attributes the extract did not produce
    assert code(lambda: hip.download_mesh(normals=False, colours=True)) == -4
    hip.download_mesh(normals=False, colours=False)
    assert code(lambda: hip.write_ply("/nonexistent/dir/x.ply")) == -1
    hip.setVoxelSize(0.1)                                                               # a new grid: no volume, no mesh
    assert code(lambda: hip.extract_mesh(normals=False, colours=False)) == -4
    hip.close()

    bare = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), upload=False, **KW)     # a volume, but neither calibration nor frame
    bare.set_tsdf(M.sphere_volume((32, 32, 32), limit=LIMIT))
    assert code(lambda: bare.extract_mesh(normals=False, colours=True)) == -4
    assert len(bare.extract_mesh(normals=True, colours=False)["position"]) > 100
    bare.close()

    slab = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), slab=(0, 16), **KW)
    assert code(lambda: slab.extract_mesh(normals=False, colours=False)) == -4
    slab.close()
