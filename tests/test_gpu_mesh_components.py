"""GPU: the mesh components (tsdf_mesh_components / _keep_components / _filter_components) against tests/mesh_component_reference.py, byte for byte, on
the arrays the device downloaded: a speckle of hundreds of blobs, the random volume of test_gpu_mesh.py, two tubes that cross every tile back and forth,
nested shells; the filtered mesh and its attributes; a level of detail; errors and lifetime."""
import ctypes as C

import numpy as np
import pytest

import mesh_component_reference as K
import mesh_reference as M
from test_gpu_mesh import KW, nan_equal, read_ply

pytestmark = pytest.mark.gpu

# name -> (volume, res, vertices, triangles, components, triangles of the largest)
CASES = dict(A=(K.speckle_volume, (20, 22, 19), 13532, 24420, 343, 1412), B=(K.random_volume, (20, 22, 19), 26312, 52714, 8, 52334),
             C=(K.snakes_volume, (40, 24, 24), 12800, 25592, 2, 12796), D=(K.shells_volume, (40, 24, 24), None, None, 3, 15192))


@pytest.fixture(scope="module")
def scene2(rr):
    return rr.scene.make_scene(n_streams=2, width=160, height=120, lut_res=32, inv_res=32)


def context(rr, scene, name, **kw):
    make, res = CASES[name][:2]
    hip = rr.ReconIntegrationHip(scene, res=res, **KW, **kw)
    hip.set_tsdf(make())
    return hip


def same_components(got, want):
    for g, w, what in zip((got["vertex_component"], got["triangle_component"], got["table"]), want, ("vertex_component", "triangle_component", "table")):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), what


def code(rr, fn):
    with pytest.raises(rr.TsdfError) as e:
        fn()
    return e.value.code


@pytest.mark.parametrize("name", list(CASES))
def test_components_equal_the_reference_and_are_reproducible(rr, scene2, name):
    _, _, nv, nt, nc, largest = CASES[name]
    hip = context(rr, scene2, name)
    mesh = hip.extract_mesh(normals=False, colours=False)
    assert hip.mesh_components() == nc
    got = hip.mesh_download_components()
    st = hip.mesh_component_stats()
    want = K.components(mesh["triangles"], len(mesh["position"]))
    print(name, len(mesh["position"]), "vertices", len(mesh["triangles"]), "triangles", st, "representatives", got["table"]["first_vertex"][:4].tolist())
    if nv is not None:
        assert (len(mesh["position"]), len(mesh["triangles"])) == (nv, nt)
    same_components(got, want)
    assert st == dict(components=nc, largest_triangles=largest, vertices_removed=0, triangles_removed=0)
    assert (got["table"]["n_triangles"] > 0).all()                      # the extraction leaves no unused vertex
    if name == "C":
        assert got["table"]["first_vertex"].tolist() == [0, 6400] and got["table"]["n_triangles"].tolist() == [12796, 12796]
    if name == "D":
        assert got["table"]["first_vertex"].tolist() == [0, 317, 5161] and got["table"]["n_triangles"].tolist() == [15192, 5968, 1320]
    # a second labelling: identical bytes; and the extract's own arrays are as they were
    assert hip.mesh_components() == nc
    same_components(hip.mesh_download_components(), (got["vertex_component"], got["triangle_component"], got["table"]))
    again = hip.download_mesh(normals=False, colours=False)
    assert again["position"].tobytes() == mesh["position"].tobytes() and again["triangles"].tobytes() == mesh["triangles"].tobytes()
    hip.close()


def test_filter_drops_the_small_components(rr, scene2):
    hip = context(rr, scene2, "A")
    mesh = hip.extract_mesh(normals=False, colours=False)
    tiles = hip.mesh_stats()
    hip.mesh_components()
    table = hip.mesh_download_components()["table"]
    want = K.keep(mesh, table["n_triangles"] >= 100)
    assert hip.mesh_filter(100) == (7958, 15180)
    got = hip.download_mesh(normals=False, colours=False)
    assert got["position"].shape == (7958, 3) and got["triangles"].shape == (15180, 3) and got["triangles"].dtype == np.uint32
    assert got["position"].tobytes() == want["position"].tobytes() and got["triangles"].tobytes() == want["triangles"].tobytes()
    st = hip.mesh_stats()
    assert st["bytes"] == got["position"].nbytes + got["triangles"].nbytes
    assert {k: st[k] for k in ("tiles", "tiles_skipped", "tiles_with_surface")} == {k: tiles[k] for k in ("tiles", "tiles_skipped", "tiles_with_surface")}
    assert hip.mesh_component_stats() == dict(components=0, largest_triangles=0, vertices_removed=5574, triangles_removed=9240)
    assert hip.mesh_components() == 61
    comps = hip.mesh_download_components()
    assert (comps["table"]["n_triangles"] >= 100).all()
    same_components(comps, K.components(got["triangles"], len(got["position"])))
    assert (comps["table"]["n_triangles"] == table["n_triangles"][table["n_triangles"] >= 100]).all()
    # filtering again removes nothing
    assert hip.mesh_filter(100) == (7958, 15180)
    assert hip.mesh_component_stats()["vertices_removed"] == 0 and hip.mesh_component_stats()["triangles_removed"] == 0
    again = hip.download_mesh(normals=False, colours=False)
    assert again["position"].tobytes() == got["position"].tobytes() and again["triangles"].tobytes() == got["triangles"].tobytes()
    hip.close()


def test_keep_largest_one_component_and_nothing(rr, scene2, tmp_path):
    hip = context(rr, scene2, "D")

    def fresh():
        mesh = hip.extract_mesh(normals=False, colours=False)
        assert hip.mesh_components() == 3
        return mesh

    mesh = fresh()
    assert hip.mesh_keep_largest(1)[1] == 15192
    got = hip.download_mesh(normals=False, colours=False)
    rep = M.manifold_report(got["triangles"], len(got["position"]))
    print("largest shell:", rep)
    assert rep["faces"] == 15192 and rep["vertices_used"] == len(got["position"])
    assert rep["directed_unique"] and rep["edges_shared_by_two"] and rep["opposite"] and rep["euler"] == 2
    assert M.signed_volume(got["position"], got["triangles"]) > 0
    want = K.keep(mesh, [1, 0, 0])
    assert got["position"].tobytes() == want["position"].tobytes() and got["triangles"].tobytes() == want["triangles"].tobytes()

    mesh = fresh()
    assert hip.mesh_keep([0, 0, 1])[1] == 1320
    got, want = hip.download_mesh(normals=False, colours=False), K.keep(mesh, [0, 0, 1])
    assert got["position"].tobytes() == want["position"].tobytes() and got["triangles"].tobytes() == want["triangles"].tobytes()
    fresh()
    assert hip.mesh_keep_largest(2)[1] == 15192 + 5968                  # ties aside, the two largest: components 0 and 1

    fresh()
    assert hip.mesh_keep([0, 0, 0]) == (0, 0)
    got = hip.download_mesh(normals=False, colours=False)
    assert got["position"].shape == (0, 3) and got["triangles"].shape == (0, 3)
    assert hip.mesh_stats()["bytes"] == 0
    hip.write_ply(tmp_path / "empty.ply")
    names, verts, faces = read_ply(tmp_path / "empty.ply")
    assert names == ["x", "y", "z"] and len(verts) == 0 and len(faces) == 0
    assert hip.mesh_components() == 0                                   # the empty mesh has no component
    assert hip.mesh_keep(np.zeros(0, np.uint8)) == (0, 0)
    hip.close()


def test_attributes_move_with_their_vertices_and_the_taps_are_released(rr, small_scene, tmp_path):
    hip = context(rr, small_scene, "A")
    mesh = hip.extract_mesh(normals=True, colours=True)
    hip.mesh_texture_taps()
    hip.mesh_components()
    comps = hip.mesh_download_components()
    kv = (comps["table"]["n_triangles"] >= 100)[comps["vertex_component"]]
    assert hip.mesh_filter(100) == (7958, 15180)
    got = hip.download_mesh(normals=True, colours=True)
    assert got["position"].tobytes() == mesh["position"][kv].tobytes()
    assert got["normal"].shape == (7958, 3) and nan_equal(got["normal"], mesh["normal"][kv]).all()
    assert got["colour"].shape == (7958, 4) and nan_equal(got["colour"], mesh["colour"][kv]).all()
    assert (got["colour"][:, 3] > 0).sum() > 100                         # the scene does colour the surface
    assert hip.mesh_stats()["bytes"] == sum(got[k].nbytes for k in ("position", "normal", "colour", "triangles"))
    hip.write_ply(tmp_path / "filtered.ply")
    names, verts, faces = read_ply(tmp_path / "filtered.ply")
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "alpha"] and len(verts) == 7958 and len(faces) == 15180
    assert (faces.astype(np.uint32) == got["triangles"]).all()
    # the taps belonged to the unfiltered mesh
    assert code(rr, lambda: hip.mesh_download_texture_taps(7958)) == -4
    taps = hip.mesh_texture_taps()
    assert taps.shape == (7958, small_scene["n"]) and taps.tobytes() == hip.texture_taps(got["position"]).tobytes()
    hip.close()


def test_level_of_detail(rr, scene2):
    hip = context(rr, scene2, "D")
    mesh = hip.extract_mesh(normals=False, colours=False, level=1)
    n = hip.mesh_components()
    got = hip.mesh_download_components()
    print("shells at level 1:", len(mesh["position"]), "vertices", len(mesh["triangles"]), "triangles", n, "components", got["table"].tolist()[:8])
    assert len(mesh["triangles"]) > 1000 and n >= 1
    same_components(got, K.components(mesh["triangles"], len(mesh["position"])))
    want = K.keep(mesh, got["table"]["n_triangles"] == got["table"]["n_triangles"].max())
    hip.mesh_keep_largest(1)
    kept = hip.download_mesh(normals=False, colours=False)
    assert kept["position"].tobytes() == want["position"].tobytes() and kept["triangles"].tobytes() == want["triangles"].tobytes()
    hip.close()


def test_errors_and_lifetime(rr, scene2, small_scene):
    lib = rr.load_library()
    hip = rr.ReconIntegrationHip(scene2, res=(40, 24, 24), **KW)
    nv, nt, out = C.c_uint64(), C.c_uint64(), (C.c_uint64 * 4)()
    keep = (C.c_uint8 * 4)(1, 1, 1, 1)
    for no_mesh in (True, False):                                       # before any volume, then with a volume but no extract
        assert lib.tsdf_mesh_components(hip._c, C.byref(nv)) == -4
        assert lib.tsdf_mesh_download_components(hip._c, None, None, None) == -4
        assert lib.tsdf_mesh_keep_components(hip._c, keep, None, None) == -4
        assert lib.tsdf_mesh_filter_components(hip._c, C.c_uint32(1), None, None) == -4
        assert lib.tsdf_mesh_component_stats(hip._c, out) == -4
        assert lib.tsdf_mesh_keep_components(hip._c, None, None, None) == -1
        assert lib.tsdf_mesh_component_stats(hip._c, None) == -1
        if no_mesh:
            hip.set_tsdf(K.shells_volume())
    # an extract, but no components yet
    mesh = hip.extract_mesh(normals=False, colours=False)
    assert lib.tsdf_mesh_download_components(hip._c, None, None, None) == -4
    assert lib.tsdf_mesh_keep_components(hip._c, keep, None, None) == -4
    assert lib.tsdf_mesh_filter_components(hip._c, C.c_uint32(1), None, None) == -4
    assert lib.tsdf_mesh_keep_components(hip._c, None, None, None) == -1
    assert hip.mesh_component_stats() == dict(components=0, largest_triangles=0, vertices_removed=0, triangles_removed=0)
    assert code(rr, hip.mesh_download_components) == -4 and code(rr, lambda: hip.mesh_keep_largest(1)) == -4
    assert lib.tsdf_mesh_components(hip._c, None) == 0                  # (the count is optional)
    assert lib.tsdf_mesh_keep_components(hip._c, None, None, None) == -1 and hip.mesh_component_stats()["components"] == 3
    with pytest.raises(ValueError):
        hip.mesh_keep([1, 1])
    # a new extract invalidates them, and forgets what a filter removed
    assert hip.mesh_filter(2000)[1] == 15192 + 5968 and hip.mesh_component_stats()["triangles_removed"] == 1320
    assert code(rr, hip.mesh_download_components) == -4                 # ... and so does a filter
    assert code(rr, lambda: hip.mesh_filter(1)) == -4 and code(rr, lambda: hip.mesh_keep([1, 1])) == -4
    assert hip.mesh_components() == 2
    again = hip.extract_mesh(normals=False, colours=False)
    assert again["triangles"].tobytes() == mesh["triangles"].tobytes()
    assert code(rr, hip.mesh_download_components) == -4 and code(rr, lambda: hip.mesh_filter(1)) == -4
    assert hip.mesh_component_stats() == dict(components=0, largest_triangles=0, vertices_removed=0, triangles_removed=0)
    assert hip.mesh_components() == 3
    hip.setVoxelSize(0.1)                                               # a new grid: no volume, no mesh, no components
    assert code(rr, hip.mesh_components) == -4 and code(rr, hip.mesh_component_stats) == -4
    hip.close()
    assert lib.tsdf_mesh_components(None, None) == -1 and lib.tsdf_mesh_component_stats(None, out) == -1

    slab = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), slab=(0, 16), **KW)           # a Z-slab context extracts no mesh
    assert code(rr, slab.mesh_components) == -4 and code(rr, lambda: slab.mesh_filter(1)) == -4 and code(rr, slab.mesh_component_stats) == -4
    slab.close()


def test_contexts_release_their_device_memory(rr, scene2):
    """create, label, filter, label again, close: free device memory after six such cycles equals what it was after the first"""
    import torch
    vol = K.speckle_volume((96, 96, 96), seed=11)                        # ~1.7 M vertices: labels, table and filtered arrays of tens of MiB

    def cycle():
        h = rr.ReconIntegrationHip(scene2, res=(96, 96, 96), **KW)
        h.set_tsdf(vol)
        h.extract_mesh(normals=True, colours=False)
        n = h.mesh_components()
        assert n > 1000 and h.mesh_filter(50)[0] > 0
        assert 0 < h.mesh_components() < n
        h.close()

    cycle()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(6):
        cycle()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < (8 << 20), f"{(free0 - free1) >> 20} MiB of device memory lost over 6 context cycles"
