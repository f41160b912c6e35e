"""CPU: known answers of tests/mesh_component_reference.py -- two hand-made meshes, the four test volumes' counts, and the numpy labelling against a plain
sequential union-find."""
import numpy as np
import pytest

import mesh_component_reference as K
import mesh_reference as M

BBOX = (np.array([-1.0, 0.0, -1.0], np.float32), np.array([1.0, 2.2, 1.0], np.float32))   # (the counts are topological: any box gives them)


def test_two_triangles_sharing_one_vertex_are_one_component():
    tri = np.array([[0, 1, 2], [2, 3, 4]], np.uint32)
    vc, tc, table = K.components(tri, 5)
    assert vc.dtype == tc.dtype == np.uint32 and table.dtype == K.TABLE and table.itemsize == 16
    assert vc.tolist() == [0] * 5 and tc.tolist() == [0, 0]
    assert table.tolist() == [(0, 5, 2, 0)]


def test_two_disjoint_triangles_and_an_unused_vertex_are_three():
    tri = np.array([[5, 1, 3], [0, 4, 2]], np.uint32)                     # vertex 6 is used by nothing
    vc, tc, table = K.components(tri, 7)
    assert vc.tolist() == [0, 1, 0, 1, 0, 1, 2] and tc.tolist() == [1, 0]
    assert table.tolist() == [(0, 3, 1, 0), (1, 3, 1, 0), (6, 1, 0, 0)]
    kept = K.keep(dict(position=np.arange(21, dtype=np.float32).reshape(7, 3), triangles=tri), [0, 1, 1])
    assert kept["position"][:, 0].tolist() == [3.0, 9.0, 15.0, 18.0] and kept["triangles"].tolist() == [[2, 0, 1]]
    none = K.keep(dict(position=np.zeros((7, 3), np.float32), triangles=tri), [0, 0, 0])
    assert none["position"].shape == (0, 3) and none["triangles"].shape == (0, 3) and none["triangles"].dtype == np.uint32


@pytest.fixture(scope="module")
def meshes():
    vols = dict(A=K.speckle_volume(), B=K.random_volume(), C=K.snakes_volume(), D=K.shells_volume())
    return {k: M.extract(v, K.LIMIT, *BBOX) for k, v in vols.items()}


def test_the_four_volumes_give_the_stated_counts(meshes):
    got = {}
    for name, mesh in meshes.items():
        vc, tc, table = K.components(mesh["triangles"], len(mesh["position"]))
        got[name] = (len(mesh["position"]), len(mesh["triangles"]), len(table))
        assert table["n_vertices"].sum() == len(vc) and table["n_triangles"].sum() == len(tc)
        assert (vc[mesh["triangles"]] == tc[:, None]).all()              # all three vertices of a triangle agree
        assert (table["first_vertex"] == [np.flatnonzero(vc == c)[0] for c in range(len(table))]).all()
    assert got["A"] == (13532, 24420, 343) and got["B"] == (26312, 52714, 8) and got["C"] == (12800, 25592, 2)
    assert got["D"][2] == 3

    a = K.components(meshes["A"]["triangles"], 13532)[2]
    assert a["n_triangles"].max() == 1412 and a["n_triangles"].min() == 2
    big = a["n_triangles"] >= 100
    assert big.sum() == 61 and a["n_vertices"][big].sum() == 7958 and a["n_triangles"][big].sum() == 15180
    kept = K.keep(meshes["A"], big)
    assert kept["position"].shape == (7958, 3) and kept["triangles"].shape == (15180, 3)
    again = K.components(kept["triangles"], 7958)[2]
    assert len(again) == 61 and (again["n_triangles"] == a["n_triangles"][big]).all()

    assert K.components(meshes["B"]["triangles"], 26312)[2]["n_triangles"].max() == 52334
    c = K.components(meshes["C"]["triangles"], 12800)[2]
    assert c["first_vertex"].tolist() == [0, 6400] and c["n_triangles"].tolist() == [12796, 12796]
    rep = M.manifold_report(meshes["C"]["triangles"], 12800)
    assert rep["directed_unique"] and rep["edges_shared_by_two"] and rep["opposite"] and rep["euler"] == 4
    d = K.components(meshes["D"]["triangles"], len(meshes["D"]["position"]))[2]
    assert d["first_vertex"].tolist() == [0, 317, 5161] and d["n_triangles"].tolist() == [15192, 5968, 1320]
    for comp in range(3):
        one = K.keep(meshes["D"], np.arange(3) == comp)
        rep = M.manifold_report(one["triangles"], len(one["position"]))
        assert rep["edges_shared_by_two"] and rep["opposite"] and rep["euler"] == 2, comp


def test_numpy_labelling_equals_a_sequential_union_find(meshes):
    for name in ("A", "C"):
        tri, nv = meshes[name]["triangles"], len(meshes[name]["position"])
        assert (K.labels(tri, nv) == K.labels_sequential(tri, nv)).all(), name
