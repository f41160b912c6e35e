"""GPU: the mesh component measures (tsdf_mesh_component_measures / _download_component_measures / _filter_components_measured) against
tests/mesh_measure_reference.py, byte for byte, on the arrays the device downloaded: the four volumes of the component tests, the 4 x 4 x 4 volume whose
triangles need more than 64 bits, a level of detail, a sparse pool; the measured filter; errors and lifetime."""
import ctypes as C

import numpy as np
import pytest

import mesh_component_reference as K
import mesh_measure_reference as R
from test_gpu_mesh import KW, integrate
from test_gpu_mesh_components import code, context

pytestmark = pytest.mark.gpu

# name -> (case of the component tests, level); S: the coarse lattice
VOLUMES = dict(A=("A", 0), B=("B", 0), C=("C", 0), D=("D", 0), D1=("D", 1), S=(None, 0))


@pytest.fixture(scope="module")
def scene2(rr):
    return rr.scene.make_scene(n_streams=2, width=160, height=120, lut_res=32, inv_res=32)


def labelled(hip, level=0):
    mesh = hip.extract_mesh(normals=False, colours=False, level=level)
    n = hip.mesh_components()
    return mesh, hip.mesh_download_components(), n


def reference(scene, mesh, comps):
    g = R.grid(scene["bbox_min"], scene["bbox_max"])
    return g, R.measures(mesh, comps["vertex_component"], comps["triangle_component"], len(comps["table"]), g)


def same_grid(got, want):
    assert got["unit"] == want["unit"] and got["bits"] == 20 and got["origin"].dtype == np.float32 and got["origin"].tobytes() == want["origin"].tobytes()


@pytest.mark.parametrize("name", list(VOLUMES))
def test_rows_equal_the_reference_and_are_reproducible(rr, scene2, name):
    case, level = VOLUMES[name]
    if case is None:
        hip = rr.ReconIntegrationHip(scene2, res=(4, 4, 4), **KW)
        hip.set_tsdf(R.random_small_volume())
    else:
        hip = context(rr, scene2, case)
    mesh, comps, n = labelled(hip, level)
    assert n >= 1 and len(mesh["triangles"]) > 100
    g = hip.mesh_component_measures()
    rows = hip.mesh_download_component_measures()
    want_g, want = reference(scene2, mesh, comps)
    same_grid(g, want_g)
    same_grid(hip.mesh_measure_grid(), want_g)
    si = rr.mesh_measures_si(rows, g, comps["table"])
    print(name, len(mesh["position"]), "vertices", len(mesh["triangles"]), "triangles", n, "components; area", si["area"][:3].tolist(), "m^2, volume",
          si["volume"][:3].tolist(), "m^3")
    assert rows.dtype == rr.MESH_COMPONENT_MEASURE_DTYPE and rows.shape == (n,)
    for field in R.ROW.names:
        assert (rows[field] == want[field]).all(), field
    assert rows.tobytes() == want.tobytes()
    if name == "S":                                                       # the wide path is taken: |e1 x e2|^2 passes 2^64 here
        assert max(R.triangle_measures(R.quantise(mesh["position"], want_g), mesh["triangles"])[0]) >= 1 << 64
    if name == "D":
        vol = rr.mesh_volume6(rows)
        assert vol[0] > 0 > vol[1] and vol[2] > 0 and abs(vol[0]) > abs(vol[1]) > abs(vol[2])
        want_si = R.si(want, want_g)
        for k in ("area", "volume"):                                      # (the two conversions multiply in another order: a few float64 roundings apart)
            assert np.abs(si[k] / want_si[k] - 1.0).max() <= 8 * np.finfo(np.float64).eps, k
        assert np.abs(si["centroid"] - [0.0, 1.1, 0.0]).max() < 0.02 and (si["bounds_min"] < si["bounds_max"]).all()
    # a second call: identical bytes; mesh, labels and table are as they were
    same_grid(hip.mesh_component_measures(), want_g)
    assert hip.mesh_download_component_measures().tobytes() == rows.tobytes()
    again, comps2 = hip.download_mesh(normals=False, colours=False), hip.mesh_download_components()
    assert again["position"].tobytes() == mesh["position"].tobytes() and again["triangles"].tobytes() == mesh["triangles"].tobytes()
    for k in ("vertex_component", "triangle_component", "table"):
        assert comps2[k].tobytes() == comps[k].tobytes(), k
    assert hip.mesh_component_stats()["components"] == n
    hip.close()


def test_sparse_pool(rr, small_scene):
    hip = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), sparse_pool_tiles=64, **KW)
    integrate(hip)
    mesh, comps, n = labelled(hip)
    assert len(mesh["triangles"]) > 200
    g = hip.mesh_component_measures()
    want_g, want = reference(small_scene, mesh, comps)
    same_grid(g, want_g)
    assert hip.mesh_download_component_measures().tobytes() == want.tobytes()
    hip.close()


def test_filter_by_area_is_not_the_filter_by_count(rr, scene2):
    hip = context(rr, scene2, "A")
    mesh, comps, n = labelled(hip)
    hip.mesh_component_measures()
    rows = hip.mesh_download_component_measures()
    rule = hip.mesh_measure_rule(min_area_m2=0.05)
    u = hip.mesh_measure_grid()["unit"]
    assert int(rule["min_area2"]) == int(np.ceil(2.0 * 0.05 / (u * u))) and int(rule["reserved"]) == 0 and int(rule["flags"]) == 0
    flags = R.keep_flags(rows, comps["table"], rule)
    by_count = comps["table"]["n_triangles"] >= 100
    print("A: kept by area", int(flags.sum()), "by count", int(by_count.sum()), "of", n)
    assert n == 343 and flags.sum() == 200 and by_count.sum() == 61      # the two rules differ on this input
    want = K.keep(mesh, flags)
    assert hip.mesh_filter_measured(rule) == (len(want["position"]), len(want["triangles"]))
    got = hip.download_mesh(normals=False, colours=False)
    assert got["position"].tobytes() == want["position"].tobytes() and got["triangles"].tobytes() == want["triangles"].tobytes()
    st = hip.mesh_component_stats()
    assert st == dict(components=0, largest_triangles=0, vertices_removed=len(mesh["position"]) - len(want["position"]),
                      triangles_removed=len(mesh["triangles"]) - len(want["triangles"]))
    assert hip.mesh_stats()["bytes"] == got["position"].nbytes + got["triangles"].nbytes
    # after a filter the measures are gone, with the labels; labelled and measured again they are those of the kept components, in order
    assert code(rr, hip.mesh_download_component_measures) == -4 and code(rr, lambda: hip.mesh_filter_measured(rule)) == -4
    assert code(rr, hip.mesh_component_measures) == -4
    assert hip.mesh_components() == 200
    assert code(rr, hip.mesh_download_component_measures) == -4          # labels alone are not measures
    hip.mesh_component_measures()
    kept = hip.mesh_download_component_measures()
    for field in ("area2", "volume6_lo", "volume6_hi", "sum_q", "q_min", "q_max"):
        assert (kept[field] == rows[field][flags]).all(), field
    # a rule of several clauses, decided on the device like the reference decides it
    rule2 = hip.mesh_measure_rule(min_triangles=30, min_extent_m=0.25, min_volume_m3=1e-4, positive_volume=True)
    flags2 = R.keep_flags(kept, hip.mesh_download_components()["table"], rule2)
    assert 0 < flags2.sum() < 200
    want2 = K.keep(got, flags2)
    assert hip.mesh_filter_measured(rule2) == (len(want2["position"]), len(want2["triangles"]))
    got2 = hip.download_mesh(normals=False, colours=False)
    assert got2["position"].tobytes() == want2["position"].tobytes() and got2["triangles"].tobytes() == want2["triangles"].tobytes()
    hip.close()


def test_positive_volume_drops_the_void_and_a_zero_rule_keeps_everything(rr, scene2):
    hip = context(rr, scene2, "D")
    mesh, comps, n = labelled(hip)
    assert n == 3
    hip.mesh_component_measures()
    # an all-zero rule: every component stays, the arrays stay in place
    assert hip.mesh_filter_measured(hip.mesh_measure_rule()) == (len(mesh["position"]), len(mesh["triangles"]))
    assert hip.mesh_component_stats()["vertices_removed"] == 0
    same = hip.download_mesh(normals=False, colours=False)
    assert same["position"].tobytes() == mesh["position"].tobytes() and same["triangles"].tobytes() == mesh["triangles"].tobytes()
    assert hip.mesh_components() == 3
    hip.mesh_component_measures()
    want = K.keep(mesh, [1, 0, 1])
    assert hip.mesh_filter_measured(hip.mesh_measure_rule(positive_volume=True)) == (len(want["position"]), len(want["triangles"]))
    got = hip.download_mesh(normals=False, colours=False)
    assert got["position"].tobytes() == want["position"].tobytes() and got["triangles"].tobytes() == want["triangles"].tobytes()
    assert hip.mesh_component_stats()["triangles_removed"] == 5968
    hip.close()


def test_errors_and_lifetime(rr, scene2, small_scene):
    lib = rr.load_library()
    hip = rr.ReconIntegrationHip(scene2, res=(40, 24, 24), **KW)
    grid = np.zeros(1, rr.MESH_MEASURE_GRID_DTYPE)
    gp = grid.ctypes.data_as(C.c_void_p)
    rows = np.zeros(8, rr.MESH_COMPONENT_MEASURE_DTYPE)
    rp = rows.ctypes.data_as(C.c_void_p)
    rule = np.zeros(1, rr.MESH_MEASURE_RULE_DTYPE)
    up = rule.ctypes.data_as(C.c_void_p)

    def all_refuse():
        assert lib.tsdf_mesh_component_measures(hip._c, gp) == -4 and lib.tsdf_mesh_component_measures(hip._c, None) == -4
        assert lib.tsdf_mesh_download_component_measures(hip._c, rp) == -4
        assert lib.tsdf_mesh_filter_components_measured(hip._c, up, None, None) == -4

    # the grid needs no mesh
    assert lib.tsdf_mesh_measure_grid_info(hip._c, gp) == 0 and grid["bits"][0] == 20 and grid["unit"][0] == R.grid(scene2["bbox_min"], scene2["bbox_max"])["unit"]
    assert lib.tsdf_mesh_measure_grid_info(hip._c, None) == -1
    all_refuse()                                                          # no volume
    hip.set_tsdf(K.shells_volume())
    all_refuse()                                                          # no extract
    mesh = hip.extract_mesh(normals=False, colours=False)
    all_refuse()                                                          # no labels yet: measures before labels
    assert lib.tsdf_mesh_download_component_measures(hip._c, None) == -1 and lib.tsdf_mesh_filter_components_measured(hip._c, None, None, None) == -1
    assert hip.mesh_components() == 3
    # labels, no measures: download and filter refuse
    assert lib.tsdf_mesh_download_component_measures(hip._c, rp) == -4 and lib.tsdf_mesh_filter_components_measured(hip._c, up, None, None) == -4
    assert lib.tsdf_mesh_component_measures(hip._c, None) == 0            # (the grid is optional)
    assert lib.tsdf_mesh_download_component_measures(hip._c, rp) == 0 and (rows["area2"][:3] > 0).all() and (rows["area2"][3:] == 0).all()
    # a bad rule changes nothing
    for field, value in (("reserved", 1), ("flags", 2), ("flags", 0x80000001)):
        bad = np.zeros(1, rr.MESH_MEASURE_RULE_DTYPE)
        bad[field] = value
        assert lib.tsdf_mesh_filter_components_measured(hip._c, bad.ctypes.data_as(C.c_void_p), None, None) == -1
    assert lib.tsdf_mesh_download_component_measures(hip._c, rp) == 0 and hip.mesh_component_stats()["components"] == 3
    # a new labelling of the same mesh releases the measures; so does a new extract
    assert hip.mesh_components() == 3
    assert code(rr, hip.mesh_download_component_measures) == -4
    hip.mesh_component_measures()
    first = hip.mesh_download_component_measures()
    again = hip.extract_mesh(normals=False, colours=False)
    assert again["triangles"].tobytes() == mesh["triangles"].tobytes()
    all_refuse()
    hip.mesh_components()
    hip.mesh_component_measures()
    assert hip.mesh_download_component_measures().tobytes() == first.tobytes()
    # the plain keep releases them too
    hip.mesh_keep([1, 0, 1])
    all_refuse()
    hip.setVoxelSize(0.1)                                                 # a new grid: no volume, no mesh, no labels, no measures
    all_refuse()
    assert lib.tsdf_mesh_measure_grid_info(hip._c, gp) == 0
    hip.close()
    assert lib.tsdf_mesh_component_measures(None, gp) == -1 and lib.tsdf_mesh_download_component_measures(None, rp) == -1
    assert lib.tsdf_mesh_measure_grid_info(None, gp) == -1 and lib.tsdf_mesh_filter_components_measured(None, up, None, None) == -1

    slab = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), slab=(0, 16), **KW)           # a Z-slab context extracts no mesh
    assert code(rr, slab.mesh_component_measures) == -4 and code(rr, slab.mesh_download_component_measures) == -4
    assert code(rr, lambda: slab.mesh_filter_measured(slab.mesh_measure_rule(min_extent_m=0.05))) == -4
    assert slab.mesh_measure_grid()["bits"] == 20
    slab.close()
