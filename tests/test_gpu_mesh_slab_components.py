"""GPU: mesh components on Z-slab contexts (tsdf_mesh_slab_components / _component_seam / _link_components / _download_components and the host merge) --
the labels of contiguous slabs' parts, concatenated in slab order, against the whole-volume context's tsdf_mesh_components and against
tests/mesh_slab_component_reference.py, byte for byte; the exported down / up / root lists and the merged links against the reference's.  Columns
that only another slab joins, speckle, a crafted volume with NaN, infinities, 0 and -0 in the seam planes, levels 1 and 2, the one-slab case, the
integrated scene with exchanged and recomputed halos and in a sparse pool, errors and lifetime, two runs.
tests/test_mesh_slab_component_reference.py asserts on the CPU that none of the cases is vacuous."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import mesh_slab_component_reference as R
import mesh_slab_reference as S

pytestmark = pytest.mark.gpu

LIMIT = R.LIMIT                                                          # the halo is one tile layer at every resolution used here
KW = dict(brick_size=[2.0 / 8, 2.2 / 8, 2.0 / 8], limit=LIMIT, view=(64, 36))
KEYS = ("vertex_component", "triangle_component", "table")
IDS = ["%s-%dx%dx%d-L%d-%dslabs" % (k, *r, l, len(s)) for k, r, l, s in R.CASES]


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


def assert_same(got, want, keys=KEYS):
    for k in keys:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert got[k].tobytes() == want[k].tobytes(), k


@pytest.fixture(scope="module")
def scene2(rr):
    return rr.scene.make_scene(n_streams=2, width=160, height=120, lut_res=32, inv_res=32)


def whole_components(rr, scene, vol, res, level):
    hip = rr.ReconIntegrationHip(scene, res=res, **KW)
    hip.set_tsdf(vol)
    mesh = hip.extract_mesh(normals=False, colours=False, level=level)
    n = hip.mesh_components()
    want = hip.mesh_download_components()
    hip.close()
    return mesh, n, want


def slab_contexts(rr, scene, vol, res, slabs):
    ctxs = [rr.ReconIntegrationHip(scene, res=res, slab=s, **KW) if len(slabs) > 1 else rr.ReconIntegrationHip(scene, res=res, **KW) for s in slabs]
    for c in ctxs:
        c.set_tsdf(vol)                                                  # fills the slab's stored layers, halo included
    return ctxs


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_joined_parts_equal_the_whole_volume_and_the_reference(rr, scene2, i):
    kind, res, level, slabs = R.CASES[i]
    vol = R.case_volume(kind, res, slabs, LIMIT)
    ref, parts = S.split(vol, LIMIT, scene2["bbox_min"], scene2["bbox_max"], level, slabs)
    run = R.components_of_parts(ref, parts, level)
    mesh, n, want = whole_components(rr, scene2, vol, res, level)
    ctxs = slab_contexts(rr, scene2, vol, res, slabs)
    joined = mgpu().mesh_slabs_on_one_device(ctxs, normals=False, colours=False, level=level)
    got = mgpu().mesh_components_on_one_device(ctxs)
    stats = [c.mesh_slab_component_stats() for c in ctxs]
    second_run = mgpu().mesh_components_on_one_device(ctxs, native=False)    # step 1 again on the same link, the numpy twin's merge
    for c in ctxs:
        c.close()
    print(IDS[i], "components:", n, "parts:", got["counts"], "stats:", stats)
    assert joined["triangles"].tobytes() == mesh["triangles"].tobytes() == ref["triangles"].tobytes()
    assert n == got["n_components"] == run["merged"]["n_components"] and n >= 1
    assert_same(got, want)                                                # the joined parts and the whole-volume context
    assert_same(got, dict(zip(KEYS, run["joined"])))                      # ... and the numpy reference
    assert_same(second_run, want)
    for k, lab in enumerate(run["labs"]):                                 # the lists, the links and every part's own arrays
        assert got["counts"][k] == dict(local_components=lab["n_local"], down=len(lab["down"]), up=len(lab["up"]), roots=len(lab["roots"])), k
        for name in ("down", "up", "roots"):
            assert got["lists"][k][name].dtype.itemsize == lab[name].dtype.itemsize and got["lists"][k][name].tobytes() == lab[name].tobytes(), (k, name)
        assert got["merged"]["links"][k].tobytes() == run["merged"]["links"][k].tobytes() and got["merged"]["component_base"][k] == run["merged"]["component_base"][k], k
        assert_same(got["parts"][k], dict(zip(KEYS, run["results"][k])))
        removed = int((run["merged"]["links"][k]["final_root"] != run["merged"]["links"][k]["root"]).sum())
        assert stats[k] == dict(local_components=lab["n_local"], owned=len(run["results"][k][2]), seam_records=len(lab["down"]) + len(lab["up"]), roots_removed=removed), k
    if len(slabs) > 1:                                                    # not vacuous here either: components cross the seams, local roots go
        assert sum(s["roots_removed"] for s in stats) > 0 and sum(s["seam_records"] for s in stats) > 0


# ---- the integrated scene
@pytest.fixture(scope="module")
def scene_whole(rr, small_scene):
    hip = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), **KW)
    integrate(hip)
    mesh = hip.extract_mesh(normals=True, colours=True)
    n = hip.mesh_components()
    out = dict(hip.mesh_download_components(), triangles=mesh["triangles"], n=n)
    hip.close()
    assert len(mesh["position"]) > 200 and len(mesh["triangles"]) > 200 and n >= 1
    return out


@pytest.mark.parametrize("halo,sparse", [("exchange", 0), ("recompute", 0), ("recompute", 512)])
def test_small_scene_two_slabs_equal_the_whole_volume(rr, small_scene, scene_whole, halo, sparse):
    m = mgpu()
    mv, pr = rr.scene.default_view(*KW["view"])
    slabs = [rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), slab=s, recompute_halo=(halo == "recompute"), sparse_pool_tiles=sparse, **KW)
             for s in ((0, 16), (16, 32))]
    m.frame_slabs_on_one_device(slabs, mv, pr, "cuda:0", halo=halo, composite="compact" if sparse else "dense")   # integrates; the halos are current
    joined = m.mesh_slabs_on_one_device(slabs, normals=True, colours=True)
    got = m.mesh_components_on_one_device(slabs)
    print("small scene,", halo, "sparse" if sparse else "dense", "components:", got["n_components"], "parts:", got["counts"])
    assert joined["triangles"].tobytes() == scene_whole["triangles"].tobytes()
    assert got["n_components"] == scene_whole["n"] and got["counts"][0]["up"] > 0 and got["counts"][1]["down"] > 0
    assert_same(got, scene_whole)
    for s in slabs:
        s.close()


# ---- errors, lifetime, determinism
def test_errors_and_lifetime(rr, scene2):
    kind, res, level, slabs = R.CASES[1]                                  # the columns in two slabs
    vol = R.case_volume(kind, res, slabs, LIMIT)
    ref, parts = S.split(vol, LIMIT, scene2["bbox_min"], scene2["bbox_max"], level, slabs)
    run = R.components_of_parts(ref, parts, level)
    lib = rr.load_library()
    low, top = slab_contexts(rr, scene2, vol, res, slabs)
    # before an extract, and before a link
    assert code(rr, low.mesh_slab_components) == -4 and code(rr, low.mesh_slab_component_stats) == -4
    nv, nt = low.extract_mesh_slab(False, False)
    top.extract_mesh_slab(False, False)
    seam = top.mesh_slab_seam()
    assert code(rr, low.mesh_slab_components) == -4
    assert lib.tsdf_mesh_slab_component_seam(low._c, None, None, None) == -4
    assert lib.tsdf_mesh_slab_link_components(low._c, C.c_uint64(0), None, C.c_uint64(0), None) == -4
    assert lib.tsdf_mesh_slab_download_components(low._c, None, None, None) == -4
    assert code(rr, low.mesh_slab_component_seam) == -4 and code(rr, low.mesh_slab_download_components) == -4
    assert low.mesh_slab_component_stats() == dict(local_components=0, owned=0, seam_records=0, roots_removed=0)
    low.mesh_slab_link(0, seam)
    top.mesh_slab_link(nv, None)
    # step 1; NULL out; before step 3
    assert lib.tsdf_mesh_slab_components(low._c, None) == -1
    assert lib.tsdf_mesh_slab_component_seam(low._c, None, None, None) == -4            # (the refused call labelled nothing)
    counts = [c.mesh_slab_components() for c in (low, top)]
    assert counts[0]["up"] > 0 and counts[0]["down"] == 0 and counts[1]["down"] > 0 and counts[1]["up"] == 0
    assert lib.tsdf_mesh_slab_download_components(low._c, None, None, None) == -4
    assert code(rr, low.mesh_slab_download_components) == -4
    assert low.mesh_slab_component_stats()["owned"] == 0
    lists = [dict(vertex_base=lab["vertex_base"], n_vertices=lab["n_vertices"], n_local=n["local_components"], **c.mesh_slab_component_seam())
             for lab, n, c in zip(run["labs"], counts, (low, top))]
    merged = rr.merge_mesh_component_seams(lists, native=True)
    good = merged["links"][1]
    assert len(good) >= 2 and (good["final_root"] < lists[1]["vertex_base"]).any()
    # bad links are refused before any launch, with the labels intact
    own_not_exported = np.setdiff1d(np.arange(lists[1]["vertex_base"], good["root"][-1]), lists[1]["roots"]["root"])   # own vertices below the last root
    assert len(own_not_exported) > 0

    def broken(field, value):
        bad = good.copy()
        bad[field][-1] = value
        return bad
    for what, bad in (("one link less", good[:-1]), ("one link more", np.concatenate([good, good[-1:]])), ("another root", broken("root", good["root"][-1] + 1)),
                      ("a final root above the root", broken("final_root", good["root"][-1] + 1)),
                      ("a final root that is an own vertex but no exported root", broken("final_root", own_not_exported[-1]))):
        assert code(rr, lambda: top.mesh_slab_link_components(merged["component_base"][1], bad)) == -1, what
    assert lib.tsdf_mesh_slab_link_components(top._c, C.c_uint64(0), None, C.c_uint64(len(good)), None) == -1   # NULL links with n_links > 0
    again = top.mesh_slab_component_seam()
    for name in ("down", "up", "roots"):
        assert again[name].tobytes() == lists[1][name].tobytes()
    assert top.mesh_slab_component_stats()["owned"] == 0 and lib.tsdf_mesh_slab_download_components(top._c, None, None, None) == -4
    # step 3, then a refused link leaves its results as they are
    for k, c in enumerate((low, top)):
        assert c.mesh_slab_link_components(merged["component_base"][k], merged["links"][k]) == len(run["results"][k][2])
    assert code(rr, lambda: top.mesh_slab_link_components(merged["component_base"][1], good[:-1])) == -1
    for k, c in enumerate((low, top)):
        assert_same(c.mesh_slab_download_components(), dict(zip(KEYS, run["results"][k])))
    assert lib.tsdf_mesh_slab_component_stats(low._c, None) == -1
    # the whole-volume entry keeps refusing on a slab context
    assert code(rr, low.mesh_components) == -4 and lib.tsdf_mesh_components(top._c, None) == -4
    # a second link drops the labels: they held the indices of the link that was
    low.mesh_slab_link(1000, seam)
    assert lib.tsdf_mesh_slab_component_seam(low._c, None, None, None) == -4 and lib.tsdf_mesh_slab_download_components(low._c, None, None, None) == -4
    assert code(rr, low.mesh_slab_component_seam) == -4
    assert low.mesh_slab_component_stats() == dict(local_components=0, owned=0, seam_records=0, roots_removed=0)
    shifted = low.mesh_slab_components()                                  # ... and the new link's labels carry its base
    assert shifted == counts[0] and (low.mesh_slab_component_seam()["up"]["vertex"].astype(np.int64) - lists[0]["up"]["vertex"] == 1000).all()
    # a new extract drops them too
    top.extract_mesh_slab(False, False)
    assert lib.tsdf_mesh_slab_component_seam(top._c, None, None, None) == -4 and code(rr, top.mesh_slab_components) == -4
    low.close()
    top.close()


def test_an_empty_part_and_a_new_grid(rr, scene2):
    res = (32, 32, 32)
    empty = rr.ReconIntegrationHip(scene2, res=res, slab=(16, 32), **KW)
    empty.set_tsdf(np.full(res[::-1], -LIMIT, np.float32))
    assert empty.extract_mesh_slab(False, False) == (0, 0)
    empty.mesh_slab_link(123, None)
    assert empty.mesh_slab_components() == dict(local_components=0, down=0, up=0, roots=0)
    assert all(len(v) == 0 for v in empty.mesh_slab_component_seam().values())
    assert empty.mesh_slab_link_components(7, np.zeros(0, rr.MESH_COMPONENT_LINK_DTYPE)) == 0
    assert all(len(v) == 0 for v in empty.mesh_slab_download_components().values())
    assert code(rr, lambda: empty.mesh_slab_link_components(7, np.zeros(1, rr.MESH_COMPONENT_LINK_DTYPE))) == -1
    assert empty.mesh_slab_component_stats() == dict(local_components=0, owned=0, seam_records=0, roots_removed=0)
    empty.close()
    # a new grid: the labels went with the part (a slab context keeps its grid: the one-slab case shows it)
    one = rr.ReconIntegrationHip(scene2, res=res, **KW)
    one.set_tsdf(R.case_volume("speckle", res, [(0, 32)], LIMIT))
    mgpu().mesh_slabs_on_one_device([one], normals=False, colours=False)
    assert mgpu().mesh_components_on_one_device([one])["n_components"] > 100
    one.setVoxelSize(0.1)
    lib = rr.load_library()
    assert lib.tsdf_mesh_slab_component_seam(one._c, None, None, None) == -4 and lib.tsdf_mesh_slab_download_components(one._c, None, None, None) == -4
    assert code(rr, one.mesh_slab_components) == -4
    one.close()


def test_two_runs_give_identical_bytes(rr, scene2):
    kind, res, level, slabs = R.CASES[3]                                  # speckle in four slabs: a thousand components, hooks racing in every launch
    vol = R.case_volume(kind, res, slabs, LIMIT)
    ctxs = slab_contexts(rr, scene2, vol, res, slabs)
    runs = []
    for _ in range(2):
        mgpu().mesh_slabs_on_one_device(ctxs, normals=False, colours=False, level=level)
        runs.append(mgpu().mesh_components_on_one_device(ctxs))
    assert_same(runs[0], runs[1])
    for a, b in zip(runs[0]["lists"], runs[1]["lists"]):
        assert all(a[k].tobytes() == b[k].tobytes() for k in ("down", "up", "roots"))
    for a, b in zip(runs[0]["merged"]["links"], runs[1]["merged"]["links"]):
        assert a.tobytes() == b.tobytes()
    for c in ctxs:
        c.close()
