"""GPU: mesh extraction on Z-slab contexts (tsdf_mesh_slab_extract / _seam / _link / _download) -- the parts of contiguous slabs, concatenated in slab
order, against the whole-volume context's extract and tests/mesh_slab_reference.py, byte for byte: crafted volumes with NaN, infinities, 0 and -0 in
every seam's planes; the integrated scene with exchanged and recomputed halos and in a sparse pool, normals and colours included; levels 1 and 2; the
one-slab case; errors and state; two runs."""
from importlib import import_module

import numpy as np
import pytest

import mesh_slab_reference as S

pytestmark = pytest.mark.gpu

LIMIT = 0.05                                                             # the halo is one tile layer at every resolution used here
KW = dict(brick_size=[2.0 / 8, 2.2 / 8, 2.0 / 8], limit=LIMIT, view=(64, 36))
SEED = 20261019                                                          # tests/test_mesh_slab_reference.py checks on the CPU that every seam of every case is crossed


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


def assert_same_arrays(got, want, keys):
    for k in keys:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert got[k].tobytes() == want[k].tobytes(), k


@pytest.fixture(scope="module")
def scene2(rr):
    return rr.scene.make_scene(n_streams=2, width=160, height=120, lut_res=32, inv_res=32)


def crafted(rr, scene, res, level, slabs):
    """the crafted volume on a whole-volume context and on one context per slab -> (whole mesh, reference, reference parts, joined slab parts)"""
    vol = S.crafted_volume(res, slabs, SEED, LIMIT)
    ref, parts = S.split(vol, LIMIT, scene["bbox_min"], scene["bbox_max"], level, slabs)
    whole = rr.ReconIntegrationHip(scene, res=res, **KW)
    whole.set_tsdf(vol)
    want = whole.extract_mesh(normals=True, colours=False, level=level)
    whole.close()
    ctxs = [rr.ReconIntegrationHip(scene, res=res, slab=s, **KW) for s in slabs]
    for c in ctxs:
        c.set_tsdf(vol)                                                  # fills the slab's stored layers, halo included
    got = mgpu().mesh_slabs_on_one_device(ctxs, normals=True, colours=False, level=level)
    stats = [c.mesh_slab_stats() for c in ctxs]
    for c in ctxs:
        c.close()
    return want, ref, parts, got, stats


CRAFTED = [((32, 32, 32), 0, [(0, 16), (16, 32)]),
           ((32, 32, 32), 0, [(0, 8), (8, 16), (16, 24), (24, 32)]),      # the thinnest legal slab: one tile layer, as thick as its halo
           ((20, 12, 28), 0, [(0, 8), (8, 24), (24, 28)]),                 # partial tiles on every axis, a top slab that is not a whole layer
           ((24, 20, 64), 1, [(0, 32), (32, 64)]),
           ((24, 20, 64), 2, [(0, 32), (32, 64)]),
           ((24, 20, 64), 1, [(0, 16), (16, 64)])]


@pytest.mark.parametrize("res,level,slabs", CRAFTED)
def test_crafted_volume_parts_join_byte_for_byte(rr, scene2, res, level, slabs):
    want, ref, parts, got, stats = crafted(rr, scene2, res, level, slabs)
    print(res, "level", level, slabs, "whole:", len(want["position"]), "vertices", len(want["triangles"]), "triangles; parts:", got["counts"])
    assert len(want["position"]) > 100 and len(want["triangles"]) > 100
    assert_same_arrays(want, ref, ("position", "triangles"))             # the whole-volume context and the numpy reference
    assert_same_arrays(got, want, ("position", "triangles", "normal"))   # the joined parts and the whole-volume context
    for k, p in enumerate(parts):
        assert got["counts"][k] == (p["vertices"][1] - p["vertices"][0], p["triangles"][1] - p["triangles"][0]), k
        assert got["seams"][k].dtype == np.uint32 and got["seams"][k].tobytes() == p["seam"].tobytes(), k
        ntx, nty, _ = ref["lattice_tiles"]
        assert stats[k]["tiles"] == (p["layers"][1] - p["layers"][0]) * ntx * nty
        assert stats[k]["bytes"] == got["counts"][k][0] * 24 + got["counts"][k][1] * 12
    for p in parts[:-1]:                                                  # not vacuous: every seam has triangles that index the slab above
        t0, t1 = p["triangles"]
        assert (got["triangles"][t0:t1] >= p["vertices"][1]).any() and S.crosses_seam(ref, p) > 0


def test_misaligned_slab_is_refused_at_a_level(rr, scene2):
    res = (24, 20, 64)
    c = rr.ReconIntegrationHip(scene2, res=res, slab=(0, 24), **KW)
    c.set_tsdf(S.crafted_volume(res, [(0, 24)], SEED, LIMIT))
    assert code(rr, lambda: c.extract_mesh_slab(False, False, level=1)) == -1
    assert code(rr, lambda: c.extract_mesh_slab(False, False, level=2)) == -1
    assert code(rr, lambda: c.extract_mesh_slab(False, False, level=3)) == -1
    assert c.extract_mesh_slab(False, False, level=0)[0] > 0              # level 0 always qualifies
    c.close()


def test_a_refused_extract_leaves_no_part(rr, scene2):
    """extract succeeds, the next extract is refused: the old part is gone -- in the library and in the binding -- so nothing can be copied into
    buffers sized for another extract (the level-1 table of this grid has 2 x 2 entries, the level-0 one 3 x 3)"""
    import ctypes as C
    res = (24, 20, 64)
    c = rr.ReconIntegrationHip(scene2, res=res, slab=(0, 24), **KW)
    c.set_tsdf(S.crafted_volume(res, [(0, 24)], SEED, LIMIT))
    lib = rr.load_library()
    refusals = (lambda: code(rr, lambda: c.extract_mesh_slab(False, False, level=1)),                          # the alignment rule
                lambda: code(rr, lambda: c.extract_mesh_slab(False, False, level=3)),
                lambda: lib.tsdf_mesh_slab_extract(c._c, C.c_uint32(4), C.c_uint32(0), None, None))           # an unknown flag, past the binding
    for refuse in refusals:
        nv, nt = c.extract_mesh_slab(False, False, level=0)
        assert nv > 0 and nt > 0 and c.mesh_slab_seam().shape == (3, 3) and c.mesh_slab_stats()["tiles"] == 27
        assert refuse() == -1
        # the library holds no part: every entry answers TSDF_ERR_STATE and writes nothing
        seam = np.full(9, 0xdeadbeef, np.uint32)
        assert lib.tsdf_mesh_slab_seam(c._c, seam.ctypes.data_as(C.POINTER(C.c_uint32))) == -4 and (seam == 0xdeadbeef).all()
        pos, tri = np.full((nv, 3), 7.0, np.float32), np.full((nt, 3), 7, np.uint32)
        assert lib.tsdf_mesh_slab_download(c._c, pos.ctypes.data_as(C.POINTER(C.c_float)), None, None, tri.ctypes.data_as(C.POINTER(C.c_uint32))) == -4
        assert (pos == 7.0).all() and (tri == 7).all()
        assert lib.tsdf_mesh_slab_link(c._c, C.c_uint64(0), seam.ctypes.data_as(C.POINTER(C.c_uint32))) == -4
        # ... and so does the binding (after its own refused extract before it makes a buffer)
        assert code(rr, c.mesh_slab_stats) == -4 and code(rr, c.mesh_slab_seam) == -4
        assert code(rr, lambda: c.mesh_slab_download(False, False, triangles=False)) == -4
    assert c.extract_mesh_slab(False, False, level=0) == (nv, nt)                         # and the context extracts again
    c.close()


# ---- the integrated scene
@pytest.fixture(scope="module")
def scene_whole(rr, small_scene):
    hip = rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), **KW)
    integrate(hip)
    mesh = hip.extract_mesh(normals=True, colours=True)
    hip.close()
    assert len(mesh["position"]) > 200 and len(mesh["triangles"]) > 200
    return mesh


@pytest.mark.parametrize("halo,sparse", [("exchange", 0), ("recompute", 0), ("recompute", 512)])
def test_small_scene_two_slabs_equal_the_whole_volume(rr, small_scene, scene_whole, halo, sparse):
    m = mgpu()
    mv, pr = rr.scene.default_view(*KW["view"])
    slabs = [rr.ReconIntegrationHip(small_scene, res=(32, 32, 32), slab=s, recompute_halo=(halo == "recompute"), sparse_pool_tiles=sparse, **KW)
             for s in ((0, 16), (16, 32))]
    m.frame_slabs_on_one_device(slabs, mv, pr, "cuda:0", halo=halo, composite="compact" if sparse else "dense")   # integrates; the halos are current
    got = m.mesh_slabs_on_one_device(slabs, normals=True, colours=True)
    print("small scene,", halo, "sparse" if sparse else "dense", "parts:", got["counts"], [s.mesh_slab_stats() for s in slabs])
    v1 = got["counts"][0][0]
    assert v1 > 0 and got["counts"][1][0] > 0
    assert (got["triangles"][:got["counts"][0][1]] >= v1).any()            # the seam is crossed
    assert_same_arrays(got, scene_whole, ("position", "normal", "colour", "triangles"))
    for s in slabs:
        s.close()


# ---- the one-slab case
@pytest.mark.parametrize("level", [0, 1, 2])
def test_whole_volume_context_is_the_one_slab_case(rr, scene2, level):
    res = (37, 43, 35)
    vol = S.crafted_volume(res, [(0, 35)], SEED, LIMIT)
    hip = rr.ReconIntegrationHip(scene2, res=res, **KW)
    hip.set_tsdf(vol)
    want = hip.extract_mesh(normals=True, colours=True, level=level)
    got = mgpu().mesh_slabs_on_one_device([hip], normals=True, colours=True, level=level)
    assert len(want["position"]) > 100
    assert_same_arrays(got, want, ("position", "normal", "colour", "triangles"))
    assert hip.mesh_slab_stats()["tiles"] == hip.mesh_stats()["tiles"] and hip.mesh_slab_stats()["tiles_with_surface"] == hip.mesh_stats()["tiles_with_surface"]
    assert_same_arrays(hip.download_mesh(normals=True, colours=True), want, ("position", "normal", "colour", "triangles"))   # the extract's own state is untouched
    hip.close()


# ---- errors, state, determinism
def test_errors_and_state(rr, scene2):
    res = (32, 32, 32)
    slabs = [(0, 16), (16, 32)]
    vol = S.crafted_volume(res, slabs, SEED, LIMIT)
    low, top = [rr.ReconIntegrationHip(scene2, res=res, slab=s, **KW) for s in slabs]
    assert code(rr, lambda: low.extract_mesh_slab(False, False)) == -4                  # no volume yet
    for c in (low, top):
        c.set_tsdf(vol)
    # before an extract
    assert code(rr, lambda: low.mesh_slab_link(0, np.zeros((4, 4), np.uint32))) == -4
    assert code(rr, low.mesh_slab_seam) == -4
    assert code(rr, lambda: low.mesh_slab_download(False, False)) == -4
    assert code(rr, low.mesh_slab_stats) == -4
    nv, nt = low.extract_mesh_slab(normals=False, colours=False)
    top.extract_mesh_slab(normals=False, colours=False)
    seam = top.mesh_slab_seam()
    assert nv > 0 and nt > 0 and seam.shape == (4, 4)
    # triangles before a link; attributes the extract did not produce
    assert code(rr, lambda: low.mesh_slab_download(False, False, triangles=True)) == -4
    assert len(low.mesh_slab_download(False, False, triangles=False)["position"]) == nv
    assert code(rr, lambda: low.mesh_slab_download(True, False, triangles=False)) == -4
    assert code(rr, lambda: low.mesh_slab_download(False, True, triangles=False)) == -4
    # the table of the slab above is needed below the top, and only there
    assert code(rr, lambda: low.mesh_slab_link(0, None)) == -1
    top.mesh_slab_link(nv, None)
    # index overflow
    assert code(rr, lambda: low.mesh_slab_link(2 ** 32 - 1, seam)) == -5
    assert code(rr, lambda: low.mesh_slab_link(2 ** 32 - nv - 1, seam)) == -5          # own indices fit, those into the slab above do not
    assert code(rr, lambda: low.mesh_slab_download(False, False)) == -4                 # a refused link wrote nothing
    # linking again with another base shifts every index by the difference
    low.mesh_slab_link(0, seam)
    a = low.mesh_slab_download(False, False)["triangles"].astype(np.int64)
    low.mesh_slab_link(1000, seam)
    b = low.mesh_slab_download(False, False)["triangles"].astype(np.int64)
    assert a.shape == (nt, 3) and ((b - a) == 1000).all() and (a >= nv).any()
    # the mesh entries of the whole-volume state keep refusing on the slab
    assert code(rr, low.mesh_components) == -4
    assert code(rr, lambda: low.extract_mesh(normals=False, colours=False)) == -4
    assert code(rr, low.mesh_stats) == -4
    # unknown flag, NULL context
    import ctypes as C
    lib = rr.load_library()
    n = C.c_uint64()
    assert lib.tsdf_mesh_slab_extract(low._c, C.c_uint32(4), C.c_uint32(0), C.byref(n), C.byref(n)) == -1
    assert lib.tsdf_mesh_slab_extract(None, C.c_uint32(0), C.c_uint32(0), None, None) == -1
    assert lib.tsdf_mesh_slab_seam(low._c, None) == -1 and lib.tsdf_mesh_slab_stats(low._c, None) == -1
    low.close()
    top.close()
    # a new grid: the part went with the old one (a slab context keeps its grid: the one-slab case shows it)
    one = rr.ReconIntegrationHip(scene2, res=res, **KW)
    one.set_tsdf(vol)
    assert one.extract_mesh_slab(False, False)[0] > 0 and one.mesh_slab_seam().shape == (4, 4)
    one.setVoxelSize(0.1)
    assert code(rr, one.mesh_slab_seam) == -4 and code(rr, one.mesh_slab_stats) == -4
    one.close()


def test_two_runs_give_identical_bytes(rr, scene2):
    res = (20, 12, 28)
    slabs = [(0, 8), (8, 24), (24, 28)]
    vol = S.crafted_volume(res, slabs, SEED, LIMIT)
    ctxs = [rr.ReconIntegrationHip(scene2, res=res, slab=s, **KW) for s in slabs]
    for c in ctxs:
        c.set_tsdf(vol)
    runs = [mgpu().mesh_slabs_on_one_device(ctxs, normals=True, colours=True, level=0) for _ in range(2)]
    assert_same_arrays(runs[0], runs[1], ("position", "normal", "colour", "triangles"))
    assert runs[0]["counts"] == runs[1]["counts"]
    for c in ctxs:
        c.close()
