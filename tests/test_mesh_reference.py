"""CPU: tests/mesh_reference.py, the numpy restatement of the mesh extraction's definition, against the properties the definition promises: the
winding of every (tetrahedron, case) pair, a closed 2-manifold for a closed surface, and the special values."""
import os
import re

import numpy as np
import pytest

import mesh_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = ([-1.0, 0.0, -1.0], [1.0, 2.2, 1.0])


@pytest.mark.parametrize("tet", range(6))
def test_winding_of_every_case(tet):
    """corner values +-1: the geometric normal of every triangle points from the inside centroid to the outside centroid"""
    corners = np.array([M.corner_xyz(b) for b in range(8)])
    for case in range(1, 15):
        v = M.TETS[tet]
        ins = [v[j] for j in range(4) if (case >> j) & 1]
        out = [x for x in v if x not in ins]
        # a 2 x 2 x 2 volume whose only tetrahedron with a sign change among ITS corners is looked at through case_triangles
        tris = M.case_triangles(tet, case)
        assert len(tris) == (2 if len(ins) == 2 else 1)
        towards = corners[out].mean(0) - corners[ins].mean(0)
        for tri in tris:
            p = [(corners[x] + corners[y]) * 0.5 for x, y in tri]
            assert np.dot(np.cross(p[1] - p[0], p[2] - p[0]), towards) > 0, (tet, case, tri)
            assert all(x < y and (x & y) == x for x, y in tri)            # every edge runs from a corner to one that contains it


def test_winding_is_a_property_of_parity_and_case():
    assert [M.tetrahedron_parity(k) for k in range(6)] == [1, -1, -1, 1, 1, -1]
    t = M.winding_table()
    assert t[0] == t[3] == t[4] and t[1] == t[2] == t[5] and t[0] ^ t[1] == 0x7ffe       # mirrored tetrahedra: every case reversed


def test_kernel_table_is_the_generated_one():
    src = open(os.path.join(ROOT, "rgbd-recon_amd", "csrc", "k_mesh.hip")).read()
    m = re.search(r"c_mesh_flip\[6\]\s*=\s*\{([^}]*)\}", src)
    assert m and [int(w, 16) for w in m.group(1).split(",")] == M.winding_table()
    m = re.search(r"c_tet\[6\]\[4\]\s*=\s*\{(.*?)\};", src)
    assert m and tuple(tuple(int(x) for x in g.split(",")) for g in re.findall(r"\{([\d, ]+)\}", m.group(1))) == M.TETS


def test_a_single_cell_through_the_whole_extract():
    """one inside corner of a 2^3 volume: the triangles of extract() carry the winding of the table, end to end"""
    for b in range(8):
        vol = np.full((2, 2, 2), -1.0, np.float32)
        vol[b >> 2, (b >> 1) & 1, b & 1] = 1.0
        r = M.extract(vol, 1.0, [0, 0, 0], [2, 2, 2])                     # lattice point (i, j, k) at world (i + .5, j + .5, k + .5)
        p, t = r["position"].astype(np.float64), r["triangles"].astype(np.int64)
        assert len(t) > 0 and len(p) == (7 if b in (0, 7) else len(p))
        inside = M.corner_xyz(b) + 0.5
        for tri in t:
            n = np.cross(p[tri[1]] - p[tri[0]], p[tri[2]] - p[tri[0]])
            assert np.dot(n, p[tri].mean(0) - inside) > 0                 # away from the only inside corner


@pytest.fixture(scope="module")
def sphere():
    vol = M.sphere_volume((24, 16, 16))
    return vol, M.extract(vol, 0.05, *BOX)


def test_sphere_is_a_closed_2_manifold(sphere):
    _, r = sphere
    rep = M.manifold_report(r["triangles"], len(r["position"]))
    assert rep["faces"] > 1000 and rep["vertices_used"] == len(r["position"])           # every vertex is used, none twice
    assert rep["directed_unique"] and rep["edges_shared_by_two"] and rep["opposite"]
    assert rep["euler"] == 2
    assert M.signed_volume(r["position"], r["triangles"]) > 0
    assert len(np.unique(r["position"], axis=0)) == len(r["position"])                  # a vertex exists once


def test_order_is_tile_major(sphere):
    vol, r = sphere
    rz, ry, rx = vol.shape
    lo, hi = np.array(BOX[0], np.float32), np.array(BOX[1], np.float32)
    # the owner of a vertex is the lattice point just below it on every axis the edge moves along; recover its tile from the position
    u = (r["position"] - lo) / (hi - lo)
    owner = np.floor(u * np.array([rx, ry, rz]) - 0.5 + 1e-4).astype(int)
    tile = ((owner[:, 2] >> 3) * 2 + (owner[:, 1] >> 3)) * 3 + (owner[:, 0] >> 3)
    assert (np.diff(tile) >= 0).all() and len(np.unique(tile)) > 4
    tri_tile = tile[r["triangles"].astype(np.int64)].min(axis=1)                        # the cell's tile is the smallest tile among its vertices' owners
    assert (np.diff(tri_tile) >= 0).all()


def test_zero_negative_zero_nan_and_inf():
    base = np.full((3, 3, 3), -0.5, np.float32)
    base[1, 1, 1] = 0.5
    want = M.extract(base, 0.5, *BOX)
    assert len(want["position"]) == 14 and len(want["triangles"]) > 0                   # one inside point: the 7 edges it owns and the 7 that end in it
    for outside in (0.0, -0.0):
        v = np.full((3, 3, 3), outside, np.float32)
        v[1, 1, 1] = 0.5
        r = M.extract(v, 0.5, *BOX)
        assert (r["triangles"] == want["triangles"]).all()                # zero and -0 are outside: the same topology ...
        g = r["unit"].astype(np.float64) * 3 - 0.5                        # ... with t = 1 (or 0 where the outside end owns the edge): every vertex sits ON the
        assert np.allclose(g, np.round(g), atol=1e-5) and (np.abs(g - 1).max(axis=1) > 0.5).all()   # outside end of its edge, a lattice point other than the centre
    for bad in (np.nan, np.inf, -np.inf):
        v = base.copy()
        v[0, 1, 2] = bad
        v[2, 2, 2] = bad
        r = M.extract(v, 0.5, *BOX)
        assert (r["position"].view(np.uint32) == want["position"].view(np.uint32)).all() and (r["triangles"] == want["triangles"]).all()   # reads as -limit = -0.5
        assert np.isfinite(r["position"]).all()
    inside_inf = base.copy()
    inside_inf[1, 1, 1] = np.inf                                          # even where it would be inside: -limit, no surface left
    assert len(M.extract(inside_inf, 0.5, *BOX)["position"]) == 0
    only_zero = np.zeros((4, 4, 4), np.float32)
    assert len(M.extract(only_zero, 0.5, *BOX)["triangles"]) == 0
    assert len(M.extract(np.ones((1, 5, 5), np.float32), 0.5, *BOX)["position"]) == 0   # a lattice one point thick has no cell


def test_degenerate_triangles_are_kept():
    v = np.full((3, 3, 3), -0.5, np.float32)
    v[1, 1, 1] = 0.5
    v[1, 1, 2] = 0.0                                                      # t = 1 on one edge only; no triangle is dropped for it
    assert len(M.extract(v, 0.5, *BOX)["triangles"]) == len(M.extract(np.where(v == 0, np.float32(-0.5), v), 0.5, *BOX)["triangles"])


def test_canonical_rotation_keeps_the_winding():
    t = np.array([[5, 2, 9], [1, 7, 3], [8, 6, 0]])
    assert (M.canonical(t) == [[2, 9, 5], [1, 7, 3], [0, 8, 6]]).all()
