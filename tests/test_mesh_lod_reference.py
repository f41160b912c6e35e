"""CPU: tests/mesh_lod_reference.py, the numpy restatement of the mesh level of detail, against what the definition promises: level 0 is the mesh
extraction itself; every coarse vertex is a level-0 vertex, bit for bit; a closed surface inside the lattice stays a closed 2-manifold at every level;
a lattice thinner than 2 is empty; and the descent of a hand-worked edge lands where it must."""
import numpy as np
import pytest

import mesh_lod_reference as L
import mesh_reference as M

LIMIT = 0.04
BOX = ([-1.0, 0.0, -1.0], [1.0, 2.2, 1.0])
RANDOM_RES = (37, 43, 35)


@pytest.fixture(scope="module")
def random_levels():
    vol = L.random_volume(RANDOM_RES, limit=LIMIT)
    assert (vol == 0).mean() > 0.08 and np.isnan(vol).sum() > 5 and np.isinf(vol).sum() > 5 and (np.signbit(vol) & (vol == 0)).sum() > 5
    return vol, [L.extract_lod(vol, LIMIT, *BOX, level) for level in range(3)]


def test_level_0_is_the_extraction_bit_for_bit(random_levels):
    vol, levels = random_levels
    want = M.extract(vol, LIMIT, *BOX)
    for k in ("position", "unit", "triangles"):
        assert levels[0][k].dtype == want[k].dtype and levels[0][k].tobytes() == want[k].tobytes(), k
    assert levels[0]["tiles"] == 5 * 6 * 5


def test_lattice_shapes_and_tiles():
    shape = RANDOM_RES[::-1]
    assert L.lattice_shape(shape, 1)[::-1] == (19, 22, 18) and L.lattice_tiles(shape, 1) == 27          # padded on every axis
    assert L.lattice_shape(shape, 2)[::-1] == (10, 11, 9) and L.lattice_tiles(shape, 2) == 8


def test_coarse_vertices_are_level_0_vertices(random_levels):
    _, levels = random_levels
    for level in range(3):
        r = levels[level]
        print("level", level, len(r["position"]), "vertices", len(r["triangles"]), "triangles", r["tiles"], "tiles", r["tiles_with_surface"], "with surface")
        assert len(r["position"]) > 1000 and len(r["triangles"]) > 1000 and np.isfinite(r["position"]).all()
        assert int(r["triangles"].max()) < len(r["position"])
    row = lambda u: np.ascontiguousarray(u, np.float32).view(np.dtype((np.void, 12))).ravel()
    fine = row(levels[0]["unit"])
    for level in (1, 2):
        assert np.isin(row(levels[level]["unit"]), fine).all(), level   # bitwise members of the level-0 position set
        assert levels[level]["tiles"] == (27, 8)[level - 1] and levels[level]["tiles_with_surface"] == levels[level]["tiles"]
    assert len(levels[0]["position"]) > len(levels[1]["position"]) > len(levels[2]["position"])


@pytest.mark.parametrize("level", [0, 1, 2])
def test_sphere_inside_the_lattice_is_a_closed_2_manifold(level):
    """48 x 40 x 40: the surface stays inside the level-2 lattice.  (At 24 x 16 x 16 the level-2 lattice ends inside the sphere and the mesh is open:
    a property of the definition -- the mesh ends at the last lattice point --, not a defect.)"""
    vol = M.sphere_volume((48, 40, 40), limit=LIMIT)
    r = L.extract_lod(vol, LIMIT, *BOX, level)
    rep = M.manifold_report(r["triangles"], len(r["position"]))
    print("sphere level", level, rep)
    assert rep["faces"] > 500 and rep["vertices_used"] == len(r["position"])
    assert rep["directed_unique"] and rep["edges_shared_by_two"] and rep["opposite"]
    assert rep["euler"] == 2
    assert M.signed_volume(r["position"], r["triangles"]) > 0


def test_the_small_sphere_is_open_at_level_2():
    """the fixture above matters: this one's level-2 lattice (6 x 4 x 4, last point at voxel 12 of 16 in y and z) ends inside the sphere"""
    r = L.extract_lod(M.sphere_volume((24, 16, 16), limit=LIMIT), LIMIT, *BOX, 2)
    assert len(r["triangles"]) > 0 and not M.manifold_report(r["triangles"], len(r["position"]))["edges_shared_by_two"]


def test_a_thin_lattice_is_empty():
    vol = np.random.default_rng(5).uniform(-LIMIT, LIMIT, (20, 20, 4)).astype(np.float32)   # rx = 4: one lattice point at level 2
    r = L.extract_lod(vol, LIMIT, *BOX, 2)
    assert len(r["position"]) == 0 and len(r["triangles"]) == 0 and r["tiles_with_surface"] == 0
    assert len(L.extract_lod(vol, LIMIT, *BOX, 1)["position"]) > 0                           # two points at level 1: cells exist


@pytest.mark.parametrize("crossing", range(8))
def test_hand_worked_edge(crossing):
    """9 voxels along x, inside up to voxel `crossing`, outside after it (one sign change), 5 x 5 in y and z so that the level-2 lattice has cells.  The
    x edge of the row y = z = 0 must land on the voxel pair (crossing, crossing + 1) at every level, with the level-0 vertex of that pair."""
    row = np.where(np.arange(9) <= crossing, 0.03, -0.02).astype(np.float32)
    row[crossing] = 0.01                                                  # the pair's values are its own: t = 0.01 / 0.03
    vol = np.broadcast_to(row, (5, 5, 9)).copy()
    fine = L.extract_lod(vol, LIMIT, *BOX, 0)
    want = fine["unit"][(fine["d"] == 1) & (fine["voxel"][:, 1] == 0) & (fine["voxel"][:, 2] == 0)]
    assert len(want) == 1
    for level in (1, 2):
        s = 1 << level
        r = L.extract_lod(vol, LIMIT, *BOX, level)
        pick = (r["d"] == 1) & (r["voxel"][:, 1] == 0) & (r["voxel"][:, 2] == 0)
        assert pick.sum() == 1                                            # the lattice edge [s * (crossing // s), + s] is the only crossed x edge of the row
        assert tuple(r["voxel"][pick][0]) == (crossing, 0, 0)
        assert r["unit"][pick].tobytes() == want.tobytes()
        a, b = np.float32(0.01), np.float32(-0.02)
        t = a / (a - b)
        ux = (np.float32(crossing) + np.float32(0.5)) / np.float32(9)
        ux1 = (np.float32(crossing + 1) + np.float32(0.5)) / np.float32(9)
        assert r["unit"][pick][0, 0] == ux + t * (ux1 - ux)
        assert crossing // s * s <= crossing < crossing // s * s + s
