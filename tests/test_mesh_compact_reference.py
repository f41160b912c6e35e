"""CPU: the tile-local triangle format (tests/mesh_compact_reference.py) on the references' own meshes.  On every volume and level: the round trip is
byte-equal, the rows are the tiles with surface, every tile with triangles has a row, offsets stay under 3584, neighbour code 7 never occurs, bit 15 is
clear; the filtered form decodes to mesh_stream_filter_reference's triangles; the empty mesh gives empty arrays."""
import numpy as np
import pytest

import mesh_compact_reference as MC
import mesh_component_reference as K
import mesh_lod_reference as LOD
import mesh_reference as M
import mesh_stream_filter_reference as SF

BMIN, BMAX = (-1.0, 0.0, -1.0), (1.0, 2.2, 1.0)
_BIG = LOD.random_volume((40, 44, 38))
VOLUMES = {
    "random": (K.random_volume(), K.LIMIT, (0, 1)),
    "speckle": (K.speckle_volume(), K.LIMIT, (0, 1)),
    "snakes": (K.snakes_volume(), K.LIMIT, (0, 1)),
    "shells": (K.shells_volume(), K.LIMIT, (0, 1)),
    "sphere": (M.sphere_volume(), 0.05, (0, 1)),
    "random40": (_BIG, 0.04, (0, 1, 2)),
    "checkerboard": (MC.checkerboard(), 0.04, (0,)),
}
CASES = [(name, level) for name, (_, _, levels) in VOLUMES.items() for level in levels]
_meshes = {}


def mesh_of(name, level):
    if (name, level) not in _meshes:
        vol, limit, _ = VOLUMES[name]
        _meshes[(name, level)] = LOD.extract_lod(vol, limit, BMIN, BMAX, level)
    return _meshes[(name, level)]


@pytest.mark.parametrize("name,level", CASES)
def test_round_trip_and_the_formats_bounds(name, level):
    vol = VOLUMES[name][0]
    m = mesh_of(name, level)
    table, codes, tiles = MC.encode(m, level, vol.shape)
    assert tiles == tuple(-(-LOD.lattice_shape(vol.shape, level)[2 - a] // 8) for a in range(3))
    tri = np.asarray(m["triangles"], np.uint32).reshape(-1, 3)
    assert len(tri) > 0 and codes.dtype == np.uint16 and codes.shape == tri.shape and table.dtype.itemsize == 16
    assert MC.decode(table, codes, tiles).tobytes() == tri.tobytes()
    assert len(table) == m["tiles_with_surface"]                          # rows == tiles with surface
    assert (np.diff(table["tile"].astype(np.int64)) > 0).all() and table["tile"].max() < tiles[0] * tiles[1] * tiles[2]
    ends = np.append(table["first_vertex"][1:], len(m["unit"]))
    assert table["first_vertex"][0] == 0 and (ends > table["first_vertex"]).all()      # every row owns a vertex: a tile with triangles has one
    assert table["first_triangle"][0] == 0 and (table["first_triangle"].astype(np.int64) + table["n_triangles"]
                                                == np.append(table["first_triangle"][1:], len(tri))).all()
    assert int((codes & 0xfff).max()) < 3584 and int((ends - table["first_vertex"]).max()) <= 3584
    assert not (codes >> 15).any() and not ((codes >> 12) == 7).any()


def test_every_neighbour_code_occurs_on_the_random_volume():
    _, codes, _ = MC.encode(mesh_of("random", 0), 0, VOLUMES["random"][0].shape)
    assert sorted(np.unique(codes >> 12)) == list(range(7))
    assert MC.tile_grid(VOLUMES["random"][0].shape, 0) == (3, 3, 3)


def test_checkerboard_is_the_densest_case():
    m = mesh_of("checkerboard", 0)
    table, _, _ = MC.encode(m, 0, (16, 16, 16))
    per_tile = np.append(table["first_vertex"][1:], len(m["unit"])) - table["first_vertex"]
    # the first tile: the three axis edges and the space diagonal of each of its 512 points are crossed, and each of its 512 cells has 12 triangles,
    # the most a cell can have (6144 is what the count kernel's 16-bit field is sized for)
    assert len(table) == 8 and per_tile[0] == 512 * 4 and table["n_triangles"][0] == 512 * 12


@pytest.mark.parametrize("min_triangles", [1, 100])
def test_filtered_form_decodes_to_the_filter_references_triangles(min_triangles):
    vol = VOLUMES["speckle"][0]
    m = mesh_of("speckle", 0)
    table, codes, tiles, mask = MC.encode_filtered(m, 0, vol.shape, min_triangles)
    _, want, words = SF.filtered_frame(vol, K.LIMIT, BMIN, BMAX, min_triangles)
    assert MC.decode(table, codes, tiles).tobytes() == np.asarray(want, np.uint32).tobytes()
    assert int(mask.sum()) == len(m["unit"]) - words[2] and len(codes) == len(m["triangles"]) - words[3]
    ends = np.append(table["first_vertex"][1:], int(mask.sum()))
    assert (ends > table["first_vertex"]).all()                           # no row without a kept vertex
    if min_triangles == 1:
        assert mask.all() and table.tobytes() == MC.encode(m, 0, vol.shape)[0].tobytes()
    else:
        assert (words[1], int(mask.sum()), len(codes)) == (61, 7958, 15180)   # DESIGN.md's speckle figures


def test_empty_mesh_gives_empty_arrays():
    vol = np.full((19, 22, 20), -K.LIMIT, np.float32)
    m = LOD.extract_lod(vol, K.LIMIT, BMIN, BMAX, 0)
    table, codes, tiles = MC.encode(m, 0, vol.shape)
    assert len(table) == 0 and codes.shape == (0, 3) and tiles == (3, 3, 3)
    assert MC.decode(table, codes, tiles).shape == (0, 3) and MC.payload_bytes(0, 8, 0, 0) == 0
    assert MC.payload_bytes(3, 8, 1, 1) == 32 + 16 + 6 and MC.payload_bytes(3, 16, 1, 1) == 48 + 16 + 6
