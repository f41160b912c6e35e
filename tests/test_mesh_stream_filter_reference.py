"""CPU: known answers of tests/mesh_stream_filter_reference.py on the components' test volumes (the counts do not depend on the bounding box), and that
packing commutes with keeping: pack(keep(mesh)) == pack(mesh)[kept]."""
import numpy as np
import pytest

import mesh_component_reference as K
import mesh_lod_reference as LOD
import mesh_pack_reference as P
import mesh_reference as M
import mesh_stream_filter_reference as F

BMIN, BMAX = (-1.0, 0.0, -1.0), (1.0, 2.2, 1.0)

# (volume, level, min_triangles) -> (vertices, triangles, components of the unfiltered mesh, components kept)
CASES = [
    ("speckle", 0, 1, (13532, 24420, 343, 343)),
    ("speckle", 0, 100, (7958, 15180, 343, 61)),
    ("speckle", 0, 2000, (0, 0, 343, 0)),
    ("random", 0, 100, (26222, 52574, 8, 2)),
    ("shells", 0, 1, (11246, 22480, 3, 3)),
    ("shells", 0, 2000, (10584, 21160, 3, 2)),
    ("snakes", 0, 12796, (12800, 25592, 2, 2)),
    ("snakes", 0, 12797, (0, 0, 2, 0)),
    ("speckle_odd", 1, 1, (13616, 24550, 333, 333)),
    ("speckle_odd", 1, 100, (8046, 15458, 333, 51)),
]
VOLUMES = dict(speckle=K.speckle_volume, random=K.random_volume, shells=K.shells_volume, snakes=K.snakes_volume,
               speckle_odd=lambda: K.speckle_volume(res=(39, 43, 37)))      # odd: the level-1 lattice ends before the volume does


@pytest.fixture(scope="module")
def volumes():
    return {name: make() for name, make in VOLUMES.items()}


@pytest.mark.parametrize("name,level,min_triangles,want", CASES)
def test_known_answers(volumes, name, level, min_triangles, want):
    v, t, words = F.filtered_frame(volumes[name], K.LIMIT, BMIN, BMAX, min_triangles, level=level)
    print(name, level, min_triangles, len(v), len(t), words)
    assert v.dtype == np.uint16 and v.shape == (want[0], 4) and t.dtype == np.uint32 and t.shape == (want[1], 3)
    assert words[:2] == want[2:]
    whole = F.filtered_frame(volumes[name], K.LIMIT, BMIN, BMAX, 1, level=level)
    assert words[2:] == (len(whole[0]) - want[0], len(whole[1]) - want[1])
    if len(t):
        assert int(t.max()) == len(v) - 1                                   # remapped: dense again


def test_shells_components(volumes):
    m = M.extract(volumes["shells"], K.LIMIT, BMIN, BMAX)
    table = K.components(m["triangles"], len(m["unit"]))[2]
    assert table["n_triangles"].tolist() == [15192, 5968, 1320]


def test_min_1_is_the_unfiltered_frame(volumes):
    v, t, words = F.filtered_frame(volumes["random"], K.LIMIT, BMIN, BMAX, 1)
    want_v, want_t, _ = P.pack_volume(volumes["random"], K.LIMIT, BMIN, BMAX)
    assert v.tobytes() == want_v.tobytes() and t.tobytes() == want_t.tobytes() and words == (8, 8, 0, 0)


@pytest.mark.parametrize("name,level,min_triangles", [("speckle", 0, 100), ("shells", 0, 2000), ("speckle_odd", 1, 100)])
def test_pack_commutes_with_keep(volumes, name, level, min_triangles):
    vol = volumes[name]
    m = M.extract(vol, K.LIMIT, BMIN, BMAX) if level == 0 else LOD.extract_lod(vol, K.LIMIT, BMIN, BMAX, level)
    rng = np.random.default_rng(5)
    nv = len(m["unit"])
    normal = rng.normal(size=(nv, 3)).astype(np.float32)
    normal[rng.random(nv) < 0.02] = np.nan
    colour = rng.uniform(-0.2, 1.2, (nv, 4)).astype(np.float32)
    mesh = dict(unit=m["unit"], triangles=m["triangles"], normal=normal, colour=colour)
    kept, mask, words = F.filter_mesh(mesh, min_triangles)
    assert 0 < mask.sum() < nv and words[2] == nv - mask.sum()
    assert P.pack(kept["unit"]).tobytes() == P.pack(m["unit"])[mask].tobytes()
    assert P.pack(kept["unit"], kept["normal"], kept["colour"]).tobytes() == P.pack(m["unit"], normal, colour)[mask].tobytes()
    v, t, w = F.filtered_frame(vol, K.LIMIT, BMIN, BMAX, min_triangles, level=level, normal=normal, colour=colour)
    assert v.tobytes() == P.pack(m["unit"], normal, colour)[mask].tobytes() and t.tobytes() == kept["triangles"].tobytes() and w == words
