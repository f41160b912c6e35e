"""CPU: tests/ray_part_reference.py (the ray queries' slab parts in numpy) -- on the slab sets of tests/test_gpu_mesh_slab.py's level-0 crafted cases the
merged reference parts equal tests/ray_reference.py's whole-volume cast byte for byte, and the cases are not vacuous: every seam of every case has rays
that hit in another slab than they start in, hits whose predecessor sample is the neighbour's, downward rays that cross it, and rays that hit in two slabs."""
import numpy as np
import pytest

import mesh_slab_reference as S
import ray_part_reference as P
import ray_reference as Q

LIMIT = 0.05                                                             # the halo is one tile layer at every resolution used here
SEED = 20261020                                                          # chosen so that the counts below hold; checked here
BBOX = ((-1.0, 0.0, -1.0), (1.0, 2.2, 1.0))
CASES = [((32, 32, 32), [(0, 16), (16, 32)]),
         ((32, 32, 32), [(0, 8), (8, 16), (16, 24), (24, 32)]),          # the thinnest legal slab
         ((20, 12, 28), [(0, 8), (8, 24), (24, 28)])]
_cache = {}


def case(res, slabs):
    """(vol, rays, trace) of a case, computed once per session: tests/test_gpu_ray_parts.py shares it"""
    key = (res, tuple(slabs))
    if key not in _cache:
        vol = S.crafted_volume(res, slabs, SEED, LIMIT)
        rays = P.seam_rays(SEED, res, slabs, vol, LIMIT)
        _cache[key] = (vol, rays, P.trace(vol, LIMIT, BBOX[0], BBOX[1], rays, True))
    return _cache[key]


@pytest.mark.parametrize("res,slabs", CASES)
def test_merged_reference_parts_equal_the_whole_cast(res, slabs):
    vol, rays, T = case(res, slabs)
    want = Q.cast(vol, LIMIT, BBOX[0], BBOX[1], rays, unit_cube=True)
    whole = P.whole(T)
    assert Q.same_bytes(whole["hits"], want["hits"]).all() and (whole["unit"].view(np.uint32) == want["unit"].view(np.uint32)).all()   # the trace reads as the march
    parts = P.parts(T, slabs)
    merged, win = P.merge([p["hits"] for p in parts])
    assert Q.same_bytes(merged, want["hits"]).all()
    st = want["hits"]["status"]
    print(res, slabs, len(rays), "rays:", int((st & 1).sum()), "hits,", int((st == 2).sum()), "outside,", int((st == 4).sum()), "invalid; winners per part",
          np.bincount(win[(st & 1) != 0], minlength=len(slabs)))
    assert 1500 <= len(rays) <= 2600 and (st & 1).sum() > 500 and (st == 2).sum() > 20 and (st == 4).sum() == 12
    for p in parts:                                                      # OUTSIDE and INVALID are identical on every slab; a part's miss reports max_n
        assert (p["hits"]["status"][(st & 6) != 0] == st[(st & 6) != 0]).all()
        miss = (p["hits"]["status"] & 1) == 0
        assert (p["hits"]["n_samples"][miss] == T["S"]["max_n"][miss]).all() and (p["hits"]["t"][miss] == -1).all() and not p["hits"]["pos"][miss].any()


@pytest.mark.parametrize("res,slabs", CASES)
def test_the_halo_covers_the_surface_of_every_winner(res, slabs):
    """a part's normals are read from the slab's stored planes (z taps clamped into them); where the part wins they are the whole volume's"""
    vol, rays, T = case(res, slabs)
    parts = P.parts(T, slabs)
    merged, win = P.merge([p["hits"] for p in parts])
    want = Q.surface(vol, None, LIMIT, BBOX[0], BBOX[1], P.whole(T), normals=True, colours=False)
    surf = [P.part_surface(vol, None, LIMIT, BBOX[0], BBOX[1], p, slab, colours=False) for p, slab in zip(parts, slabs)]
    _, joined, _ = P.merge([p["hits"] for p in parts], surf)
    assert Q.same_bytes(joined, want).all() and (np.nan_to_num(want["normal"]) != 0).any(1).sum() > 500
    assert P.stored_planes(res[2], LIMIT, slabs[0]) == (0, slabs[0][1] + 7) and P.stored_planes(res[2], LIMIT, (0, res[2])) == (0, res[2] - 1)   # one halo layer


@pytest.mark.parametrize("res,slabs", CASES)
def test_every_seam_is_exercised(res, slabs):
    _, _, T = case(res, slabs)
    per, two = P.seam_counts(T, slabs)
    print(res, slabs, per, "rays that hit in two slabs:", two)
    assert len(per) == len(slabs) - 1
    for s, c in enumerate(per):
        assert c["elsewhere"] >= 10 and c["predecessor"] >= 10 and c["downward"] >= 10, (s, c)
    assert two >= 1


def test_merge_rule_known_answers():
    h = np.zeros((3, 4), Q.RAY_HIT_DTYPE)
    h["t"] = -1
    h["n_samples"] = 9                                                   # every part's miss: max_n
    h[0]["n_samples"][0], h[0]["status"][0] = 5, 1                       # ray 0: parts 0 and 2 hit, the smaller count wins
    h[2]["n_samples"][0], h[2]["status"][0] = 3, 1
    h[1]["n_samples"][1], h[1]["status"][1] = 9, 1                       # ray 1: a hit at the last sample beats the misses with the same count
    h["status"][:, 3] = 2                                                # ray 3: outside on every slab
    for k in range(3):
        h[k]["pos"] = k + 1
    merged, win = P.merge(list(h))
    assert list(win) == [2, 1, 0, 0]
    assert merged["n_samples"].tolist() == [3, 9, 9, 9] and merged["status"].tolist() == [1, 1, 0, 2] and merged["pos"][:, 0].tolist() == [3, 2, 1, 1]
    surf = np.zeros((3, 4), Q.RAY_SURFACE_DTYPE)
    for k in range(3):
        surf[k]["rgba"] = 10 + k
    _, s, _ = P.merge(list(h), list(surf))
    assert s["rgba"][:, 0].tolist() == [12, 11, 10, 10]


def test_owner_plane_formula():
    """plane = fminf(fmaxf(floorf(z * rz), 0), rz - 1): NaN gives plane 0, +-inf clamp, the seam plane itself belongs to the slab above"""
    z = np.array([[np.nan, -np.inf, np.inf, 0.5, np.nextafter(np.float32(0.5), np.float32(0)), -0.1, 1.0, 0.99]], np.float32)
    plane = P.owner_plane(z, 16)
    assert plane.tolist() == [[0, 0, 15, 8, 7, 0, 15, 15]]
    assert P.owner(dict(plane=plane), [(0, 8), (8, 16)]).tolist() == [[0, 0, 1, 1, 0, 0, 1, 1]]
