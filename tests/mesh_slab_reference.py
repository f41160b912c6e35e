"""numpy restatement of the mesh extraction on Z-slab contexts (include/rgbd_recon_hip.h, "mesh extraction on Z-slab contexts"), on top of
tests/mesh_reference.py and tests/mesh_lod_reference.py.

The whole reference mesh of a level is ordered by 8^3 lattice tile with the tile layer outermost, so a slab that owns lattice tile layers [L0, L1)
owns one contiguous range of its vertices and one of its triangles.  From a volume, a level and slab ranges (voxel planes [z0, z1)) this gives each
slab's two ranges, its seam table (the slab-local vertex base of every lattice tile of its first owned layer) and its part in the form a device keeps
it before the link: own indices slab-local, indices into the slab above as (tile of the layer above, offset behind that tile's base)."""
import numpy as np

import mesh_lod_reference as L
import mesh_reference as M

f32 = np.float32


def slab_layers(shape, level, z0, z1):
    """lattice tile layers [L0, L1) of voxel planes [z0, z1) of a [rz][ry][rx] volume; ValueError where the planes do not lie on the level's lattice tiles"""
    rz = shape[0]
    t = 8 << level
    ntz = (L.lattice_shape(shape, level)[0] + 7) // 8
    if z0 % t or (z1 % t and z1 != rz) or not 0 <= z0 < z1 <= rz:
        raise ValueError(f"planes [{z0}, {z1}) do not lie on level {level}'s lattice tiles")
    return z0 // t, (ntz if z1 == rz else z1 // t)


def _cell_triangle_counts(sub):
    """triangles of every cell of the lattice `sub` (sanitised), [cz - 1][cy - 1][cx - 1]"""
    inside = sub > 0
    cz, cy, cx = (n - 1 for n in sub.shape)
    corner = [inside[(b >> 2):(b >> 2) + cz, ((b >> 1) & 1):((b >> 1) & 1) + cy, (b & 1):(b & 1) + cx] for b in range(8)]
    per_case = np.array([[len(M.case_triangles(k, cs)) for cs in range(16)] for k in range(6)])
    n = np.zeros((cz, cy, cx), np.int64)
    for k in range(6):
        case = sum(corner[M.TETS[k][j]].astype(np.int64) << j for j in range(4))
        n += per_case[k][case]
    return n


def split(vol, limit, bbox_min, bbox_max, level, slabs):
    """-> (ref, parts): ref = mesh_lod_reference.extract_lod of the whole volume; parts[k] for slabs[k] = (z0, z1):
    dict(vertices=(v0, v1), triangles=(t0, t1), seam=[nty][ntx] uint32, layers=(L0, L1))."""
    ref = L.extract_lod(vol, limit, bbox_min, bbox_max, level)
    s = 1 << level
    f = M.sanitised(vol, limit)
    cz, cy, cx = L.lattice_shape(f.shape, level)
    ntx, nty, ntz = (cx + 7) // 8, (cy + 7) // 8, (cz + 7) // 8
    lat = ref["voxel"] // s                                              # the owning lattice point (the descent stays inside its lattice edge)
    tile = ((lat[:, 2] >> 3) * nty + (lat[:, 1] >> 3)) * ntx + (lat[:, 0] >> 3)
    assert (np.diff(tile) >= 0).all()                                    # vertices are ordered by tile, the layer outermost
    tile_vbase = np.concatenate([[0], np.cumsum(np.bincount(tile, minlength=ntx * nty * ntz))])
    tri_of_layer = np.zeros(ntz, np.int64)
    if min(cx, cy, cz) >= 2:
        n = _cell_triangle_counts(np.ascontiguousarray(f[::s, ::s, ::s]))
        for z in range(cz - 1):
            tri_of_layer[z >> 3] += int(n[z].sum())
    layer_tbase = np.concatenate([[0], np.cumsum(tri_of_layer)])
    assert layer_tbase[-1] == len(ref["triangles"])
    parts = []
    for z0, z1 in slabs:
        l0, l1 = slab_layers(f.shape, level, z0, z1)
        v0, v1 = int(tile_vbase[l0 * ntx * nty]), int(tile_vbase[l1 * ntx * nty])
        seam = (tile_vbase[l0 * ntx * nty:(l0 + 1) * ntx * nty] - v0).astype(np.uint32).reshape(nty, ntx)
        parts.append(dict(vertices=(v0, v1), triangles=(int(layer_tbase[l0]), int(layer_tbase[l1])), seam=seam, layers=(l0, l1)))
    ref = dict(ref, tile=tile, tile_vbase=tile_vbase, lattice_tiles=(ntx, nty, ntz))
    return ref, parts


def unlinked(ref, part):
    """the part's triangles as a slab holds them before a link: dict(local [T][3] int64 (own vertex: slab-local index, else -1),
    tile [T][3] (of an index into the slab above: its tile inside that slab's first layer, x fastest), offset [T][3] (behind that tile's base))"""
    (v0, v1), (t0, t1), (_, l1) = part["vertices"], part["triangles"], part["layers"]
    ntx, nty, _ = ref["lattice_tiles"]
    tri = ref["triangles"][t0:t1].astype(np.int64)
    assert (tri >= v0).all()                                             # a cell's corners lie in its own layer or above it
    own = tri < v1
    t = ref["tile"][np.minimum(tri, len(ref["tile"]) - 1)] if len(ref["tile"]) else np.zeros_like(tri)
    assert (own | (t // (ntx * nty) == l1)).all()                        # ... and no further than the first layer above
    return dict(local=np.where(own, tri - v0, -1), tile=np.where(own, 0, t - l1 * ntx * nty), offset=np.where(own, 0, tri - ref["tile_vbase"][t]),
                n_vertices=v1 - v0)


def link(u, vertex_base, above_seam):
    """tsdf_mesh_slab_link on unlinked(): own index -> vertex_base + local, index into the slab above -> vertex_base + n_vertices + above_seam[tile] + offset"""
    above = np.zeros(1, np.int64) if above_seam is None else np.asarray(above_seam, np.int64).reshape(-1)
    assert above_seam is not None or (u["local"] >= 0).all()
    idx = np.where(u["local"] >= 0, vertex_base + u["local"], vertex_base + u["n_vertices"] + above[u["tile"]] + u["offset"])
    return idx.astype(np.uint32)


def crosses_seam(ref, part):
    """triangles of the part that index vertices of the slab above"""
    t0, t1 = part["triangles"]
    return int((ref["triangles"][t0:t1] >= part["vertices"][1]).any(axis=1).sum())


def crafted_volume(res, slabs, seed, limit=0.05):
    """res = (rx, ry, rz): a seeded random field in [-limit, limit] with NaN, +inf, -inf, 0 and -0 planted in the seam planes z1 - 1, z1, z1 + 1 of
    every seam -> [rz][ry][rx] float32"""
    rng = np.random.default_rng(seed)
    vol = rng.uniform(-limit, limit, res[::-1]).astype(f32)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], f32)
    for _, z1 in slabs:
        if z1 >= res[2]:
            continue
        for z in (z1 - 1, z1, z1 + 1):
            if 0 <= z < res[2]:
                pick = rng.random(vol[z].shape) < 0.15
                vol[z][pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    return vol
