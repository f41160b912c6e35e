"""numpy restatement of the mesh level of detail (include/rgbd_recon_hip.h, "mesh level of detail"), on top of tests/mesh_reference.py.

Level L has stride s = 1 << L.  The lattice is vol[::s, ::s, ::s] (point samples).  The topology is mesh_reference.extract of that lattice: its triangle
array IS the level's triangle array, so the existing reference pins the topology.  The owners are recomputed here in mesh_reference._order_key order and
every vertex is placed by the descent: bisection along the lattice edge to the voxel edge that carries the surface, then the level-0 vertex of that
voxel edge at the FULL resolution.  float32 throughout, in the order the header gives."""
import numpy as np

import mesh_reference as M

f32 = np.float32


def lattice_shape(shape, level):
    """(cz, cy, cx) = ceil(r / s) per axis"""
    s = 1 << level
    return tuple((r + s - 1) // s for r in shape)


def lattice_tiles(shape, level):
    """the number of 8^3 lattice tiles of a [rz][ry][rx] volume at a level"""
    cz, cy, cx = lattice_shape(shape, level)
    return ((cx + 7) // 8) * ((cy + 7) // 8) * ((cz + 7) // 8)


def descend(f, x, y, z, bx, by, bz, level):
    """The descent of the definition on arrays of edges.  f: the sanitised volume [rz][ry][rx]; (x, y, z): the VOXEL P = s * p of every edge's lower
    end; (bx, by, bz): its 0/1 offset vector d.  Returns the voxel P after `level` steps: P and P + d are neighbours, exactly one of them inside."""
    x, y, z = (np.array(v, np.int64) for v in (x, y, z))
    inside = f[z, y, x] > 0
    h = (1 << level) >> 1
    while h >= 1:
        mx, my, mz = x + h * bx, y + h * by, z + h * bz
        same = (f[mz, my, mx] > 0) == inside
        x, y, z = np.where(same, mx, x), np.where(same, my, y), np.where(same, mz, z)
        h >>= 1
    assert ((f[z + bz, y + by, x + bx] > 0) != inside).all()            # the invariant: the other end is on the other side
    return x, y, z


def extract_lod(vol, limit, bbox_min, bbox_max, level):
    """vol [rz][ry][rx] -> dict(position [V][3] f32, unit [V][3] f32, triangles [T][3] uint32, voxel [V][3] (x, y, z of the voxel edge's lower end),
    d [V] (the edge's bit offset), tiles, tiles_with_surface (8^3 lattice tiles)) of level 0, 1 or 2."""
    assert level in (0, 1, 2)
    s = 1 << level
    f = M.sanitised(vol, limit)
    rz, ry, rx = f.shape
    sub = np.ascontiguousarray(f[::s, ::s, ::s])
    cz, cy, cx = sub.shape
    assert (cz, cy, cx) == lattice_shape(f.shape, level)
    base = M.extract(sub, limit, bbox_min, bbox_max)                     # the topology: its triangles are the level's, byte for byte
    out = dict(position=np.zeros((0, 3), f32), unit=np.zeros((0, 3), f32), triangles=base["triangles"], voxel=np.zeros((0, 3), np.int64),
               d=np.zeros(0, np.int64), tiles=lattice_tiles(f.shape, level), tiles_with_surface=0)
    if min(cx, cy, cz) < 2:
        assert len(base["position"]) == 0 and len(base["triangles"]) == 0
        return out
    # owners, in _order_key order: lattice tile (x fastest), owner inside the tile, d
    inside = sub > 0
    key = M._order_key(cz, cy, cx)
    crossed = np.zeros((cz, cy, cx, 7), bool)
    for d in range(1, 8):
        bx, by, bz = d & 1, (d >> 1) & 1, d >> 2
        crossed[:cz - bz, :cy - by, :cx - bx, d - 1] = inside[:cz - bz, :cy - by, :cx - bx] != inside[bz:, by:, bx:]
    zz, yy, xx, dd = np.nonzero(crossed)
    order = np.argsort(key[zz, yy, xx] * 8 + dd, kind="stable")
    zz, yy, xx, dd = zz[order], yy[order], xx[order], dd[order] + 1
    assert len(zz) == len(base["position"])                             # one vertex per crossed edge, as that extract counts them
    bx, by, bz = dd & 1, (dd >> 1) & 1, dd >> 2
    # positions: descent, then the level-0 vertex of the voxel edge at the full resolution
    px, py, pz = descend(f, xx * s, yy * s, zz * s, bx, by, bz, level)
    qx, qy, qz = px + bx, py + by, pz + bz
    a, b = f[pz, py, px], f[qz, qy, qx]
    with np.errstate(over="ignore"):
        t = (a / (a - b)).astype(f32)
    bmin, bmax = np.asarray(bbox_min, f32), np.asarray(bbox_max, f32)
    ext = (bmax - bmin).astype(f32)
    unit = np.zeros((len(zz), 3), f32)
    for axis, (p, q, r) in enumerate(((px, qx, rx), (py, qy, ry), (pz, qz, rz))):
        up = (p.astype(f32) + f32(0.5)) / f32(r)
        uq = (q.astype(f32) + f32(0.5)) / f32(r)
        unit[:, axis] = up + t * (uq - up)
    out.update(position=(bmin[None, :] + unit * ext[None, :]).astype(f32), unit=unit, voxel=np.stack([px, py, pz], -1), d=dd,
               tiles_with_surface=len(np.unique(key[zz, yy, xx] >> 9)))
    return out


def empty_lattice_tiles(vol, limit, level):
    """lattice tiles whose (s + 1)^3 storage tiles [ct s, ct s + s] per axis, clipped to the grid, hold nothing but -limit: the tiles a class skip can
    take at best (a device's class says "all -limit" only for tiles it never integrated into, so it may skip fewer, never others)"""
    s = 1 << level
    f = np.asarray(vol, f32)
    rz, ry, rx = f.shape
    cz, cy, cx = lattice_shape(f.shape, level)
    n = 0
    for tz in range((cz + 7) // 8):
        for ty in range((cy + 7) // 8):
            for tx in range((cx + 7) // 8):
                box = f[tz * s * 8:min((tz * s + s + 1) * 8, rz), ty * s * 8:min((ty * s + s + 1) * 8, ry), tx * s * 8:min((tx * s + s + 1) * 8, rx)]
                n += int((box == f32(-f32(limit))).all())
    return n


def random_volume(res, seed=20221019, limit=0.04):
    """res = (rx, ry, rz): uniform in +-limit with ~10 % exact zeros and ~2 % of -0, NaN, +inf, -inf (tests/test_gpu_mesh.py's random volume)"""
    rng = np.random.default_rng(seed)
    vol = rng.uniform(-limit, limit, res[::-1]).astype(f32)
    vol[rng.random(vol.shape) < 0.10] = 0.0
    special = np.array([-0.0, np.nan, np.inf, -np.inf], f32)
    pick = rng.random(vol.shape) < 0.02
    vol[pick] = special[rng.integers(0, 4, int(pick.sum()))]
    return vol
