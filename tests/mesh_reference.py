"""numpy restatement of the mesh extraction's definition (include/rgbd_recon_hip.h, tsdf_mesh_extract), float32 throughout.

Marching tetrahedra on the voxel-centre lattice: Kuhn's six tetrahedra per cell, one vertex per crossed tetrahedron edge (owned by the
lattice point p of the edge p -> p + d), vertices ordered by (storage tile of p, p inside the tile, d), triangles by (storage tile of the
cell, cell inside the tile, tetrahedron, triangle).  The gradient and colour taps go through the oracle's sampling primitives
(oracle.tex3d, tex2d_linear, tex2d_nearest); everything else is elementwise float32 arithmetic in the order the definition gives.
"""
import numpy as np

f32 = np.float32
TETS = ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))
NORMALS, COLOURS = 1, 2


def corner_xyz(b):
    return np.array([b & 1, (b >> 1) & 1, b >> 2], np.float64)


def base_triangles(tet, case):
    """The triangles of one tetrahedron for one case (bit j: vertex j of the tetrahedron is inside) BEFORE the winding rule, each a
    tuple of three edges, an edge a pair of cell corners (x, y) with x < y."""
    v = TETS[tet]
    ins = [v[j] for j in range(4) if (case >> j) & 1]
    out = [v[j] for j in range(4) if not (case >> j) & 1]
    edge = lambda p, q: (min(p, q), max(p, q))
    if len(ins) in (0, 4):
        return []
    if len(ins) == 1 or len(out) == 1:
        a = ins[0] if len(ins) == 1 else out[0]
        return [tuple(edge(a, x) for x in v if x != a)]
    (a, b), (c, d) = ins, out
    return [(edge(a, c), edge(a, d), edge(b, d)), (edge(a, c), edge(b, d), edge(b, c))]


def _midpoint_normal(tri):
    p = [(corner_xyz(x) + corner_xyz(y)) * 0.5 for x, y in tri]
    return np.cross(p[1] - p[0], p[2] - p[0])


def winding_table():
    """6 words: bit `case` of word `tetrahedron` = the triangles of that case are emitted reversed.  Generated from the rule: with
    corner values +-1 (every vertex at its edge's midpoint) the geometric normal points from the inside corners to the outside ones."""
    words = []
    for k in range(6):
        w = 0
        for case in range(1, 15):
            v = TETS[k]
            cin = np.mean([corner_xyz(v[j]) for j in range(4) if (case >> j) & 1], axis=0)
            cout = np.mean([corner_xyz(v[j]) for j in range(4) if not (case >> j) & 1], axis=0)
            signs = [np.sign(np.dot(_midpoint_normal(t), cout - cin)) for t in base_triangles(k, case)]
            assert all(s != 0 for s in signs) and len(set(signs)) == 1, (k, case, signs)
            if signs[0] < 0:
                w |= 1 << case
        words.append(w)
    return words


_FLIP = winding_table()


def case_triangles(tet, case):
    """base_triangles with the winding applied: a reversed triangle (p, q, r) is (p, r, q)."""
    tris = base_triangles(tet, case)
    if (_FLIP[tet] >> case) & 1:
        tris = [(t[0], t[2], t[1]) for t in tris]
    return tris


def tetrahedron_parity(tet):
    v = [corner_xyz(b) for b in TETS[tet]]
    return int(np.sign(np.linalg.det(np.stack([v[1] - v[0], v[2] - v[0], v[3] - v[0]]))))


def _order_key(rz, ry, rx):
    """per lattice point: storage tile id (x fastest) * 512 + index inside the 8^3 tile (x fastest)"""
    z, y, x = np.meshgrid(np.arange(rz), np.arange(ry), np.arange(rx), indexing="ij")
    ntx, nty = (rx + 7) // 8, (ry + 7) // 8
    tile = ((z >> 3) * nty + (y >> 3)) * ntx + (x >> 3)
    return tile.astype(np.int64) * 512 + (((z & 7) << 6) | ((y & 7) << 3) | (x & 7))


def sanitised(vol, limit):
    vol = np.asarray(vol, f32)
    return np.where(np.isfinite(vol), vol, f32(-f32(limit))).astype(f32)


def extract(vol, limit, bbox_min, bbox_max):
    """vol [rz][ry][rx] -> dict(position [V][3] f32, unit [V][3] f32 (unit-cube positions), triangles [T][3] uint32)."""
    f = sanitised(vol, limit)
    rz, ry, rx = f.shape
    empty = dict(position=np.zeros((0, 3), f32), unit=np.zeros((0, 3), f32), triangles=np.zeros((0, 3), np.uint32))
    if min(rx, ry, rz) < 2:
        return empty
    inside = f > 0                                                   # zero and -0 are outside
    key = _order_key(rz, ry, rx)
    crossed = np.zeros((rz, ry, rx, 7), bool)
    for d in range(1, 8):
        bx, by, bz = d & 1, (d >> 1) & 1, d >> 2
        crossed[:rz - bz, :ry - by, :rx - bx, d - 1] = inside[:rz - bz, :ry - by, :rx - bx] != inside[bz:, by:, bx:]
    zz, yy, xx, dd = np.nonzero(crossed)
    order = np.argsort(key[zz, yy, xx] * 8 + dd, kind="stable")
    zz, yy, xx, dd = zz[order], yy[order], xx[order], dd[order] + 1
    vid = np.full((rz, ry, rx, 7), -1, np.int64)
    vid[zz, yy, xx, dd - 1] = np.arange(len(zz))
    # vertices
    qx, qy, qz = xx + (dd & 1), yy + ((dd >> 1) & 1), zz + (dd >> 2)
    a, b = f[zz, yy, xx], f[qz, qy, qx]
    with np.errstate(over="ignore"):
        t = (a / (a - b)).astype(f32)
    bmin, bmax = np.asarray(bbox_min, f32), np.asarray(bbox_max, f32)
    ext = (bmax - bmin).astype(f32)
    unit = np.zeros((len(zz), 3), f32)
    for axis, (p, q, r) in enumerate(((xx, qx, rx), (yy, qy, ry), (zz, qz, rz))):
        up = (p.astype(f32) + f32(0.5)) / f32(r)
        uq = (q.astype(f32) + f32(0.5)) / f32(r)
        unit[:, axis] = up + t * (uq - up)
    position = (bmin[None, :] + unit * ext[None, :]).astype(f32)
    # triangles
    cz, cy, cx = rz - 1, ry - 1, rx - 1
    corner = [inside[(b >> 2):(b >> 2) + cz, ((b >> 1) & 1):((b >> 1) & 1) + cy, (b & 1):(b & 1) + cx] for b in range(8)]
    rows, keys = [], []
    for k in range(6):
        case = sum(corner[TETS[k][j]].astype(np.int64) << j for j in range(4))
        for cs in range(1, 15):
            z, y, x = np.nonzero(case == cs)
            if len(z) == 0:
                continue
            for n, tri in enumerate(case_triangles(k, cs)):
                idx = [vid[z + (p >> 2), y + ((p >> 1) & 1), x + (p & 1), (q - p) - 1] for p, q in tri]
                rows.append(np.stack(idx, -1))
                keys.append((key[z, y, x] * 6 + k) * 2 + n)
    if not rows:
        return dict(position=position, unit=unit, triangles=np.zeros((0, 3), np.uint32))
    rows, keys = np.concatenate(rows), np.concatenate(keys)
    assert (rows >= 0).all()
    return dict(position=position, unit=unit, triangles=rows[np.argsort(keys, kind="stable")].astype(np.uint32))


def normalize3(a):
    a = np.asarray(a, f32)
    with np.errstate(all="ignore"):
        s = f32(1.0) / np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2])
        return (a * s[:, None]).astype(f32)


def normals(vol, limit, bbox_min, bbox_max, unit):
    """get_gradient (tsdf_raymarch.fs:140-149) on the volume as stored (NaN voxels stay NaN), then inverseTranspose(vol_to_world) of -gn."""
    from oracle import oracle as orc
    t = np.ascontiguousarray(np.asarray(vol, f32)[..., None])
    sd = f32(limit) * f32(0.5)
    g = np.zeros((len(unit), 3), f32)
    for i, u in enumerate(np.asarray(unit, f32)):
        for axis in range(3):
            hi, lo = u.copy(), u.copy()
            hi[axis] = u[axis] + sd
            lo[axis] = u[axis] - sd
            g[i, axis] = orc.tex3d(t, *hi)[0] - orc.tex3d(t, *lo)[0]
    gn = normalize3(g)
    ext = (np.asarray(bbox_max, f32) - np.asarray(bbox_min, f32)).astype(f32)
    with np.errstate(all="ignore"):
        return normalize3((-gn) / ext[None, :])


def colours(scene, limit, unit):
    """blendColors (tsdf_raymarch.fs:295-330) of the scene's frame at the unit-cube positions: rgba, alpha +1 valid / -1 fallback."""
    from oracle import oracle as orc
    n, nv = scene["n"], len(unit)
    limit = f32(limit)
    rgb = (np.asarray(scene["color"], np.uint8).astype(f32) / f32(255.0)).astype(f32)
    depth = np.ascontiguousarray(scene["depth"], f32)
    quality = np.ascontiguousarray(np.asarray(scene["quality"], f32)[..., None])
    ri, rl = [int(x) for x in scene["inv_res"]], [int(x) for x in scene["lut_res"]]
    tc, tc2 = np.zeros((nv, 3), f32), np.zeros((nv, 3), f32)
    tw, tw2 = np.zeros(nv, f32), np.zeros(nv, f32)
    with np.errstate(all="ignore"):
        for i in range(n):
            inv = np.asarray(scene["cv_xyz_inv"][i], f32).reshape(ri[2], ri[1], ri[0], 4)
            uv = np.asarray(scene["cv_uv"][i], f32).reshape(rl[2], rl[1], rl[0], 2)
            pc = np.stack([orc.tex3d(inv, *u)[:3] for u in unit]).astype(f32) if nv else np.zeros((0, 3), f32)
            pcol = np.stack([orc.tex3d(uv, *p) for p in pc]).astype(f32) if nv else np.zeros((0, 2), f32)
            col = np.stack([orc.tex2d_linear(rgb, i, p[0], p[1]) for p in pcol]).astype(f32) if nv else np.zeros((0, 3), f32)
            d = np.array([orc.tex2d_nearest(depth, i, p[0], p[1], 0) for p in pc], f32)
            q = np.array([orc.tex2d_linear(quality, i, p[0], p[1])[0] for p in pc], f32)
            dist = np.abs(d - pc[:, 2]).astype(f32)
            q = np.where(dist < limit, q, f32(0.0)).astype(f32)
            de = dist + f32(0.01)
            tc = tc + col * q[:, None] / de[:, None]
            tw = tw + q / de
            tc2 = tc2 + col / dist[:, None]
            tw2 = tw2 + f32(1.0) / dist
        valid = tw > 0
        out = np.zeros((nv, 4), f32)
        out[:, :3] = np.where(valid[:, None], tc / tw[:, None], tc2 / tw2[:, None])
        out[:, 3] = np.where(valid, f32(1.0), f32(-1.0))
    return out


# ---- checks shared by the CPU and the GPU tests
def canonical(tri):
    """every triangle rotated to its smallest index first: keeps the winding"""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    k = np.argmin(tri, axis=1)
    i = np.arange(len(tri))
    return np.stack([tri[i, k], tri[i, (k + 1) % 3], tri[i, (k + 2) % 3]], -1)


def manifold_report(tri, n_vertices):
    """closed 2-manifold facts of an indexed mesh: every undirected edge shared by exactly two triangles, once in each direction"""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    a = np.concatenate([tri[:, 0], tri[:, 1], tri[:, 2]])
    b = np.concatenate([tri[:, 1], tri[:, 2], tri[:, 0]])
    directed = a * n_vertices + b
    undirected = np.minimum(a, b) * n_vertices + np.maximum(a, b)
    _, counts = np.unique(undirected, return_counts=True)
    used = np.unique(tri)
    return dict(directed_unique=len(np.unique(directed)) == len(directed), edges=len(counts), edges_shared_by_two=bool((counts == 2).all()),
                opposite=bool(np.isin(b * n_vertices + a, directed).all()), vertices_used=len(used), faces=len(tri),
                euler=len(used) - len(counts) + len(tri), degenerate=int((a == b).sum()))


def signed_volume(position, tri):
    p = np.asarray(position, np.float64)
    t = np.asarray(tri, np.int64).reshape(-1, 3)
    return float(np.einsum("ij,ij->i", p[t[:, 0]], np.cross(p[t[:, 1]], p[t[:, 2]])).sum() / 6.0)


def sphere_volume(res=(24, 16, 16), radius=0.3, limit=0.05):
    """a sphere's truncated signed distance, positive INSIDE (the side the raymarch's hit test f > 0 calls the surface), [rz][ry][rx]"""
    rx, ry, rz = res
    z, y, x = np.meshgrid((np.arange(rz) + 0.5) / rz, (np.arange(ry) + 0.5) / ry, (np.arange(rx) + 0.5) / rx, indexing="ij")
    d = radius - np.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2)
    return np.clip(d, -limit, limit).astype(f32)
