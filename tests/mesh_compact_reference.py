"""numpy restatement of the streamed mesh's tile-local triangle format (include/rgbd_recon_hip.h, "mesh streaming: compact triangles"), on top of the
references that exist.  Nothing here knows a cell: a vertex's tile comes from the lattice point that owns it (mesh_lod_reference.extract_lod's `voxel`),
a triangle's tile is the smallest of its corners' tiles -- every triangle has a corner owned by its cell's origin, and the +x / +y / +z neighbours'
linear ids are larger."""
import numpy as np

import mesh_stream_filter_reference as SF

ROW = np.dtype([("tile", "<u4"), ("first_vertex", "<u4"), ("first_triangle", "<u4"), ("n_triangles", "<u4")])   # tsdf_mesh_tile_row


def tile_grid(shape, level):
    """(tx, ty, tz) = ceil(ceil(r / s) / 8) per axis of a [rz][ry][rx] volume"""
    s = 1 << level
    return tuple(((r + s - 1) // s + 7) // 8 for r in shape[::-1])


def vertex_tiles(mesh, level, shape):
    """the linear lattice-tile id (x fastest) of every vertex's owner: `voxel` is the lower end of the voxel edge the descent ended on, at most
    s - 1 voxels along the lattice edge from the owner"""
    tx, ty, _ = tile_grid(shape, level)
    t = (np.asarray(mesh["voxel"], np.int64).reshape(-1, 3) >> level) >> 3
    return (t[:, 2] * ty + t[:, 1]) * tx + t[:, 0]


def encode_tiles(vt, triangles, tiles):
    """vt: the tile of every vertex (ascending); triangles: uint32 [T][3] -> (table ROW [R], codes uint16 [T][3])"""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    vt = np.asarray(vt, np.int64)
    assert (np.diff(vt) >= 0).all()
    ids = np.unique(vt)
    table = np.zeros(len(ids), ROW)
    table["tile"], table["first_vertex"] = ids, np.searchsorted(vt, ids)
    ct = vt[tri]                                                          # the corners' tiles; the cell's is the smallest
    tt = ct.min(axis=1) if len(tri) else np.zeros(0, np.int64)
    assert (np.diff(tt) >= 0).all()
    table["first_triangle"] = np.searchsorted(tt, ids)
    table["n_triangles"] = np.searchsorted(tt, ids, side="right") - table["first_triangle"]
    assert table["n_triangles"].sum() == len(tri)                         # every triangle's tile has a row
    tx, ty = int(tiles[0]), int(tiles[1])
    xyz = lambda t: np.stack([t % tx, t // tx % ty, t // (tx * ty)], -1)
    d = xyz(ct) - xyz(tt)[:, None, :]
    assert ((d >= 0) & (d <= 1)).all()
    offset = tri - table["first_vertex"].astype(np.int64)[np.searchsorted(ids, ct)]
    assert ((offset >= 0) & (offset < 3584)).all()
    return table, (offset | ((d[..., 0] + 2 * d[..., 1] + 4 * d[..., 2]) << 12)).astype(np.uint16)


def encode(mesh, level, shape):
    """mesh: mesh_lod_reference.extract_lod(vol, ..., level) of a [rz][ry][rx] = shape volume -> (table, codes, tiles)"""
    tiles = tile_grid(shape, level)
    return encode_tiles(vertex_tiles(mesh, level, shape), mesh["triangles"], tiles) + (tiles,)


def encode_filtered(mesh, level, shape, min_triangles):
    """the frame without its components of fewer than min_triangles triangles -> (table, codes, tiles, kept-vertex mask)"""
    tiles = tile_grid(shape, level)
    kept, mask, _ = SF.filter_mesh(dict(unit=mesh["unit"], triangles=mesh["triangles"]), min_triangles)
    return encode_tiles(vertex_tiles(mesh, level, shape)[mask], kept["triangles"], tiles) + (tiles, mask)


def decode(table, codes, tiles):
    """the header's decoding rule -> uint32 [T][3]"""
    codes = np.asarray(codes, np.uint16).reshape(-1, 3).astype(np.int64)
    if not len(codes):
        return np.zeros((0, 3), np.uint32)
    row = np.repeat(np.arange(len(table)), table["n_triangles"].astype(np.int64))
    owner = (table["tile"].astype(np.int64)[row][:, None] + ((codes >> 12) & 1) + ((codes >> 13) & 1) * tiles[0] + ((codes >> 14) & 1) * tiles[0] * tiles[1])
    owner_row = np.searchsorted(table["tile"], owner.ravel(), side="right").reshape(owner.shape) - 1
    return (table["first_vertex"].astype(np.int64)[owner_row] + (codes & 0xfff)).astype(np.uint32)


def payload_bytes(n_vertices, stride, rows, n_triangles):
    return (n_vertices * stride + 15) // 16 * 16 + rows * 16 + n_triangles * 6 if n_vertices else 0


def checkerboard(n=16, limit=0.04):
    """+-limit by the parity of x + y + z: every lattice edge along an axis is crossed, the densest mesh a grid carries"""
    z, y, x = np.indices((n, n, n))
    return np.where((x + y + z) & 1, limit, -limit).astype(np.float32)
