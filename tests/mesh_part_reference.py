"""numpy restatement of the streamed slab parts (include/rgbd_recon_hip.h, "mesh streaming: slab parts"), composed of the references that exist:
mesh_slab_reference.split (which vertices and triangles a slab owns), mesh_pack_reference.pack (the packed vertex) and mesh_compact_reference.encode_tiles
(table rows and corner codes).

A part is encoded from what its slab can know: the vertices of its own lattice tile layers and of the first layer above them (the seam layer, whose
plane-0 offsets the slab computes from its halo), with indices local to that range.  Nothing of the whole frame's table is consulted; that the joined
parts equal mesh_compact_reference.encode of the whole mesh is what the tests check."""
import numpy as np

import mesh_compact_reference as MC
import mesh_pack_reference as P
import mesh_slab_reference as S

ROW = MC.ROW


def parts(vol, limit, bbox_min, bbox_max, level, slabs, normal=None, colour=None):
    """-> (ref, parts): ref = mesh_slab_reference.split's whole mesh; parts[k] for slabs[k] = (z0, z1) =
    dict(vertices (packed), table (ROW, tile in the WHOLE grid, first_vertex / first_triangle part-local), codes uint16 [T][3], tiles, layers, top,
    level, overflow=0).  normal / colour: the whole mesh's attribute arrays (or None), packed by the streaming rule."""
    ref, split = S.split(vol, limit, bbox_min, bbox_max, level, slabs)
    tiles = MC.tile_grid(vol.shape, level)
    per_layer = tiles[0] * tiles[1]
    packed = P.pack(ref["unit"], normal, colour)
    out = []
    for p in split:
        (v0, v1), (t0, t1), (l0, l1) = p["vertices"], p["triangles"], p["layers"]
        top = l1 == tiles[2]
        seam_end = int(ref["tile_vbase"][min(l1 + 1, tiles[2]) * per_layer])     # the seam layer's vertices follow the owned ones in the whole order
        local_tri = ref["triangles"][t0:t1].astype(np.int64) - v0
        assert (local_tri >= 0).all() and (local_tri < seam_end - v0).all()     # a cell's corners lie in its own layer or the one above
        table, codes = MC.encode_tiles(ref["tile"][v0:seam_end], local_tri, tiles)
        own = table["tile"] < l1 * per_layer                                  # a seam tile has a record in the slab, but no row in its part
        assert not table["n_triangles"][~own].any()
        out.append(dict(vertices=packed[v0:v1], table=table[own], codes=codes, tiles=tiles, layers=(l0, l1), top=top, level=level, overflow=0,
                        seam_tiles=int((~own).sum())))
    return ref, out


def join(parts):
    """the header's join rule: parts of contiguous slabs in slab order -> (vertices, table, codes); ValueError when a part overflowed (the frame is
    dropped whole) or the slabs are not contiguous"""
    if not parts:
        raise ValueError("no part")
    if any(p.get("overflow", 0) for p in parts):
        raise ValueError("a part overflowed: the frame is dropped whole")
    for a, b in zip(parts, parts[1:]):
        if a["layers"][1] != b["layers"][0]:
            raise ValueError("the parts are not contiguous in slab order")
    rows, nv, nt = [], 0, 0
    for p in parts:
        t = np.array(p["table"], ROW)
        t["first_vertex"] += np.uint32(nv)
        t["first_triangle"] += np.uint32(nt)
        rows.append(t)
        nv += len(p["vertices"])
        nt += len(p["codes"])
    return (np.concatenate([p["vertices"] for p in parts]), np.concatenate(rows), np.concatenate([np.asarray(p["codes"], np.uint16).reshape(-1, 3) for p in parts]))


def seam_codes(part):
    """corner codes of the part with dz = 1 (bit 14) whose owner row lies in the next part: the owner tile is in the first layer above the owned ones"""
    codes = np.asarray(part["codes"], np.int64).reshape(-1, 3)
    if not len(codes):
        return 0
    tx, ty, _ = part["tiles"]
    row = np.repeat(np.arange(len(part["table"])), part["table"]["n_triangles"].astype(np.int64))
    owner = part["table"]["tile"].astype(np.int64)[row][:, None] + ((codes >> 12) & 1) + ((codes >> 13) & 1) * tx + ((codes >> 14) & 1) * tx * ty
    return int((((codes >> 14) & 1) == 1)[owner >= part["layers"][1] * tx * ty].sum())


def payload_bytes(part, stride):
    return MC.payload_bytes(len(part["vertices"]), stride, len(part["table"]), len(part["codes"]))
