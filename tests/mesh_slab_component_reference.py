"""numpy restatement of the mesh components on Z-slab contexts (include/rgbd_recon_hip.h, "mesh components on Z-slab contexts"), on top of
tests/mesh_slab_reference.py (the split into parts) and tests/mesh_component_reference.py (the components' definition): the definition, not the
device's algorithm.

A part is labelled from its OWN triangles only (global indices: own vertices and, in the top cell layer, vertices of the slab above); what crosses a seam
leaves the slab as three sorted lists; the merge joins the lists of all slabs (here: the components of a graph over the root records, labelled by
mesh_component_reference.labels itself); the link turns a slab's merged links into global numbers.  The joined results must equal
mesh_component_reference.components of the whole reference mesh byte for byte."""
import numpy as np

import mesh_component_reference as K
import mesh_slab_reference as S

SEAM_VERTEX = np.dtype([("vertex", "<u4"), ("root", "<u4")])                                                # tsdf_mesh_seam_vertex
SEAM_ROOT = np.dtype([("root", "<u4"), ("rank", "<u4"), ("n_vertices", "<u4"), ("n_triangles", "<u4")])    # tsdf_mesh_seam_root
LINK = np.dtype([("root", "<u4"), ("final_root", "<u4"), ("component", "<u4"), ("reserved0", "<u4"),
                 ("n_vertices", "<u4"), ("n_triangles", "<u4"), ("reserved1", "<u4"), ("reserved2", "<u4")])  # tsdf_mesh_component_link


def label_part(ref, part, level):
    """step 1 on one part of S.split's (ref, parts): dict(vertex_base, n_vertices, n_local, down, up, roots -- the merge's input -- and label (local
    root of every local index), own_roots, local_table (K.TABLE, first_vertex global) for the link)"""
    (v0, v1), (t0, t1), (l0, _) = part["vertices"], part["triangles"], part["layers"]
    nv = v1 - v0
    tri = ref["triangles"][t0:t1].astype(np.int64)
    end = max(v1, int(tri.max()) + 1) if tri.size else v1                # the own vertices and whatever of the slab above the triangles name
    label = K.labels(tri - v0, end - v0).astype(np.int64)
    assert tri.size == 0 or ((tri >= v0) & (tri < v1)).any(axis=1).all()   # every triangle of a part has an own vertex ...
    assert (label[nv:][label[nv:] != np.arange(nv, end - v0)] < nv).all()  # ... so a used vertex of the slab above hangs under an own root
    own_roots = np.flatnonzero(label[:nv] == np.arange(nv))
    rank = np.searchsorted(own_roots, label)                              # (of a root; meaningful where label < nv)
    table = np.zeros(len(own_roots), K.TABLE)
    table["first_vertex"] = v0 + own_roots
    table["n_vertices"] = np.bincount(rank[:nv], minlength=len(own_roots))
    table["n_triangles"] = np.bincount(rank[tri[:, 0] - v0], minlength=len(own_roots)) if tri.size else 0
    used_above = nv + np.flatnonzero(label[nv:] != np.arange(nv, end - v0))
    up = np.zeros(len(used_above), SEAM_VERTEX)
    up["vertex"], up["root"] = v0 + used_above, v0 + label[used_above]
    lattice_z = ref["voxel"][v0:v1, 2] // (1 << level)
    plane0 = np.flatnonzero(lattice_z == l0 * 8) if l0 > 0 else np.zeros(0, np.int64)   # what the slab below can index
    down = np.zeros(len(plane0), SEAM_VERTEX)
    down["vertex"], down["root"] = v0 + plane0, v0 + label[plane0]
    seam_roots = np.unique(np.concatenate([label[used_above], label[plane0]])).astype(np.int64)
    roots = np.zeros(len(seam_roots), SEAM_ROOT)
    roots["root"], roots["rank"] = v0 + seam_roots, rank[seam_roots]
    roots["n_vertices"], roots["n_triangles"] = table["n_vertices"][rank[seam_roots]], table["n_triangles"][rank[seam_roots]]
    return dict(vertex_base=v0, n_vertices=nv, n_local=len(own_roots), down=down, up=up, roots=roots, label=label, own_roots=own_roots, local_table=table,
                triangles=tri)


def merge(slabs):
    """step 2 as a definition: the root records are the nodes of a graph, an up record and the down record of the same vertex in the slab above an
    edge; a node's final root is the smallest node of its class.  -> dict(component_base, links (one LINK array per slab), n_components)"""
    first = np.concatenate([[0], np.cumsum([len(s["roots"]) for s in slabs])]).astype(np.int64)
    edges = []
    for k, s in enumerate(slabs[:-1]):
        a = slabs[k + 1]
        at = np.searchsorted(a["down"]["vertex"], s["up"]["vertex"])
        assert (a["down"]["vertex"][at] == s["up"]["vertex"]).all()      # every up record has its partner
        lo = first[k] + np.searchsorted(s["roots"]["root"], s["up"]["root"])
        hi = first[k + 1] + np.searchsorted(a["roots"]["root"], a["down"]["root"][at])
        edges.append(np.stack([lo, hi, hi], axis=1))
    assert not len(slabs) or not len(slabs[-1]["up"])
    top = K.labels(np.concatenate(edges) if edges else np.zeros((0, 3), np.int64), int(first[-1])).astype(np.int64)
    records = np.concatenate([s["roots"] for s in slabs])
    nv, nt = np.bincount(top, records["n_vertices"], len(top)).astype(np.int64), np.bincount(top, records["n_triangles"], len(top)).astype(np.int64)
    base, links = [0], []
    number = np.zeros(len(top), np.int64)
    for k, s in enumerate(slabs):
        nodes = np.arange(first[k], first[k + 1])
        removed = top[nodes] != nodes
        number[nodes] = base[k] + s["roots"]["rank"] - (np.cumsum(removed) - removed)
        base.append(base[k] + s["n_local"] - int(removed.sum()))
    for k, s in enumerate(slabs):
        t = top[first[k]:first[k + 1]]
        out = np.zeros(len(t), LINK)
        out["root"], out["final_root"], out["component"] = s["roots"]["root"], records["root"][t], number[t]
        out["n_vertices"], out["n_triangles"] = nv[t], nt[t]
        links.append(out)
    return dict(component_base=base[:-1], links=links, n_components=base[-1])


def link(lab, component_base, links):
    """step 3 on label_part's result: (vertex_component [V] uint32, triangle_component [T] uint32, table of the owned components)"""
    v0, nv = lab["vertex_base"], lab["n_vertices"]
    roots = lab["own_roots"]
    link_of = np.full(len(roots), -1, np.int64)
    link_of[np.searchsorted(v0 + roots, links["root"])] = np.arange(len(links))
    linked = link_of >= 0
    links = links if len(links) else np.zeros(1, LINK)                    # (nothing is linked then: the one row is never taken)
    final = ~linked | (links["final_root"][link_of] == links["root"][link_of])
    number = np.where(linked, links["component"][link_of].astype(np.int64), component_base + np.cumsum(final) - final)
    table = lab["local_table"][final].copy()
    boundary = linked[final]
    table["n_vertices"][boundary] = links["n_vertices"][link_of[final][boundary]]
    table["n_triangles"][boundary] = links["n_triangles"][link_of[final][boundary]]
    rank = np.searchsorted(roots, lab["label"])
    vertex_component = number[rank[:nv]].astype(np.uint32)
    tri = lab["triangles"]
    triangle_component = number[rank[tri[:, 0] - v0]].astype(np.uint32) if tri.size else np.zeros(0, np.uint32)
    return vertex_component, triangle_component, table


def components_of_parts(ref, parts, level, merged=None):
    """the whole protocol -> dict(labs, merged, results=[link(...) per part], joined=(vertex_component, triangle_component, table))"""
    labs = [label_part(ref, p, level) for p in parts]
    merged = merged or merge(labs)
    results = [link(lab, merged["component_base"][k], merged["links"][k]) for k, lab in enumerate(labs)]
    return dict(labs=labs, merged=merged, results=results, joined=tuple(np.concatenate([r[j] for r in results]) for j in range(3)))


def figures(ref, parts, run):
    """what makes a case worth running: dict(components, spanning (>= 2 slabs), spanning3 (>= 3), per_seam (components with vertices on both sides of
    each seam), local, removed (per slab), own_slab (roots under a root of their OWN slab: joined only through another slab), up_records)"""
    vc = run["joined"][0].astype(np.int64)
    n = len(run["joined"][2])
    inside = np.zeros((len(parts), n), bool)
    for k, p in enumerate(parts):
        inside[k, np.unique(vc[p["vertices"][0]:p["vertices"][1]])] = True
    slabs_of = inside.sum(axis=0)
    links, labs = run["merged"]["links"], run["labs"]
    return dict(components=n, spanning=int((slabs_of >= 2).sum()), spanning3=int((slabs_of >= 3).sum()),
                per_seam=[int((inside[k] & inside[k + 1]).sum()) for k in range(len(parts) - 1)],
                local=[lab["n_local"] for lab in labs], removed=[int((l["final_root"] != l["root"]).sum()) for l in links],
                own_slab=sum(int(((l["final_root"] != l["root"]) & (l["final_root"] >= lab["vertex_base"])).sum()) for l, lab in zip(links, labs)),
                up_records=sum(len(lab["up"]) for lab in labs))


# ---- the test volumes
def columns_volume(res, limit=0.05):
    """res = (rx, ry, rz) -> [rz][ry][rx]: everything -limit but a U, an inverted U, an N of three columns and a straight column on a tile corner, all
    two voxels thick and as tall as the volume: in Z-slabs their columns are separate local components that only another slab joins"""
    rx, ry, rz = res
    vol = np.full((rz, ry, rx), -limit, np.float32)
    bot, top = 2, rz - 3
    for box in [(slice(bot, top), slice(2, 4), slice(2, 4)), (slice(bot, top), slice(2, 4), slice(7, 9)), (slice(top - 2, top), slice(2, 4), slice(2, 9)),
                (slice(bot, top), slice(7, 9), slice(13, 15)), (slice(bot, top), slice(7, 9), slice(18, 20)), (slice(bot, bot + 2), slice(7, 9), slice(13, 20)),
                (slice(bot, top), slice(13, 15), slice(2, 4)), (slice(bot, top), slice(13, 15), slice(6, 8)), (slice(bot, top), slice(13, 15), slice(10, 12)),
                (slice(top - 2, top), slice(13, 15), slice(2, 8)), (slice(bot, bot + 2), slice(13, 15), slice(6, 12)),
                (slice(bot, top), slice(15, 17), slice(15, 17))]:
        vol[box] = limit
    return vol


def case_volume(kind, res, slabs, limit=0.05):
    if kind == "columns":
        return columns_volume(res, limit)
    if kind == "speckle":
        return K.speckle_volume(res, limit=limit)
    return S.crafted_volume(res, slabs, 20261021, limit)                 # NaN, +-inf, 0 and -0 in the seam planes


# ---- the cases the CPU and the GPU tests share: kind, (rx, ry, rz), level, slabs (voxel planes).  tests/test_mesh_slab_component_reference.py asserts
# that none of them is vacuous: components span every seam, the columns are joined only through another slab, the 4-slab cases span three slabs.
BBOX = ((-1.0, 0.0, -1.0), (1.0, 2.2, 1.0))
LIMIT = 0.05
FOUR = [(0, 8), (8, 16), (16, 24), (24, 32)]
CASES = [("columns", (24, 20, 32), 0, FOUR),
         ("columns", (24, 20, 32), 0, [(0, 16), (16, 32)]),
         ("columns", (24, 20, 28), 0, [(0, 8), (8, 24), (24, 28)]),
         ("speckle", (32, 32, 32), 0, FOUR),
         ("speckle", (20, 12, 28), 0, [(0, 8), (8, 24), (24, 28)]),
         ("crafted", (32, 32, 32), 0, [(0, 16), (16, 32)]),
         ("speckle", (24, 20, 64), 1, [(0, 32), (32, 64)]),
         ("speckle", (24, 20, 64), 2, [(0, 32), (32, 64)]),
         ("columns", (24, 20, 64), 1, [(0, 32), (32, 64)]),
         ("crafted", (37, 43, 35), 0, [(0, 35)]),                          # the one-slab case, levels 0 .. 2
         ("crafted", (37, 43, 35), 1, [(0, 35)]),
         ("crafted", (37, 43, 35), 2, [(0, 35)])]
