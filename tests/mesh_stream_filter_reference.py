"""The filtered streamed frame (tsdf_mesh_stream_config_filter with min_triangles >= 1), composed from the references that exist: the extraction's
(mesh_reference / mesh_lod_reference), the components' keep (mesh_component_reference) and the packing (mesh_pack_reference).  No arithmetic of its own."""
import numpy as np

import mesh_component_reference as K
import mesh_lod_reference as LOD
import mesh_pack_reference as P
import mesh_reference as M


def filter_mesh(mesh, min_triangles):
    """(the mesh without the components of fewer than min_triangles triangles, the kept-vertex mask [V],
    (components, kept, vertices removed, triangles removed))"""
    tri = np.asarray(mesh["triangles"], np.uint32).reshape(-1, 3)
    nv = len(mesh["unit"])
    vc, _, table = K.components(tri, nv)
    flags = table["n_triangles"] >= min_triangles
    kept = K.keep(dict(mesh, position=mesh["unit"]), flags)                # (keep counts the vertices by "position")
    words = (len(table), int(flags.sum()), nv - len(kept["unit"]), len(tri) - len(kept["triangles"]))
    return kept, flags[vc] if nv else np.zeros(0, bool), words


def filtered_frame(vol, limit, bbox_min, bbox_max, min_triangles, level=0, normal=None, colour=None):
    """-> (packed vertices, triangles, (components, kept, vertices removed, triangles removed)) of the frame the ring delivers for this volume.
    normal / colour: the UNFILTERED mesh's attribute rows (the device's own arrays, or a reference's), None where the ring is configured without."""
    m = M.extract(vol, limit, bbox_min, bbox_max) if level == 0 else LOD.extract_lod(vol, limit, bbox_min, bbox_max, level)
    mesh = dict(unit=m["unit"], triangles=m["triangles"])
    if normal is not None:
        mesh["normal"] = normal
    if colour is not None:
        mesh["colour"] = colour
    kept, _, words = filter_mesh(mesh, min_triangles)
    return P.pack(kept["unit"], kept.get("normal"), kept.get("colour")), kept["triangles"], words
