"""The mesh component measures (tsdf_mesh_component_measures / tsdf_mesh_filter_components_measured, include/rgbd_recon_hip.h) restated in numpy and
Python integers: the definition, not the device's algorithm.  Vertices are rounded to an isotropic grid of 2^20 units along the box's longest edge (three
float64 operations per coordinate); a triangle's doubled area is floor(sqrt(|e1 x e2|^2)) and its six-fold signed volume det(q0, q1, q2), both exact;
a component's row holds the bounds, the sums and the vertex sum.  Everything that could pass 64 bits is a Python integer."""
import math

import numpy as np

BITS = 20
QMAX = 1 << BITS
ROW = np.dtype([("q_min", "<u4", (3,)), ("q_max", "<u4", (3,)), ("area2", "<u8"), ("volume6_lo", "<u8"), ("volume6_hi", "<i8"), ("sum_q", "<u8", (3,)),
                ("reserved", "<u8")])                                                                  # tsdf_mesh_component_measure, 80 bytes
GRID = np.dtype([("unit", "<f8"), ("origin", "<f4", (3,)), ("bits", "<u4")])                           # tsdf_mesh_measure_grid, 24 bytes
RULE = np.dtype([("min_triangles", "<u4"), ("min_extent", "<u4"), ("min_area2", "<u8"), ("min_abs_volume6", "<u8"), ("flags", "<u4"), ("reserved", "<u4")])
RULE_POSITIVE_VOLUME = 1


def grid(bbox_min, bbox_max):
    """dict(scale, unit, origin [3] float32, bits): ext in fp32 as vol_to_world forms it, one float64 division"""
    lo, hi = np.asarray(bbox_min, np.float32), np.asarray(bbox_max, np.float32)
    ext = hi - lo
    assert ext.dtype == np.float32
    scale = 1048576.0 / float(ext.max())
    return dict(scale=scale, unit=1.0 / scale, origin=lo, bits=BITS)


def quantise(position, g):
    """[V, 3] int64 grid coordinates: rint((p - origin) * scale) in float64, half-way cases to even, clamped to [0, 2^20]; NaN gives 0"""
    p = np.asarray(position, np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint((p.astype(np.float64) - g["origin"].astype(np.float64)) * np.float64(g["scale"]))
    r = np.where(np.isnan(r), 0.0, r)
    return np.clip(r, 0.0, float(QMAX)).astype(np.int64)


def pack(q):
    """[V] uint64: qx | qy << 21 | qz << 42"""
    q = np.asarray(q).astype(np.uint64).reshape(-1, 3)
    return q[:, 0] | q[:, 1] << np.uint64(21) | q[:, 2] << np.uint64(42)


def unpack(words):
    w = np.asarray(words, np.uint64)
    return np.stack([w & np.uint64(0x1fffff), w >> np.uint64(21) & np.uint64(0x1fffff), w >> np.uint64(42) & np.uint64(0x1fffff)], axis=-1).astype(np.int64)


def _det3(a, b, c):
    return (a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2]) + a[2] * (b[0] * c[1] - b[1] * c[0]))


def triangle_measures(q, triangles):
    """(n2, a2, v6): three lists of Python integers, one entry per triangle"""
    rows = np.asarray(q, np.int64).reshape(-1, 3).tolist()
    n2, a2, v6 = [], [], []
    for i0, i1, i2 in np.asarray(triangles, np.int64).reshape(-1, 3).tolist():
        q0, q1, q2 = rows[i0], rows[i1], rows[i2]
        e1 = [q1[a] - q0[a] for a in range(3)]
        e2 = [q2[a] - q0[a] for a in range(3)]
        c = (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0])
        n = c[0] * c[0] + c[1] * c[1] + c[2] * c[2]
        n2.append(n)
        a2.append(math.isqrt(n))
        v6.append(_det3(q0, q1, q2))
    return n2, a2, v6


def measures(mesh, vertex_component, triangle_component, n_components, g):
    """[C] of ROW for the mesh (dict: position, triangles) labelled by vertex_component / triangle_component, on the grid g"""
    q = quantise(mesh["position"], g)
    vc, tc = np.asarray(vertex_component, np.int64), np.asarray(triangle_component, np.int64)
    _, a2, v6 = triangle_measures(q, mesh["triangles"])
    area, vol = [0] * n_components, [0] * n_components
    for c, a, v in zip(tc.tolist(), a2, v6):
        area[c] += a
        vol[c] += v
    rows = np.zeros(n_components, ROW)
    order = np.argsort(vc, kind="stable")
    bounds = np.searchsorted(vc[order], np.arange(n_components + 1))
    for c in range(n_components):
        mine = q[order[bounds[c]:bounds[c + 1]]]
        assert len(mine)                                                  # every component has a vertex
        rows["q_min"][c], rows["q_max"][c] = mine.min(axis=0), mine.max(axis=0)
        rows["sum_q"][c] = mine.sum(axis=0)                               # (V * 2^20 < 2^63)
        rows["area2"][c] = area[c]
        twos = vol[c] & ((1 << 128) - 1)
        rows["volume6_lo"][c] = twos & ((1 << 64) - 1)
        hi = twos >> 64
        rows["volume6_hi"][c] = hi - (1 << 64) if hi >= 1 << 63 else hi
    return rows


def volume6(rows):
    """the signed 128-bit sums as Python integers"""
    return [int(hi) * (1 << 64) + int(lo) for lo, hi in zip(rows["volume6_lo"].tolist(), rows["volume6_hi"].tolist())]


def keep_flags(rows, table, rule):
    """[C] bool: every clause of the rule (a RULE record or a dict of its fields) holds"""
    r = {k: int(rule[k]) for k in RULE.names}
    extent = (rows["q_max"].astype(np.int64) - rows["q_min"].astype(np.int64)).max(axis=1) if len(rows) else np.zeros(0, np.int64)
    vol = volume6(rows)
    return np.array([int(table["n_triangles"][c]) >= r["min_triangles"] and int(extent[c]) >= r["min_extent"] and int(rows["area2"][c]) >= r["min_area2"] and
                     abs(vol[c]) >= r["min_abs_volume6"] and (not (r["flags"] & RULE_POSITIVE_VOLUME) or vol[c] > 0) for c in range(len(rows))], bool)


def si(rows, g):
    """dict of float64 arrays in world units: area [C], volume [C], bounds_min / bounds_max [C, 3] (centroids need n_vertices: the table has it)"""
    u = float(g["unit"])
    origin = np.asarray(g["origin"], np.float64)
    return dict(area=rows["area2"].astype(np.float64) * u * u / 2.0, volume=np.array([v * u ** 3 / 6.0 for v in volume6(rows)], np.float64),
                bounds_min=origin + rows["q_min"] * u, bounds_max=origin + rows["q_max"] * u)


def random_small_volume(res=(4, 4, 4), seed=3, limit=0.04):
    """the 4 x 4 x 4 volume whose coarse lattice gives triangles with |e1 x e2|^2 >= 2^64: uniform in +-limit"""
    return np.random.default_rng(seed).uniform(-limit, limit, res[::-1]).astype(np.float32)
