"""The mesh components (tsdf_mesh_components / tsdf_mesh_keep_components, include/rgbd_recon_hip.h) restated in numpy: the definition, not the device's
algorithm.  Connectivity is by index: vertices are adjacent iff a triangle contains both; a component's representative is its smallest vertex index;
components are numbered by increasing representative; a vertex no triangle uses is a component of its own.  numpy only."""
import numpy as np

TABLE = np.dtype([("first_vertex", "<u4"), ("n_vertices", "<u4"), ("n_triangles", "<u4"), ("reserved", "<u4")])   # tsdf_mesh_component


def labels(triangles, n_vertices):
    """label[v] = the smallest vertex index of v's component.  Rounds of: flatten every parent chain, then hang every root an edge still separates from
    a smaller root under the smallest such root (parent[x] <= x throughout, so the root of a tree is its smallest index)."""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    parent = np.arange(n_vertices, dtype=np.int64)
    e0, e1 = np.concatenate([tri[:, 0], tri[:, 0]]), np.concatenate([tri[:, 1], tri[:, 2]])
    while True:
        while True:
            up = parent[parent]
            if (up == parent).all():
                break
            parent = up
        a, b = parent[e0], parent[e1]
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        apart = lo != hi
        if not apart.any():
            return parent.astype(np.uint32)
        np.minimum.at(parent, hi[apart], lo[apart])


def labels_sequential(triangles, n_vertices):
    """the same labels from a plain sequential union-find, the smaller root always on top"""
    parent = list(range(n_vertices))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for v0, v1, v2 in np.asarray(triangles, np.int64).reshape(-1, 3).tolist():
        for w in (v1, v2):
            a, b = find(v0), find(w)
            if a != b:
                parent[max(a, b)] = min(a, b)
    return np.array([find(v) for v in range(n_vertices)], np.uint32)


def from_labels(label, triangles):
    """(vertex_component [V] uint32, triangle_component [T] uint32, table [C] of TABLE) from the labels"""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    roots = np.flatnonzero(label == np.arange(len(label)))                # increasing: the numbering
    vertex_component = np.searchsorted(roots, label).astype(np.uint32)
    triangle_component = vertex_component[tri[:, 0]] if len(tri) else np.zeros(0, np.uint32)
    table = np.zeros(len(roots), TABLE)
    table["first_vertex"] = roots
    table["n_vertices"] = np.bincount(vertex_component, minlength=len(roots))
    table["n_triangles"] = np.bincount(triangle_component, minlength=len(roots))
    return vertex_component, triangle_component.astype(np.uint32), table


def components(triangles, n_vertices):
    return from_labels(labels(triangles, n_vertices), triangles)


def keep(mesh, keep_flags):
    """mesh (dict: position, triangles, and normal / colour where present) without the components whose flag is 0: kept vertices and triangles in their
    order, rows moved bit for bit, indices remapped to the number of kept vertices before them"""
    tri = np.asarray(mesh["triangles"], np.uint32).reshape(-1, 3)
    vc, tc, table = components(tri, len(mesh["position"]))
    flags = np.asarray(keep_flags).astype(bool)
    assert flags.shape == (len(table),)
    kv, kt = flags[vc], flags[tc]
    new_index = (np.cumsum(kv) - kv).astype(np.uint32)
    out = {k: np.ascontiguousarray(v[kv]) for k, v in mesh.items() if k in ("position", "unit", "normal", "colour")}
    out["triangles"] = np.ascontiguousarray(new_index[tri[kt]].reshape(-1, 3))
    return out


# ---- the test volumes (shape = res[::-1], limit 0.04)
LIMIT = 0.04


def speckle_volume(res=(20, 22, 19), seed=7, limit=LIMIT):
    """A: every voxel inside with probability 0.15: hundreds of small closed blobs"""
    shape = tuple(res[::-1])
    rng = np.random.default_rng(seed)
    inside = rng.random(shape) < 0.15
    pos = rng.uniform(0.001, limit, shape)
    neg = rng.uniform(-limit, -0.001, shape)
    return np.where(inside, pos, neg).astype(np.float32)


def random_volume(res=(20, 22, 19), seed=20221019, limit=LIMIT):
    """B: the random volume of tests/test_gpu_mesh.py, with its planted zeros, -0, NaN and +-inf"""
    rng = np.random.default_rng(seed)
    vol = rng.uniform(-limit, limit, res[::-1]).astype(np.float32)
    vol[rng.random(vol.shape) < 0.10] = 0.0
    special = np.array([-0.0, np.nan, np.inf, -np.inf], np.float32)
    pick = rng.random(vol.shape) < 0.02
    vol[pick] = special[rng.integers(0, 4, int(pick.sum()))]
    return vol


def snakes_volume(res=(40, 24, 24), limit=LIMIT):
    """C: two tubes that cross the 5 x 3 x 3 tiles back and forth: the smallest label has to travel the whole length"""
    vol = np.full(res[::-1], -limit, np.float32)
    ys = [3, 9, 15, 21]
    for z0 in (6, 17):
        for i, y in enumerate(ys):
            vol[z0 - 1:z0 + 2, y - 1:y + 2, 3:37] = limit
            if i + 1 < len(ys):
                xe = slice(34, 37) if i % 2 == 0 else slice(3, 6)
                vol[z0 - 1:z0 + 2, y - 1:ys[i + 1] + 2, xe] = limit
    return vol


def shells_volume(res=(40, 24, 24), limit=LIMIT):
    """D: a ball inside a hollow shell: three nested closed surfaces"""
    z, y, x = np.meshgrid(*[(np.arange(n) + 0.5) / n for n in res[::-1]], indexing="ij")
    r = np.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2)
    inside = (r < 0.12) | ((r > 0.25) & (r < 0.40))
    f = np.min(np.abs(r[..., None] - np.array([0.12, 0.25, 0.40])), axis=-1)
    return np.clip(np.where(inside, f, -f), -limit, limit).astype(np.float32)
