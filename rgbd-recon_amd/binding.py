"""ctypes binding of librgbd_recon_hip.so (include/rgbd_recon_hip.h) and a Python mirror of the
reference operator surface, ``kinect::ReconIntegration``
(framework/reconstruction/recon_integration.hpp:35-103): same method names, same call order
(source/kinect_client.cpp:569-599,614), GL implicit state passed explicitly.

There is NO CPU fallback: if the HIP library is missing or no device is visible the constructor raises.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
LIB_PATH = os.environ.get("RGBDR_LIB", os.path.join(_PKG, "librgbd_recon_hip.so"))   # override: A/B builds of the kernels
HEADER_PATH = os.path.join(_ROOT, "include", "rgbd_recon_hip.h")

TSDF_MAX_STREAMS = 16


class TsdfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"tsdf error {code}: {msg}")
        self.code = code


class TsdfConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("bbox_min", C.c_float * 3), ("bbox_max", C.c_float * 3),
                ("voxel_size", C.c_float), ("res", C.c_uint32 * 3), ("brick_size", C.c_float * 3),
                ("limit", C.c_float), ("num_streams", C.c_uint32), ("depth_w", C.c_uint32), ("depth_h", C.c_uint32),
                ("color_w", C.c_uint32), ("color_h", C.c_uint32), ("view_w", C.c_uint32), ("view_h", C.c_uint32),
                ("device", C.c_int32), ("slab_z0", C.c_uint32), ("slab_z1", C.c_uint32), ("slab_recompute_halo", C.c_uint32),
                ("sparse_pool_tiles", C.c_uint32), ("proj_cache_mib", C.c_uint32), ("lane_flags", C.c_uint32), ("lane_priority", C.c_int32 * 4)]


LANES_ONE_STREAM, LANES_NO_INTEGRATE_LANE, LANES_NO_FILL_THREAD, LANES_SHARED_FILL_LANE = 1, 2, 4, 8   # tsdf_config::lane_flags


def build_library():
    """hipcc cross-compiles gfx950 without a GPU."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(_PKG, "csrc")])


def declared_symbols():
    """Every entry point include/rgbd_recon_hip.h declares."""
    text = open(HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(tsdf_[a-z0-9_]+)\s*\(", text)))


_lib = None


def load_library():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} is missing: run __graft_entry__.build() (there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        L.tsdf_last_error.restype = C.c_char_p
        L.tsdf_last_error.argtypes = [C.c_void_p]
        _lib = L
    return _lib


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


# ---------------------------------------------------------------------- calibration volume files (host only)
_TEXEL = {"cv_xyz": 3, "cv_uv": 2, "cv_xyz_inv": 4}


def read_calib_volume(path, kind):
    """Reads a *.cv_xyz / *.cv_uv / *.cv_xyz_inv file (calibration_volume.hpp:62-78) -> (array [rz][ry][rx][c], depth limits)."""
    L = load_library()
    L.tsdf_calib_last_error.restype = C.c_char_p
    c = _TEXEL[kind]
    res, lim = (C.c_uint32 * 3)(), (C.c_float * 2)()
    if L.tsdf_calib_volume_info(path.encode(), c, res, lim) != 0:
        raise TsdfError(-1, L.tsdf_calib_last_error().decode())
    out = np.empty((res[2], res[1], res[0], c), np.float32)
    if L.tsdf_calib_volume_read(path.encode(), c, _fp(out), C.c_uint64(out.size)) != 0:
        raise TsdfError(-1, L.tsdf_calib_last_error().decode())
    return out, (lim[0], lim[1])


def write_calib_volume(path, kind, volume, depth_limits):
    """Writes volume [rz][ry][rx][c] in the reference's on-disk format (calibration_volume.hpp:30-38)."""
    L = load_library()
    L.tsdf_calib_last_error.restype = C.c_char_p
    v = _f32(volume)
    assert v.ndim == 4 and v.shape[3] == _TEXEL[kind]
    res = (C.c_uint32 * 3)(v.shape[2], v.shape[1], v.shape[0])
    lim = (C.c_float * 2)(*[float(x) for x in depth_limits])
    if L.tsdf_calib_volume_write(path.encode(), _TEXEL[kind], res, lim, _fp(v)) != 0:
        raise TsdfError(-1, L.tsdf_calib_last_error().decode())


# ---------------------------------------------------------------------- draw() host matrices (recon_integration.cpp:66-72,182-205)
def view_matrices(mv, proj, view, bbox_min, bbox_max):
    """-> dict(vol_to_world [16], image_to_eye [16], normal_matrix [16], camera_pos [3]), column major; host only (no GPU)."""
    L = load_library()
    out = np.zeros(51, np.float32)
    rc = L.tsdf_view_matrices(_fp(_f32(mv).reshape(-1)), _fp(_f32(proj).reshape(-1)), C.c_uint32(int(view[0])), C.c_uint32(int(view[1])),
                              _fp(_f32(bbox_min)), _fp(_f32(bbox_max)), _fp(out))
    if rc != 0:
        raise TsdfError(rc, "singular modelview / projection matrix")
    return {"vol_to_world": out[:16].copy(), "image_to_eye": out[16:32].copy(), "normal_matrix": out[32:48].copy(), "camera_pos": out[48:].copy()}


# ---------------------------------------------------------------------- inverse calibration volumes (source/calib_inverter.cpp)
def frustum_from_volume(cv_xyz):
    """cv_xyz [rz][ry][rx][3] -> (planes [6][4], camera position): kinect::Frustum of the volume's corner texels (host only)."""
    L = load_library()
    L.tsdf_calib_last_error.restype = C.c_char_p
    v = _f32(cv_xyz)
    assert v.ndim == 4 and v.shape[3] == 3
    planes, cam = np.zeros((6, 4), np.float32), np.zeros(3, np.float32)
    if L.tsdf_frustum_from_volume(_fp(v), (C.c_uint32 * 3)(v.shape[2], v.shape[1], v.shape[0]), _fp(planes), _fp(cam)) != 0:
        raise TsdfError(-1, L.tsdf_calib_last_error().decode())
    return planes, cam


def inverse_volume_resolution(bbox_min, bbox_max, voxel_size=0.007):
    L = load_library()
    res = (C.c_uint32 * 3)()
    if L.tsdf_inverse_volume_resolution(_fp(_f32(bbox_min)), _fp(_f32(bbox_max)), C.c_float(voxel_size), res) != 0:
        raise TsdfError(-1, "bad argument")
    return tuple(res)


def invert_calibration(cv_xyz, bbox_min, bbox_max, res_inv, device=0):
    """CalibrationInverter::calculateInverseVolumes for one sensor on the GPU -> ([rz][ry][rx][4], device milliseconds)."""
    L = load_library()
    L.tsdf_calib_last_error.restype = C.c_char_p
    v = _f32(cv_xyz)
    assert v.ndim == 4 and v.shape[3] == 3
    out = np.empty((int(res_inv[2]), int(res_inv[1]), int(res_inv[0]), 4), np.float32)
    ms = C.c_float()
    rc = L.tsdf_invert_calibration(int(device), _fp(v), (C.c_uint32 * 3)(v.shape[2], v.shape[1], v.shape[0]), _fp(_f32(bbox_min)), _fp(_f32(bbox_max)),
                                   (C.c_uint32 * 3)(*[int(x) for x in res_inv]), _fp(out), C.byref(ms))
    if rc != 0:
        raise TsdfError(rc, L.tsdf_calib_last_error().decode())
    return out, ms.value


def stream_num_frames(path, record_bytes):
    """FileBuffer::calcNumFrames for recordings/<sensor>.stream."""
    L = load_library()
    L.tsdf_calib_last_error.restype = C.c_char_p
    n = C.c_uint64()
    if L.tsdf_stream_num_frames(path.encode(), C.c_uint64(record_bytes), C.byref(n)) != 0:
        raise TsdfError(-1, L.tsdf_calib_last_error().decode())
    return n.value


def read_stream_record(path, record_bytes, frame):
    """Record `frame` ([colour][depth]) of one sensor's .stream file (NetKinectArray::readFromFiles)."""
    L = load_library()
    L.tsdf_calib_last_error.restype = C.c_char_p
    out = np.empty(record_bytes, np.uint8)
    if L.tsdf_stream_read_record(path.encode(), C.c_uint64(record_bytes), C.c_uint64(frame), out.ctypes.data_as(C.c_void_p)) != 0:
        raise TsdfError(-1, L.tsdf_calib_last_error().decode())
    return out


COLOR_RGB8, COLOR_DXT1, COLOR_DXT5 = 0, 1, 5
DEPTH_F32, DEPTH_U8 = 0, 1
PRESENT_RGBA8, PRESENT_DXT1 = 0, 1    # tsdf_present_config: format
PRESENT_TOP_DOWN = 1                  # ... flags
MESH_NORMALS, MESH_COLOURS = 1, 2     # tsdf_mesh_extract: flags
MESH_OVERFLOW_VERTICES, MESH_OVERFLOW_TRIANGLES, MESH_OVERFLOW_TILES = 1, 2, 4   # tsdf_mesh_frame: overflow bits
# tsdf_mesh_component as a numpy dtype: what mesh_download_components returns as its table
MESH_COMPONENT_DTYPE = np.dtype([("first_vertex", "<u4"), ("n_vertices", "<u4"), ("n_triangles", "<u4"), ("reserved", "<u4")])
# tsdf_mesh_component_measure (80 bytes), tsdf_mesh_measure_grid (24) and tsdf_mesh_measure_rule (32) as numpy dtypes
MESH_COMPONENT_MEASURE_DTYPE = np.dtype([("q_min", "<u4", (3,)), ("q_max", "<u4", (3,)), ("area2", "<u8"), ("volume6_lo", "<u8"), ("volume6_hi", "<i8"),
                                         ("sum_q", "<u8", (3,)), ("reserved", "<u8")])
MESH_MEASURE_GRID_DTYPE = np.dtype([("unit", "<f8"), ("origin", "<f4", (3,)), ("bits", "<u4")])
MESH_MEASURE_RULE_DTYPE = np.dtype([("min_triangles", "<u4"), ("min_extent", "<u4"), ("min_area2", "<u8"), ("min_abs_volume6", "<u8"), ("flags", "<u4"),
                                    ("reserved", "<u4")])
MESH_RULE_POSITIVE_VOLUME = 1


def mesh_volume6(rows):
    """the components' six-fold signed volumes in unit^3 as Python integers (volume6_hi * 2^64 + volume6_lo)"""
    return [int(hi) * (1 << 64) + int(lo) for lo, hi in zip(rows["volume6_lo"].tolist(), rows["volume6_hi"].tolist())]


def mesh_measure_rule_for(unit, min_triangles=0, min_extent_m=0.0, min_area_m2=0.0, min_volume_m3=0.0, positive_volume=False):
    """A keep rule for tsdf_mesh_filter_components_measured (one MESH_MEASURE_RULE_DTYPE record) on a grid of `unit` metres: metres converted to grid
    integers with a ceiling -- min_extent = ceil(m / unit), min_area2 = ceil(2 m2 / unit^2), min_abs_volume6 = ceil(6 m3 / unit^3) -- so a component
    that passes is at least that large.  ValueError for a negative or NaN threshold and for one the rule's field cannot hold (with a unit of 2.1 um:
    an extent above 9 km, a volume above 28 m^3)."""
    u = float(unit)
    rule = np.zeros((), MESH_MEASURE_RULE_DTYPE)
    for field, name, value in (("min_triangles", "min_triangles", float(min_triangles)), ("min_extent", "min_extent_m", float(min_extent_m) / u),
                               ("min_area2", "min_area_m2", 2.0 * float(min_area_m2) / (u * u)), ("min_abs_volume6", "min_volume_m3", 6.0 * float(min_volume_m3) / (u * u * u))):
        top = int(np.iinfo(MESH_MEASURE_RULE_DTYPE[field]).max)
        if not 0.0 <= value <= float(top):                                # (NaN too)
            raise ValueError(f"{name} gives {value:g} grid units: outside 0 .. {top}, what the rule's {field} holds")
        rule[field] = min(int(math.ceil(value)), top)
    rule["flags"] = MESH_RULE_POSITIVE_VOLUME if positive_volume else 0
    return rule


def mesh_measures_si(rows, grid, table=None):
    """The measure rows in world units, float64: dict(area [C] = area2 * unit^2 / 2, volume [C] = volume6 * unit^3 / 6 (signed: a closed void is
    negative), bounds_min / bounds_max [C, 3] = origin + q * unit, centroid [C, 3] = origin + sum_q / n_vertices * unit -- the vertex centroid, with the
    components' table (mesh_download_components()["table"]); without it the entry is absent).  grid: what mesh_component_measures() returned."""
    u = float(grid["unit"])
    origin = np.asarray(grid["origin"], np.float64)
    out = dict(area=rows["area2"].astype(np.float64) * (u * u / 2.0), volume=np.array([v * (u ** 3 / 6.0) for v in mesh_volume6(rows)], np.float64),
               bounds_min=origin + rows["q_min"].astype(np.float64) * u, bounds_max=origin + rows["q_max"].astype(np.float64) * u)
    if table is not None:
        out["centroid"] = origin + rows["sum_q"].astype(np.float64) / np.maximum(table["n_vertices"], 1)[:, None].astype(np.float64) * u
    return out


class MeshFrame(C.Structure):
    """tsdf_mesh_frame of rgbd_recon_hip.h"""
    _fields_ = [("vertices", C.c_void_p), ("triangles", C.POINTER(C.c_uint32)), ("n_vertices", C.c_uint64), ("n_triangles", C.c_uint64),
                ("needed_vertices", C.c_uint64), ("needed_triangles", C.c_uint64), ("needed_tiles", C.c_uint64), ("tag", C.c_uint64),
                ("flags", C.c_uint32), ("vertex_stride", C.c_uint32), ("overflow", C.c_uint32), ("res", C.c_uint32 * 3),
                ("bbox_min", C.c_float * 3), ("bbox_max", C.c_float * 3)]


MESH_INDEX_U32, MESH_INDEX_TILE16 = 0, 1   # tsdf_mesh_stream_config_compact: index_format
MESH_TILE_ROW_DTYPE = np.dtype([("tile", "<u4"), ("first_vertex", "<u4"), ("first_triangle", "<u4"), ("n_triangles", "<u4")])   # tsdf_mesh_tile_row


class MeshCompact(C.Structure):
    """tsdf_mesh_compact of rgbd_recon_hip.h"""
    _fields_ = [("table", C.c_void_p), ("triangles", C.POINTER(C.c_uint16)), ("n_tile_rows", C.c_uint64), ("tiles", C.c_uint32 * 3), ("level", C.c_uint32)]


def unpack_mesh_triangles(table, codes, tiles):
    """the header's decoding rule of the tile-local format: table (MESH_TILE_ROW_DTYPE [R]), codes (uint16 [T][3]), tiles (the level's lattice-tile
    grid) -> uint32 [T][3], byte for byte the uint32 triangle array of the same frame"""
    codes = np.asarray(codes, np.uint16).reshape(-1, 3).astype(np.int64)
    if not len(codes):
        return np.zeros((0, 3), np.uint32)
    row = np.repeat(np.arange(len(table)), table["n_triangles"].astype(np.int64))          # the row of every triangle: rows own consecutive ranges
    owner = (table["tile"].astype(np.int64)[row][:, None] + ((codes >> 12) & 1) + ((codes >> 13) & 1) * int(tiles[0])
             + ((codes >> 14) & 1) * int(tiles[0]) * int(tiles[1]))
    owner_row = np.searchsorted(table["tile"], owner.ravel(), side="right").reshape(owner.shape) - 1   # the last row whose tile is <= owner
    return (table["first_vertex"].astype(np.int64)[owner_row] + (codes & 0xfff)).astype(np.uint32)


class MeshPart(C.Structure):
    """tsdf_mesh_part of rgbd_recon_hip.h"""
    _fields_ = [("layers", C.c_uint32 * 2), ("level", C.c_uint32), ("top", C.c_uint32), ("seam_tiles", C.c_uint32), ("reserved", C.c_uint32 * 3)]


def join_mesh_parts(parts):
    """the header's join rule ("mesh streaming: slab parts"): parts = the (vertices, codes, info) frames of part rings (mesh_stream_config(part=True)) of
    contiguous slabs, in slab order -> (vertices, codes, info) of the whole-volume compact frame: the vertices and codes concatenated, the rows
    concatenated with the vertices and triangles of the parts below added to first_vertex and first_triangle.  ValueError when a part overflowed (the
    frame is dropped whole), when the parts are not contiguous or differ in level or vertex stride."""
    parts = list(parts)
    if not parts:
        raise ValueError("no part")
    first = parts[0][2]
    rows, nv, nt = [], 0, 0
    for k, (vertices, codes, info) in enumerate(parts):
        if info["overflow"]:
            raise ValueError(f"part {k} overflowed (bits {info['overflow']}): the frame is dropped whole")
        if info["vertex_stride"] != first["vertex_stride"] or info["compact"]["level"] != first["compact"]["level"] or info["compact"]["tiles"] != first["compact"]["tiles"]:
            raise ValueError(f"part {k} has another vertex stride, level or tile grid")
        if k and info["part"]["layers"][0] != parts[k - 1][2]["part"]["layers"][1]:
            raise ValueError(f"part {k} does not follow part {k - 1}: layers {parts[k - 1][2]['part']['layers']} then {info['part']['layers']}")
        t = np.array(info["compact"]["table"], MESH_TILE_ROW_DTYPE)
        t["first_vertex"] += np.uint32(nv)
        t["first_triangle"] += np.uint32(nt)
        rows.append(t)
        nv += len(vertices)
        nt += len(codes)
    info = dict(first, n_vertices=nv, n_triangles=nt, needed_vertices=nv, needed_triangles=nt, needed_tiles=sum(len(r) for r in rows), overflow=0,
                compact=dict(first["compact"], table=np.concatenate(rows)),
                part=dict(layers=(first["part"]["layers"][0], parts[-1][2]["part"]["layers"][1]), level=first["part"]["level"], top=parts[-1][2]["part"]["top"], seam_tiles=parts[-1][2]["part"]["seam_tiles"]))
    info.pop("taps", None)
    if all("taps" in p[2] for p in parts):                               # ("texture taps in the frame": the parts' blocks join by concatenation, like the vertices)
        info["taps"] = np.concatenate([np.ascontiguousarray(p[2]["taps"], PACKED_TAP_DTYPE).view(np.uint64) for p in parts]).view(PACKED_TAP_DTYPE)   # ([V_k][N] each, joined as 8-byte words; a part without a vertex adds nothing)
    return np.concatenate([p[0] for p in parts]), np.concatenate([np.asarray(p[1], np.uint16).reshape(-1, 3) for p in parts]), info


def unpack_mesh_vertices(vertices):
    """a streamed frame's vertex array -> dict(position uint16 [V][3], and for the 16-byte stride normal int16 [V][2], colour uint8 [V][4])"""
    if vertices.dtype == np.uint16:
        return dict(position=vertices[:, :3])
    v = np.ascontiguousarray(vertices)
    return dict(position=v[:, :8].view(np.uint16)[:, :3], normal=v[:, 8:12].view(np.int16), colour=v[:, 12:16])


# ---------------------------------------------------------------------- mesh components on Z-slab contexts: the lists, the merge, the joined mesh
MESH_SEAM_VERTEX_DTYPE = np.dtype([("vertex", "<u4"), ("root", "<u4")])                                                # tsdf_mesh_seam_vertex
MESH_SEAM_ROOT_DTYPE = np.dtype([("root", "<u4"), ("rank", "<u4"), ("n_vertices", "<u4"), ("n_triangles", "<u4")])    # tsdf_mesh_seam_root
MESH_COMPONENT_LINK_DTYPE = np.dtype([("root", "<u4"), ("final_root", "<u4"), ("component", "<u4"), ("reserved0", "<u4"),
                                      ("n_vertices", "<u4"), ("n_triangles", "<u4"), ("reserved1", "<u4"), ("reserved2", "<u4")])   # tsdf_mesh_component_link


class MeshComponentSeams(C.Structure):
    """tsdf_mesh_component_seams of rgbd_recon_hip.h"""
    _fields_ = [("vertex_base", C.c_uint64), ("n_vertices", C.c_uint64), ("n_local", C.c_uint64), ("n_down", C.c_uint64), ("n_up", C.c_uint64),
                ("n_roots", C.c_uint64), ("down", C.c_void_p), ("up", C.c_void_p), ("roots", C.c_void_p)]


def _component_seam_lists(slabs):
    """the merge's input with every list as a contiguous array of its dtype"""
    return [dict(vertex_base=int(s["vertex_base"]), n_vertices=int(s["n_vertices"]), n_local=int(s["n_local"]),
                 down=np.ascontiguousarray(s["down"], MESH_SEAM_VERTEX_DTYPE).reshape(-1), up=np.ascontiguousarray(s["up"], MESH_SEAM_VERTEX_DTYPE).reshape(-1),
                 roots=np.ascontiguousarray(s["roots"], MESH_SEAM_ROOT_DTYPE).reshape(-1)) for s in slabs]


def component_seams_struct(slabs):
    """(the tsdf_mesh_component_seams array of `slabs`, the arrays it points into -- keep them alive as long as the array)"""
    lists = _component_seam_lists(slabs)
    arr = (MeshComponentSeams * max(len(lists), 1))()
    for a, s in zip(arr, lists):
        a.vertex_base, a.n_vertices, a.n_local = s["vertex_base"], s["n_vertices"], s["n_local"]
        a.n_down, a.n_up, a.n_roots = len(s["down"]), len(s["up"]), len(s["roots"])
        a.down, a.up, a.roots = s["down"].ctypes.data, s["up"].ctypes.data, s["roots"].ctypes.data
    return arr, lists


def merge_mesh_component_seams(slabs, native=False):
    """The host merge of the slabs' seam lists (tsdf_mesh_merge_component_seams; csrc/mesh_cc_seams.hpp): slabs = per slab, in slab order,
    dict(vertex_base, n_vertices, n_local, down, up, roots) with the lists of mesh_slab_component_seam().  Returns dict(component_base=[per slab],
    links=[MESH_COMPONENT_LINK_DTYPE array per slab, one record per root record], n_components).  native=False: the numpy twin, ValueError for lists
    the library refuses; native=True: the library's function through ctypes (it needs no device), TsdfError with code -1.  Identical bytes."""
    lists = _component_seam_lists(slabs)
    n_roots = [len(s["roots"]) for s in lists]
    first = np.concatenate([[0], np.cumsum(n_roots)]).astype(np.int64)
    split = lambda links: [links[first[k]:first[k + 1]] for k in range(len(lists))]
    if native:
        arr, keep = component_seams_struct(lists)
        base, links, n = np.zeros(max(len(lists), 1), np.uint64), np.zeros(int(first[-1]), MESH_COMPONENT_LINK_DTYPE), C.c_uint64()
        rc = load_library().tsdf_mesh_merge_component_seams(arr, C.c_uint32(len(lists)), base.ctypes.data_as(C.c_void_p), links.ctypes.data_as(C.c_void_p), C.byref(n))
        if rc:
            raise TsdfError(rc, "tsdf_mesh_merge_component_seams refused the lists")
        return dict(component_base=[int(b) for b in base[:len(lists)]], links=split(links), n_components=int(n.value))
    for k, s in enumerate(lists):
        v0, v1 = s["vertex_base"], s["vertex_base"] + s["n_vertices"]
        if v1 > 1 << 32 or s["n_local"] > s["n_vertices"] or (k and v0 < lists[k - 1]["vertex_base"] + lists[k - 1]["n_vertices"]):
            raise ValueError(f"slab {k}: out of order, or past the 32-bit indices")
        r, d, u = s["roots"], s["down"], s["up"]
        ascending = lambda a: len(a) < 2 or bool((np.diff(a.astype(np.int64)) > 0).all())
        if not (ascending(r["root"]) and ascending(r["rank"]) and ascending(d["vertex"]) and ascending(u["vertex"])):
            raise ValueError(f"slab {k}: a list is not strictly ascending")
        if ((r["root"] < v0) | (r["root"] >= v1) | (r["rank"] >= s["n_local"])).any() or not (np.isin(d["root"], r["root"]).all() and np.isin(u["root"], r["root"]).all()):
            raise ValueError(f"slab {k}: a root outside its slab")
        if ((d["vertex"] < v0) | (d["vertex"] >= v1) | (d["root"] > d["vertex"])).any() or (u["vertex"] < v1).any():
            raise ValueError(f"slab {k}: a seam record's vertex on the wrong side of the seam")
        if len(u) and (k + 1 == len(lists) or not np.isin(u["vertex"], lists[k + 1]["down"]["vertex"]).all()):
            raise ValueError(f"slab {k}: an up record without its down record")
    # the union-find over all root records: node ids ascend with the roots, the smaller on top
    parent = list(range(int(first[-1])))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for k in range(len(lists) - 1):
        s, a = lists[k], lists[k + 1]
        if not len(s["up"]):
            continue
        below = first[k] + np.searchsorted(s["roots"]["root"], s["up"]["root"])
        above_root = a["down"]["root"][np.searchsorted(a["down"]["vertex"], s["up"]["vertex"])]
        above = first[k + 1] + np.searchsorted(a["roots"]["root"], above_root)
        for x, y in zip(below.tolist(), above.tolist()):
            x, y = find(x), find(y)
            if x != y:
                parent[max(x, y)] = min(x, y)
    top = np.array([find(x) for x in range(len(parent))], np.int64)
    records = np.concatenate([s["roots"] for s in lists]) if lists else np.zeros(0, MESH_SEAM_ROOT_DTYPE)
    nv, nt = np.zeros(len(parent), np.int64), np.zeros(len(parent), np.int64)
    np.add.at(nv, top, records["n_vertices"].astype(np.int64))
    np.add.at(nt, top, records["n_triangles"].astype(np.int64))
    if len(parent) and (nv.max() > 0xffffffff or nt.max() > 0xffffffff):
        raise ValueError("a component's totals leave 32 bits")
    base, number = [0], np.zeros(len(parent), np.int64)
    for k, s in enumerate(lists):
        nodes = np.arange(first[k], first[k + 1])
        removed = top[nodes] != nodes
        number[nodes] = base[k] + s["roots"]["rank"].astype(np.int64) - np.cumsum(removed)   # (read at surviving roots only)
        base.append(base[k] + s["n_local"] - int(removed.sum()))
    links = np.zeros(len(parent), MESH_COMPONENT_LINK_DTYPE)
    links["root"], links["final_root"], links["component"] = records["root"], records["root"][top], number[top]
    links["n_vertices"], links["n_triangles"] = nv[top], nt[top]
    return dict(component_base=base[:-1], links=split(links), n_components=base[-1])


def drop_mesh_components(mesh, vertex_component, triangle_component, keep):
    """The joined mesh without the components c with keep[c] == 0, by tsdf_mesh_keep_components' rule: kept vertices and triangles in their order, rows
    moved bit for bit, a vertex's new index the number of kept vertices before it.  mesh: dict(position, triangles, and normal / colour where present);
    vertex_component / triangle_component: the joined arrays of the slabs' mesh_slab_download_components()."""
    flags = np.asarray(keep) != 0
    kv, kt = flags[np.asarray(vertex_component, np.int64)], flags[np.asarray(triangle_component, np.int64)]
    new_index = (np.cumsum(kv) - kv).astype(np.uint32)
    out = {k: np.ascontiguousarray(v[kv]) for k, v in mesh.items() if k in ("position", "normal", "colour")}
    out["triangles"] = np.ascontiguousarray(new_index[np.asarray(mesh["triangles"], np.uint32).reshape(-1, 3)[kt]].reshape(-1, 3))
    return out


RAYS_UNIT_CUBE, RAY_NORMALS, RAY_COLOURS = 1, 2, 4   # tsdf_cast_rays: flags
RAY_HIT, RAY_OUTSIDE, RAY_INVALID = 1, 2, 4         # tsdf_ray_hit: status bits


class Ray(C.Structure):
    """tsdf_ray of rgbd_recon_hip.h"""
    _fields_ = [("origin", C.c_float * 3), ("t_min", C.c_float), ("dir", C.c_float * 3), ("t_max", C.c_float)]


class RayHit(C.Structure):
    """tsdf_ray_hit of rgbd_recon_hip.h"""
    _fields_ = [("pos", C.c_float * 3), ("t", C.c_float), ("n_samples", C.c_uint32), ("status", C.c_uint32), ("pad", C.c_uint32 * 2)]


class RaySurface(C.Structure):
    """tsdf_ray_surface of rgbd_recon_hip.h"""
    _fields_ = [("normal", C.c_float * 3), ("pad", C.c_float), ("rgba", C.c_float * 4)]


# the same three records as numpy dtypes: what cast_rays / view_rays take and return
RAY_DTYPE = np.dtype([("origin", np.float32, 3), ("t_min", np.float32), ("dir", np.float32, 3), ("t_max", np.float32)])
RAY_HIT_DTYPE = np.dtype([("pos", np.float32, 3), ("t", np.float32), ("n_samples", np.uint32), ("status", np.uint32), ("pad", np.uint32, 2)])
RAY_SURFACE_DTYPE = np.dtype([("normal", np.float32, 3), ("pad", np.float32), ("rgba", np.float32, 4)])


def as_rays(rays):
    """RAY_DTYPE records from records or from floats [n][8] = origin, t_min, dir, t_max"""
    rays = np.asarray(rays)
    if rays.dtype != RAY_DTYPE:
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8).view(RAY_DTYPE).reshape(-1)
    return np.ascontiguousarray(rays)


def merge_ray_parts(parts):
    """The merge rule of the header's "ray queries: slab parts" in numpy, for a receiver without a GPU.  parts: per contiguous slab, in slab order, what
    cast_rays_part returned -- hits, or (hits, surface).  Per ray the part with RAY_HIT and the smallest n_samples wins (no two tie: a sample has one
    owner), part 0 when none hit; the surface record travels with the winner.  -> hits, or (hits, surface): what cast_rays gives on the whole volume."""
    parts = list(parts)
    if not parts:
        raise ValueError("no part to merge")
    with_surface = isinstance(parts[0], tuple)
    hits = np.stack([np.ascontiguousarray(p[0] if with_surface else p, RAY_HIT_DTYPE) for p in parts])
    key = np.where((hits["status"] & RAY_HIT) != 0, hits["n_samples"].astype(np.int64), np.int64(1) << 40)
    win = np.argmin(key, axis=0)                                         # (the first minimum: part 0 where no part hit)
    at = np.arange(hits.shape[1])
    merged = hits[win, at]
    if not with_surface:
        return merged
    surface = np.stack([np.ascontiguousarray(p[1], RAY_SURFACE_DTYPE) for p in parts])
    return merged, surface[win, at]


def make_rays(origin, direction, t_min=0.0, t_max=np.inf):
    """RAY_DTYPE records from origins [n][3] and directions [n][3] (t_min / t_max scalars or [n])"""
    origin = np.asarray(origin, np.float32).reshape(-1, 3)
    rays = np.zeros(len(origin), RAY_DTYPE)
    rays["origin"], rays["dir"] = origin, np.asarray(direction, np.float32).reshape(-1, 3)
    rays["t_min"], rays["t_max"] = t_min, t_max
    return rays


TAPS_UNIT_CUBE, TAPS_SENSOR = 1, 2   # tsdf_texture_taps: flags


class TextureTap(C.Structure):
    """tsdf_texture_tap of rgbd_recon_hip.h"""
    _fields_ = [("u", C.c_float), ("v", C.c_float), ("quality", C.c_float), ("dist", C.c_float)]


class SensorTap(C.Structure):
    """tsdf_sensor_tap of rgbd_recon_hip.h"""
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("depth", C.c_float)]


# the same two records as numpy dtypes: what texture_taps / mesh_texture_taps return, [points][streams]
TEXTURE_TAP_DTYPE = np.dtype([("u", np.float32), ("v", np.float32), ("quality", np.float32), ("dist", np.float32)])
SENSOR_TAP_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("z", np.float32), ("depth", np.float32)])


MESH_STREAM_TAPS = 1   # tsdf_mesh_stream_config_taps: tap_flags


class PackedTap(C.Structure):
    """tsdf_packed_tap of rgbd_recon_hip.h"""
    _fields_ = [("u", C.c_uint16), ("v", C.c_uint16), ("quality_h", C.c_uint16), ("dist_h", C.c_uint16)]


class MeshTaps(C.Structure):
    """tsdf_mesh_taps of rgbd_recon_hip.h"""
    _fields_ = [("taps", C.c_void_p), ("n_vertices", C.c_uint64), ("n_streams", C.c_uint32), ("tap_bytes", C.c_uint32)]


PACKED_TAP_DTYPE = np.dtype([("u", "<u2"), ("v", "<u2"), ("quality_h", "<u2"), ("dist_h", "<u2")])   # a streamed frame's tap block, [vertices][streams]


def unpack_mesh_taps(packed):
    """the receiver's unpacking of a streamed frame's tap block (the header's "mesh streaming: texture taps in the frame"): PACKED_TAP_DTYPE [V][N] ->
    TEXTURE_TAP_DTYPE [V][N] in float32, u = code / 65535.0f and the binary16 weights widened; blend_from_taps takes the result as it is"""
    packed = np.asarray(packed)
    assert packed.dtype == PACKED_TAP_DTYPE
    out = np.zeros(packed.shape, TEXTURE_TAP_DTYPE)
    out["u"] = packed["u"].astype(np.float32) / np.float32(65535.0)
    out["v"] = packed["v"].astype(np.float32) / np.float32(65535.0)
    out["quality"] = np.ascontiguousarray(packed["quality_h"]).view(np.float16).astype(np.float32)
    out["dist"] = np.ascontiguousarray(packed["dist_h"]).view(np.float16).astype(np.float32)
    return out


def _axis_linear(u, n):
    """LINEAR + CLAMP_TO_EDGE along one axis in float32: f = u * n - 0.5, texels clamp(floor(f)), clamp(floor(f) + 1), weight f - floor(f)"""
    f32 = np.float32
    f = (u * f32(n) - f32(0.5)).astype(f32)
    fl = np.floor(f)
    a = (f - fl).astype(f32)
    hi = f32(n - 1)
    i0 = np.where(np.isnan(fl), f32(0), np.clip(fl, f32(0), hi)).astype(np.int64)
    i1 = np.where(np.isnan(fl), f32(0), np.clip((fl + f32(1)).astype(f32), f32(0), hi)).astype(np.int64)
    return i0, i1, a


def blend_from_taps(taps, colour_rgb8):
    """The receiver's rule of the header's texture tap section in float32 numpy: taps TEXTURE_TAP_DTYPE [n][N], colour_rgb8 uint8 [N][Hc][Wc][3] (the
    frame's colour images) -> rgba float32 [n][4], alpha +1 (weighted by quality) / -1 (fallback).  Fed the taps of a unit-cube point it gives the bits of
    blendColors there: the ray surface's rgba, the mesh colour."""
    f32 = np.float32
    taps = np.asarray(taps)
    assert taps.dtype == TEXTURE_TAP_DTYPE and taps.ndim == 2
    img = np.asarray(colour_rgb8, np.uint8)
    n, N = taps.shape
    assert img.ndim == 4 and img.shape[0] == N and img.shape[3] == 3
    ch, cw = img.shape[1], img.shape[2]
    lerp = lambda a, b, t: (a + ((b - a).astype(f32) * t).astype(f32)).astype(f32)
    tc, tc2 = np.zeros((n, 3), f32), np.zeros((n, 3), f32)
    tw, tw2 = np.zeros(n, f32), np.zeros(n, f32)
    with np.errstate(all="ignore"):
        for i in range(N):
            x0, x1, ax = _axis_linear(taps["u"][:, i], cw)
            y0, y1, ay = _axis_linear(taps["v"][:, i], ch)
            tex = lambda y, x: (img[i][y, x].astype(f32) / f32(255.0)).astype(f32)
            ax3, ay3 = ax[:, None], ay[:, None]
            col = lerp(lerp(tex(y0, x0), tex(y0, x1), ax3), lerp(tex(y1, x0), tex(y1, x1), ax3), ay3)
            q, dist = taps["quality"][:, i].astype(f32), taps["dist"][:, i].astype(f32)
            de = (dist + f32(0.01)).astype(f32)
            tc = (tc + ((col * q[:, None]).astype(f32) / de[:, None]).astype(f32)).astype(f32)
            tw = (tw + (q / de).astype(f32)).astype(f32)
            tc2 = (tc2 + (col / dist[:, None]).astype(f32)).astype(f32)
            tw2 = (tw2 + (f32(1.0) / dist).astype(f32)).astype(f32)
        valid = tw > 0
        out = np.zeros((n, 4), f32)
        out[:, :3] = np.where(valid[:, None], tc / tw[:, None], tc2 / tw2[:, None])
        out[:, 3] = np.where(valid, f32(1.0), f32(-1.0))
    return out


K1_FORMS = ("generic", "lds_direct", "lds_separable", "record", "cached")   # TSDF_K1_* of rgbd_recon_hip.h


class ReconIntegrationHip:
    """HIP drop-in for kinect::ReconIntegration.  `scene` supplies what CalibrationFiles / CalibVolumes /
    NetKinectArray hold in the reference (rgbd-recon_amd/scene.py layout)."""

    def __init__(self, scene, res=None, voxel_size=0.01, brick_size=0.1, limit=0.01, view=(1280, 720),
                 device=0, slab=(0, 0), upload=True, recompute_halo=False, sparse_pool_tiles=0, proj_cache_mib=0, lane_flags=0, lane_priority=(0, 0, 0, 0)):
        self._L = load_library()
        self._c = None
        cfg = TsdfConfig()
        cfg.struct_size = C.sizeof(TsdfConfig)
        cfg.bbox_min[:] = [float(x) for x in scene["bbox_min"]]
        cfg.bbox_max[:] = [float(x) for x in scene["bbox_max"]]
        cfg.voxel_size = voxel_size
        cfg.res[:] = list(res) if res is not None else [0, 0, 0]
        cfg.brick_size[:] = [brick_size] * 3 if np.isscalar(brick_size) else list(brick_size)
        cfg.limit = limit
        cfg.num_streams = scene["n"]
        cfg.depth_w, cfg.depth_h = scene["width"], scene["height"]
        cfg.color_w, cfg.color_h = scene["color_width"], scene["color_height"]
        cfg.view_w, cfg.view_h = view
        cfg.device = device
        cfg.slab_z0, cfg.slab_z1 = slab
        cfg.slab_recompute_halo = int(bool(recompute_halo))
        cfg.sparse_pool_tiles = int(sparse_pool_tiles)
        cfg.proj_cache_mib = int(proj_cache_mib or 0)   # opt-in projection cache of the integrate kernel, MiB (0 / None: off)
        cfg.lane_flags = int(lane_flags)
        cfg.lane_priority[:] = [int(x) for x in lane_priority]
        ctx = C.c_void_p()
        rc = self._L.tsdf_create(C.byref(cfg), C.byref(ctx))
        if rc != 0:
            raise TsdfError(rc, self._L.tsdf_last_error(None).decode())
        self._c = ctx
        self.view = tuple(view)
        self._bbox = (np.array([float(x) for x in scene["bbox_min"]], np.float32), np.array([float(x) for x in scene["bbox_max"]], np.float32))
        self.n = scene["n"]
        self._dims = (scene["height"], scene["width"], scene["color_height"], scene["color_width"])
        r3, b3, s3 = (C.c_uint32 * 3)(), (C.c_uint32 * 3)(), (C.c_float * 3)()
        self._ck(self._L.tsdf_get_resolution(self._c, r3, b3, s3))
        self.res, self.res_bricks, self.brick_size = tuple(r3), tuple(b3), tuple(s3)
        n = C.c_uint32()
        self._ck(self._L.tsdf_num_lods(self._c, C.byref(n)))
        self.num_lods = n.value
        if upload:
            self.set_calibration(scene)
            self.upload_frame(scene)

    # ------------------------------------------------------------------ plumbing
    def _ck(self, rc):
        if rc != 0:
            raise TsdfError(rc, self._L.tsdf_last_error(self._c).decode())

    def close(self):
        if self._c:
            self._L.tsdf_destroy(self._c)
            self._c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream_ptr):
        """Adopt a caller-owned HIP stream.  None: back to the context's own stream.  0 is the handle of the process's NULL
        ("legacy default") stream -- what torch.cuda.default_stream().cuda_stream returns -- and is adopted as such
        (tsdf_adopt_null_stream); passed to tsdf_set_stream it would mean "back to own" and leave the context's kernels
        unordered against torch ops and RCCL collectives on the default stream."""
        if hip_stream_ptr is None:
            self._ck(self._L.tsdf_set_stream(self._c, None))
        elif int(hip_stream_ptr) == 0:
            self._ck(self._L.tsdf_adopt_null_stream(self._c))
        else:
            self._ck(self._L.tsdf_set_stream(self._c, C.c_void_p(int(hip_stream_ptr))))

    def sync(self):
        self._ck(self._L.tsdf_sync(self._c))

    def set_calibration(self, scene):
        ri = (C.c_uint32 * 3)(*[int(x) for x in scene["inv_res"]])
        rl = (C.c_uint32 * 3)(*[int(x) for x in scene["lut_res"]])
        for i in range(self.n):
            self._ck(self._L.tsdf_set_calibration(self._c, i, _fp(_f32(scene["cv_xyz_inv"][i])), ri,
                                                  _fp(_f32(scene["cv_uv"][i])), rl, _fp(_f32(scene["cv_xyz"][i])), rl))

    def upload_frame(self, scene):
        col = np.ascontiguousarray(scene["color"], np.uint8)
        self._ck(self._L.tsdf_upload_frame(self._c, _fp(_f32(scene["depth"])), _fp(_f32(scene["quality"])),
                                           _fp(_f32(scene["silhouette"])), col.ctypes.data_as(C.POINTER(C.c_uint8))))

    def upload_frame_dev(self, depth_ptr, quality_ptr, silhouette_ptr, colour_ptr=0, complete=False):
        """the frame's arrays are in device memory already (raw device pointers, e.g. torch tensors' data_ptr()): one re-layout launch.
        complete: the arrays are finished when the call is made (TSDF_FRAME_ARRAYS_COMPLETE: the launch need not wait for the context's stream)"""
        self._ck(self._L.tsdf_upload_frame_dev(self._c, C.c_void_p(int(depth_ptr)), C.c_void_p(int(quality_ptr)), C.c_void_p(int(silhouette_ptr)),
                                               C.c_void_p(int(colour_ptr)) if colour_ptr else None, C.c_uint32(1 if complete else 0)))

    # asynchronous upload into the frame slot that is not current (double PBO analog) + slot switch
    def frame_staging(self):
        """numpy views of the pinned staging buffer of the next upload_frame_async (depth_rg, quality, silhouette, colour)"""
        h, w, ch, cw = self._dims
        p = [C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.POINTER(C.c_uint8)()]
        self._ck(self._L.tsdf_frame_staging(self._c, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(p[3])))
        return (np.ctypeslib.as_array(p[0], shape=(self.n, h, w, 2)), np.ctypeslib.as_array(p[1], shape=(self.n, h, w)),
                np.ctypeslib.as_array(p[2], shape=(self.n, h, w)), np.ctypeslib.as_array(p[3], shape=(self.n, ch, cw, 3)))

    def upload_frame_async(self, scene=None, with_colour=True):
        """scene None: the staging buffer was filled in place (frame_staging)"""
        if scene is None:
            self._ck(self._L.tsdf_upload_frame_async(self._c, None, None, None, None, int(with_colour)))
            return
        col = np.ascontiguousarray(scene["color"], np.uint8) if with_colour else None
        self._ck(self._L.tsdf_upload_frame_async(self._c, _fp(_f32(scene["depth"])), _fp(_f32(scene["quality"])), _fp(_f32(scene["silhouette"])),
                                                 col.ctypes.data_as(C.POINTER(C.c_uint8)) if col is not None else None, int(with_colour)))

    def select_frame_slot(self, slot): self._ck(self._L.tsdf_select_frame_slot(self._c, int(slot)))

    def current_frame_slot(self):
        s = C.c_uint32()
        self._ck(self._L.tsdf_current_frame_slot(self._c, C.byref(s)))
        return s.value

    # ------------------------------------------------------------------ NetKinectArray side: raw frame -> processTextures()
    def upload_raw_frame(self, scene):
        col = np.ascontiguousarray(scene["color"], np.uint8)
        self._ck(self._L.tsdf_upload_raw_frame(self._c, _fp(_f32(scene["depth_raw"])), col.ctypes.data_as(C.POINTER(C.c_uint8))))
        self.set_preprocess_calibration(scene)

    def set_preprocess_calibration(self, scene):
        """what processTextures() needs beside the LUTs: CalibVolumes::getDepthLimits / getCameraPositions of every sensor"""
        for i in range(self.n):
            self._ck(self._L.tsdf_set_depth_limits(self._c, i, C.c_float(float(scene["depth_limits"][0])), C.c_float(float(scene["depth_limits"][1]))))
            self._ck(self._L.tsdf_set_camera_position(self._c, i, _fp(_f32(scene["camera_positions"][i]))))
        self._pp_shape = (self.n, scene["height"], scene["width"])

    # ------------------------------------------------------------------ frame ingest: wire message -> raw frame (readLoop / update)
    def setWireFormat(self, color_format=COLOR_RGB8, depth_format=DEPTH_F32):
        self._ck(self._L.tsdf_set_wire_format(self._c, int(color_format), int(depth_format)))

    def wireSizes(self):
        cs, ds, total = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._ck(self._L.tsdf_wire_sizes(self._c, C.byref(cs), C.byref(ds), C.byref(total)))
        return cs.value, ds.value, total.value

    def setDepthCompression(self, stream, compressed, near, far):
        self._ck(self._L.tsdf_set_depth_compression(self._c, int(stream), int(compressed), C.c_float(near), C.c_float(far)))

    def upload_wire_frame(self, message, scene=None):
        """message: bytes-like, per sensor [colour][depth]; returns the timestamp in its first 8 bytes."""
        m = np.frombuffer(message, np.uint8)
        ts = C.c_double()
        self._ck(self._L.tsdf_upload_wire_frame(self._c, m.ctypes.data_as(C.c_void_p), C.c_uint64(m.size), C.byref(ts)))
        if scene is not None:
            for i in range(self.n):
                self._ck(self._L.tsdf_set_depth_limits(self._c, i, C.c_float(float(scene["depth_limits"][0])), C.c_float(float(scene["depth_limits"][1]))))
                self._ck(self._L.tsdf_set_camera_position(self._c, i, _fp(_f32(scene["camera_positions"][i]))))
            self._pp_shape = (self.n, scene["height"], scene["width"])
        return ts.value

    def raw_frame(self):
        """(raw depth [N][H][W], colour RGBA8 [N][ch][cw][4]) as unpacked on the GPU."""
        h, w, ch, cw = self._dims
        d = np.zeros((self.n, h, w), np.float32)
        col = np.zeros((self.n, ch, cw, 4), np.uint8)
        self._ck(self._L.tsdf_download_raw_frame(self._c, _fp(d), col.ctypes.data_as(C.POINTER(C.c_uint8))))
        return d, col

    def setPreprocess(self, filter_textures=True, processed_depth=True, refine=True):
        self._ck(self._L.tsdf_set_preprocess(self._c, int(filter_textures), int(processed_depth), int(refine)))

    def processTextures(self): self._ck(self._L.tsdf_process_textures(self._c))

    def preprocessed(self, lab=True):
        """the products of processTextures(); lab=False leaves out the Lab image, which the library produces on request from the processed frame's inputs
        (an error once a newer raw frame has been uploaded)"""
        n, h, w = self._pp_shape
        out = dict(depth2=np.zeros((n, h, w), np.float32), depth_rg=np.zeros((n, h, w, 2), np.float32), lab=np.zeros((n, h, w, 3), np.float32),
                   depth_b=np.zeros((n, h, w, 2), np.float32), silhouette=np.zeros((n, h, w), np.float32),
                   normals=np.zeros((n, h, w, 3), np.float32), quality=np.zeros((n, h, w), np.float32))
        if not lab:
            del out["lab"]
        self._ck(self._L.tsdf_download_preprocessed(self._c, _fp(out["depth2"]), _fp(out["depth_rg"]), _fp(out["lab"]) if lab else None, _fp(out["depth_b"]),
                                                    _fp(out["silhouette"]), _fp(out["normals"]), _fp(out["quality"])))
        return out

    # ------------------------------------------------------------------ reference operator surface
    def clearOccupiedBricks(self): self._ck(self._L.tsdf_clear_bricks(self._c))
    def markBricks(self): self._ck(self._L.tsdf_mark_bricks(self._c))

    def updateOccupiedBricks(self, want_ratio=True):
        if not want_ratio:
            self._ck(self._L.tsdf_update_occupied(self._c, None))
            return None
        r = C.c_float()
        self._ck(self._L.tsdf_update_occupied(self._c, C.byref(r)))
        return r.value

    def integrate(self): self._ck(self._L.tsdf_integrate(self._c))
    def draw(self, mv, proj): self._ck(self._L.tsdf_raymarch(self._c, _fp(_f32(mv)), _fp(_f32(proj))))
    # kinect::ReconPoints (recon_points.cpp): the point back-end
    def upload_normals(self, normals):
        self._ck(self._L.tsdf_upload_normals(self._c, _fp(_f32(normals))))

    def drawPoints(self, mv, proj):
        self._ck(self._L.tsdf_draw_points(self._c, _fp(_f32(mv)), _fp(_f32(proj))))

    # kinect::ReconTrigrid (recon_trigrid.cpp): the triangle-grid back-end
    def setMinLength(self, v): self._ck(self._L.tsdf_set_min_length(self._c, C.c_float(v)))

    def drawTrigrid(self, mv, proj):
        self._ck(self._L.tsdf_draw_trigrid(self._c, _fp(_f32(mv)), _fp(_f32(proj))))

    # kinect::ReconMVT (recon_mvt.cpp): the triangle grid from the raw depth, bilateral-filtered per grid vertex
    def drawMVT(self, mv, proj):
        self._ck(self._L.tsdf_draw_mvt(self._c, _fp(_f32(mv)), _fp(_f32(proj))))

    def mvt_vertices(self):
        """the last drawMVT's vertex stage: [N][W+1][H+1][2] (filtered depth in metres, lateral quality) of grid vertex (gx, gy) at [l][gy][gx]"""
        h, w, _, _ = self._dims
        out = np.zeros((self.n, w + 1, h + 1, 2), np.float32)
        self._ck(self._L.tsdf_download_mvt_vertices(self._c, _fp(out)))
        return out

    # the client's overlays after drawF() in mono mode (kinect_client.cpp:672-683): "Draw TSDF" (kinect::ReconCalibs) and "Draw frustums"
    def drawCalibVis(self, mv, proj):
        self._ck(self._L.tsdf_draw_calibvis(self._c, _fp(_f32(mv)), _fp(_f32(proj))))

    def setActiveKinect(self, i): self._ck(self._L.tsdf_set_active_kinect(self._c, C.c_uint32(int(i))))

    def drawFrustums(self, mv, proj):
        self._ck(self._L.tsdf_draw_frustums(self._c, _fp(_f32(mv)), _fp(_f32(proj))))

    # ... and the two after them (:685-707): the bounding-box wireframe (gloost::BoundingBox::draw) and the texture view
    # (TextureBlitter::blit of unit 15 + which: 0 = the hole-filling atlas, 1 = the depth-limit image)
    def drawBBox(self, mv, proj):
        self._ck(self._L.tsdf_draw_bbox(self._c, _fp(_f32(mv)), _fp(_f32(proj))))

    def drawTextures(self, which): self._ck(self._L.tsdf_draw_textures(self._c, C.c_uint32(int(which))))

    # the GUI's "Show textures" windows (kinect_client.cpp:483-515): layer `stream` of NetKinectArray's array `type` (0 Color, 1 Depth, 2 Quality,
    # 3 Normals, 4 Silhouette, 5 Orig Depth, 6 LAB colors) as the ImGui image quad rect = (p_min.x, p_min.y, p_max.x, p_max.y), ImGui coordinates
    # (origin top left, y down); clip = ImDrawCmd::ClipRect or None for the whole view
    def drawSensorTexture(self, type, stream, rect, clip=None):
        r = _f32(rect).reshape(-1)
        cl = _f32(clip).reshape(-1) if clip is not None else None
        assert r.size == 4 and (cl is None or cl.size == 4)
        self._ck(self._L.tsdf_draw_sensor_texture(self._c, C.c_uint32(int(type)), C.c_uint32(int(stream)), _fp(r), _fp(cl)))

    def sensorViewSize(self, width):
        """ImVec2(width, width / aspect) of the client's image (kinect_client.cpp:502-509)"""
        out = (C.c_float * 2)()
        self._ck(self._L.tsdf_sensor_view_size(self._c, C.c_float(width), out))
        return float(out[0]), float(out[1])

    # "Draw occupied bricks" (ReconIntegration::drawOccupiedBricks): 12 red lines per brick of the latest updateOccupiedBricks(); the client
    # calls it between the frustums and the bounding box while another back-end is showing.  setDrawBricks(True): drawF() ends with it.
    def drawOccupiedBricks(self, mv, proj):
        self._ck(self._L.tsdf_draw_bricks(self._c, _fp(_f32(mv)), _fp(_f32(proj))))

    def setDrawBricks(self, a): self._ck(self._L.tsdf_set_draw_bricks(self._c, int(bool(a))))

    def calibvis_stats(self):
        """(grid points of the last drawCalibVis, of them removed by its empty-space test)"""
        out = (C.c_uint64 * 2)()
        self._ck(self._L.tsdf_calibvis_stats(self._c, out))
        return int(out[0]), int(out[1])

    def fillColors(self): self._ck(self._L.tsdf_fill_colors(self._c))
    def drawF(self, mv, proj): self._ck(self._L.tsdf_draw_f(self._c, _fp(_f32(mv)), _fp(_f32(proj))))

    def frame_dev(self, mv, proj, new_frame=None, complete=True):
        """one frame of the client's loop in ONE call (tsdf_frame_dev): [the re-layout of a frame that arrived in device memory -- new_frame =
        (depth_rg, quality, silhouette[, colour]) device pointers --,] clear / mark / update of the bricks, integrate, drawF"""
        d, q, s, col = (tuple(new_frame) + (0,))[:4] if new_frame is not None else (0, 0, 0, 0)
        self._ck(self._L.tsdf_frame_dev(self._c, C.c_void_p(d), C.c_void_p(q), C.c_void_p(s), C.c_void_p(col), C.c_uint32(1 if complete else 0),
                                        _fp(_f32(mv)), _fp(_f32(proj))))

    def upload_raw_frame_dev(self, depth_raw_ptr, colour_ptr, complete=False):
        """the RAW frame (depth in metres [N][H][W] float32, colour RGB8) is in device memory already: processTextures() reads it where it lies"""
        self._ck(self._L.tsdf_upload_raw_frame_dev(self._c, C.c_void_p(int(depth_raw_ptr)), C.c_void_p(int(colour_ptr)), C.c_uint32(1 if complete else 0)))

    def frame_raw_dev(self, mv, proj, new_frame=None, complete=True):
        """one frame of the client's loop from the RAW frame in ONE call (tsdf_frame_raw_dev): [new_frame = (depth_raw, colour) device pointers,]
        clearOccupiedBricks, processTextures (marks the bricks), updateOccupiedBricks, integrate, drawF"""
        d, col = tuple(new_frame) if new_frame is not None else (0, 0)
        self._ck(self._L.tsdf_frame_raw_dev(self._c, C.c_void_p(d), C.c_void_p(col), C.c_uint32(1 if complete else 0), _fp(_f32(mv)), _fp(_f32(proj))))

    def setTsdfLimit(self, v): self._ck(self._L.tsdf_set_tsdf_limit(self._c, C.c_float(v)))

    def setVoxelSize(self, size):
        self._ck(self._L.tsdf_set_voxel_size(self._c, C.c_float(size)))
        self._mesh_counts = None                                       # (the mesh went with the old grid)
        self._mesh_slab = None
        r3, b3, s3 = (C.c_uint32 * 3)(), (C.c_uint32 * 3)(), (C.c_float * 3)()
        self._ck(self._L.tsdf_get_resolution(self._c, r3, b3, s3))
        self.res, self.res_bricks, self.brick_size = tuple(r3), tuple(b3), tuple(s3)
    def setUseBricks(self, a): self._ck(self._L.tsdf_set_use_bricks(self._c, int(a)))
    def setSpaceSkip(self, a): self._ck(self._L.tsdf_set_space_skip(self._c, int(a)))
    def setColorFilling(self, a): self._ck(self._L.tsdf_set_color_filling(self._c, int(a)))
    def setMinVoxelsPerBrick(self, n): self._ck(self._L.tsdf_set_min_voxels_per_brick(self._c, int(n)))
    def setMarchCap(self, samples): self._ck(self._L.tsdf_set_march_cap(self._c, C.c_uint32(int(samples))))
    def setShadeMode(self, m): self._ck(self._L.tsdf_set_shade_mode(self._c, int(m)))
    # stereo modes of the client (kinect_client.cpp:616-669): Reconstruction::setViewportOffset / setColorMaskMode + the GL state around them
    def setViewportOffset(self, x, y): self._ck(self._L.tsdf_set_viewport_offset(self._c, C.c_float(x), C.c_float(y)))
    def setViewportOrigin(self, x, y): self._ck(self._L.tsdf_set_viewport_origin(self._c, int(x), int(y)))
    def setColorMaskMode(self, m): self._ck(self._L.tsdf_set_color_mask_mode(self._c, int(m)))
    def setFramebufferClear(self, clear_color): self._ck(self._L.tsdf_set_framebuffer_clear(self._c, int(bool(clear_color))))

    def setBrickSize(self, size):
        s = (C.c_float * 3)(*([size] * 3 if np.isscalar(size) else list(size)))
        self._ck(self._L.tsdf_set_brick_size(self._c, s))
        r3, b3, s3 = (C.c_uint32 * 3)(), (C.c_uint32 * 3)(), (C.c_float * 3)()
        self._ck(self._L.tsdf_get_resolution(self._c, r3, b3, s3))
        self.res_bricks, self.brick_size = tuple(b3), tuple(s3)

    def resize(self, w, h):
        self._ck(self._L.tsdf_resize(self._c, w, h))
        self.view = (w, h)
        n = C.c_uint32()
        self._ck(self._L.tsdf_num_lods(self._c, C.byref(n)))
        self.num_lods = n.value

    def occupiedRatio(self):
        r = C.c_float()
        self._ck(self._L.tsdf_occupied_ratio(self._c, C.byref(r)))
        return r.value

    def getBrickSize(self): return self.brick_size

    def numBricks(self):
        n = C.c_uint32()
        self._ck(self._L.tsdf_num_bricks(self._c, C.byref(n)))
        return n.value

    # ------------------------------------------------------------------ state transfer (tests, harness)
    def tsdf(self):
        out = np.empty((self.res[2], self.res[1], self.res[0]), np.float32)
        self._ck(self._L.tsdf_download_volume(self._c, _fp(out)))
        return out

    def set_tsdf(self, v):
        v = _f32(v)
        assert v.size == self.res[0] * self.res[1] * self.res[2]
        self._ck(self._L.tsdf_upload_volume(self._c, _fp(v)))

    def bricks(self):
        n = self.numBricks()
        cnt, fl = np.empty(n, np.uint32), np.empty(n, np.uint8)
        self._ck(self._L.tsdf_download_bricks(self._c, cnt.ctypes.data_as(C.POINTER(C.c_uint32)), fl.ctypes.data_as(C.POINTER(C.c_uint8))))
        return cnt, fl

    def active_tiles(self):
        """(tile coordinates [n][3] (x, y, z in units of 8 voxels), number of integrated tiles) of the last culled integrate()"""
        n, grid = C.c_uint32(), (C.c_uint32 * 4)()
        self._ck(self._L.tsdf_download_active_tiles(self._c, None, 0, C.byref(n), grid))
        ids = np.zeros(max(1, n.value), np.uint32)
        self._ck(self._L.tsdf_download_active_tiles(self._c, ids.ctypes.data_as(C.POINTER(C.c_uint32)), ids.size, C.byref(n), grid))
        ids = ids[:n.value].astype(np.int64)
        ntx, nty, tz0 = int(grid[0]), int(grid[1]), int(grid[2])
        return np.stack([ids % ntx, (ids // ntx) % nty, tz0 + ids // (ntx * nty)], -1), int(grid[3])

    def integrate_form(self):
        """dict of the last integrate() launch (tsdf_integrate_form): form (one of K1_FORMS), grid (workgroups), items (tiles), culled"""
        out = (C.c_uint32 * 4)()
        self._ck(self._L.tsdf_integrate_form(self._c, out))
        return dict(form=K1_FORMS[int(out[0])], grid=int(out[1]), items=int(out[2]), culled=bool(out[3]))

    def set_counters(self, a):
        a = np.ascontiguousarray(a, np.uint32)
        assert a.size == self.numBricks()
        self._ck(self._L.tsdf_upload_brick_counters(self._c, a.ctypes.data_as(C.POINTER(C.c_uint32))))

    def view_images(self):
        w, h = self.view
        rgba, d, ns, pe = np.empty((h, w, 4), np.float32), np.empty((h, w), np.float32), np.empty((h, w), np.float32), np.empty((h, w, 4), np.float32)
        self._ck(self._L.tsdf_download_image(self._c, _fp(rgba), _fp(d), _fp(ns), _fp(pe)))
        return rgba, d, ns, pe

    def set_view_images(self, rgba, depth):
        self._ck(self._L.tsdf_upload_image(self._c, _fp(_f32(rgba)), _fp(_f32(depth))))

    def framebuffer(self):
        w, h = self.view
        rgba, d = np.empty((h, w, 4), np.float32), np.empty((h, w), np.float32)
        self._ck(self._L.tsdf_download_framebuffer(self._c, _fp(rgba), _fp(d)))
        return rgba, d

    def set_framebuffer(self, rgba, depth):
        w, h = self.view
        rgba, depth = _f32(rgba), _f32(depth)
        assert rgba.shape == (h, w, 4) and depth.shape == (h, w)
        self._ck(self._L.tsdf_upload_framebuffer(self._c, _fp(rgba), _fp(depth)))

    # ------------------------------------------------------------------ frame read-out: the swap (glfwSwapBuffers, source/kinect_client.cpp:533)
    def present_config(self, format=PRESENT_RGBA8, flags=0, slots=3):
        self._ck(self._L.tsdf_present_config(self._c, C.c_uint32(int(format)), C.c_uint32(int(flags)), C.c_uint32(int(slots))))
        self._present_format = int(format)

    def present_size(self):
        n = C.c_uint64()
        self._ck(self._L.tsdf_present_size(self._c, C.byref(n)))
        return n.value

    def present(self, tag=0):
        """queue conversion + copy of the finished framebuffer into the next ring slot; never blocks (TsdfError, code -4, when every slot is taken)"""
        self._ck(self._L.tsdf_present(self._c, C.c_uint64(int(tag))))

    def present_acquire(self, wait=True):
        """the oldest presented frame not yet released as (a numpy COPY of its bytes, tag, (w, h)) -- uint8 [h][w][4] for RGBA8, the flat block
        bytes for DXT1 -- and still held until present_release(); None while its copy is still under way (wait=False)"""
        data, n, tag, size = C.c_void_p(), C.c_uint64(), C.c_uint64(), (C.c_uint32 * 2)()
        self._ck(self._L.tsdf_present_acquire(self._c, C.c_int32(1 if wait else 0), C.byref(data), C.byref(n), C.byref(tag), size))
        if not data.value:
            return None
        a = np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_uint8)), shape=(n.value,)).copy()
        w, h = int(size[0]), int(size[1])
        if getattr(self, "_present_format", PRESENT_RGBA8) == PRESENT_RGBA8:
            a = a.reshape(h, w, 4)
        return a, tag.value, (w, h)

    def present_release(self):
        self._ck(self._L.tsdf_present_release(self._c))

    def atlas(self):
        w, h = self.view
        aw = int(np.float32(w) * np.float32(1.5))
        rgba, d = np.empty((h, aw, 4), np.float32), np.empty((h, aw), np.float32)
        self._ck(self._L.tsdf_download_atlas(self._c, _fp(rgba), _fp(d)))
        return rgba, d

    # ------------------------------------------------------------------ mesh extraction (no counterpart in the reference)
    def extract_mesh(self, normals=True, colours=True, level=0):
        """The fused surface as an indexed triangle mesh (tsdf_mesh_extract): dict(position [V][3] f32, triangles [T][3] uint32, and where asked
        for normal [V][3] f32, colour [V][4] f32 with alpha +1 valid / -1 fallback), in the defined order.  level 1 / 2: the same surface on the
        lattice of every 2nd / 4th voxel (tsdf_mesh_extract_lod); level 0 calls tsdf_mesh_extract itself."""
        nv, nt = C.c_uint64(), C.c_uint64()
        flags = (MESH_NORMALS if normals else 0) | (MESH_COLOURS if colours else 0)
        self._mesh_counts = None
        if level:
            self._ck(self._L.tsdf_mesh_extract_lod(self._c, C.c_uint32(flags), C.c_uint32(int(level)), C.byref(nv), C.byref(nt)))
        else:
            self._ck(self._L.tsdf_mesh_extract(self._c, C.c_uint32(flags), C.byref(nv), C.byref(nt)))
        self._mesh_counts = (nv.value, nt.value)
        return self.download_mesh(normals, colours)

    def download_mesh(self, normals=True, colours=True):
        """the arrays of the last extract_mesh (TsdfError, code -4, for an attribute it did not produce)"""
        if getattr(self, "_mesh_counts", None) is None:
            raise TsdfError(-4, "no mesh (extract_mesh)")
        nv, nt = self._mesh_counts
        out = dict(position=np.zeros((nv, 3), np.float32), triangles=np.zeros((nt, 3), np.uint32))
        if normals:
            out["normal"] = np.zeros((nv, 3), np.float32)
        if colours:
            out["colour"] = np.zeros((nv, 4), np.float32)
        self._ck(self._L.tsdf_mesh_download(self._c, _fp(out["position"]), _fp(out.get("normal")), _fp(out.get("colour")),
                                            out["triangles"].ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def write_ply(self, path):
        """binary little-endian PLY of the last extract_mesh"""
        self._ck(self._L.tsdf_mesh_write_ply(self._c, os.fspath(path).encode()))

    def mesh_stats(self):
        """dict of the last extract_mesh: tiles, tiles_skipped (by class, no voxel read), tiles_with_surface, bytes (of mesh storage)"""
        out = (C.c_uint64 * 4)()
        self._ck(self._L.tsdf_mesh_stats(self._c, out))
        return dict(tiles=int(out[0]), tiles_skipped=int(out[1]), tiles_with_surface=int(out[2]), bytes=int(out[3]))

    # ------------------------------------------------------------------ a Z-slab's part of the mesh (no counterpart in the reference)
    def extract_mesh_slab(self, normals=True, colours=True, level=0):
        """This context's part of the whole volume's mesh (tsdf_mesh_slab_extract): vertices of the owned lattice tile layers -> (n_vertices,
        n_triangles).  The halo must be current, as for a draw.  The triangles exist after mesh_slab_link."""
        nv, nt = C.c_uint64(), C.c_uint64()
        flags = (MESH_NORMALS if normals else 0) | (MESH_COLOURS if colours else 0)
        self._mesh_slab = self._mesh_slab_cc = None
        self._ck(self._L.tsdf_mesh_slab_extract(self._c, C.c_uint32(flags), C.c_uint32(int(level)), C.byref(nv), C.byref(nt)))
        s = 8 << int(level)
        self._mesh_slab = (nv.value, nt.value, (-(-self.res[1] // s), -(-self.res[0] // s)))
        return nv.value, nt.value

    def mesh_slab_seam(self):
        """[nty][ntx] uint32: the slab-local vertex base of every lattice tile of the first owned layer (tsdf_mesh_slab_seam): what the slab below links with"""
        if getattr(self, "_mesh_slab", None) is None:                    # (no sizes: nothing may be copied into a buffer of this method's)
            raise TsdfError(-4, "no slab mesh (extract_mesh_slab)")
        out = np.zeros(self._mesh_slab[2], np.uint32)
        self._ck(self._L.tsdf_mesh_slab_seam(self._c, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def mesh_slab_link(self, vertex_base, above_seam=None):
        """Write the part's triangles with global indices (tsdf_mesh_slab_link): vertex_base = the vertices of the slabs below, above_seam = the
        mesh_slab_seam() of the slab directly above (None at the volume's top)."""
        above = None if above_seam is None else np.ascontiguousarray(above_seam, np.uint32)
        self._ck(self._L.tsdf_mesh_slab_link(self._c, C.c_uint64(int(vertex_base)), above.ctypes.data_as(C.POINTER(C.c_uint32)) if above is not None else None))
        self._mesh_slab_cc = None                                        # (the labels held the indices of the link that was: the library has released them)

    def mesh_slab_download(self, normals=True, colours=True, triangles=True):
        """dict of the part's arrays, shaped as download_mesh's (TsdfError, code -4, before an extract, and for the triangles before a link)"""
        if getattr(self, "_mesh_slab", None) is None:
            raise TsdfError(-4, "no slab mesh (extract_mesh_slab)")
        nv, nt = self._mesh_slab[:2]
        out = dict(position=np.zeros((nv, 3), np.float32))
        if triangles:
            out["triangles"] = np.zeros((nt, 3), np.uint32)
        if normals:
            out["normal"] = np.zeros((nv, 3), np.float32)
        if colours:
            out["colour"] = np.zeros((nv, 4), np.float32)
        self._ck(self._L.tsdf_mesh_slab_download(self._c, _fp(out["position"]), _fp(out.get("normal")), _fp(out.get("colour")),
                                                 out["triangles"].ctypes.data_as(C.POINTER(C.c_uint32)) if triangles else None))
        return out

    def mesh_slab_stats(self):
        """dict of the last extract_mesh_slab: tiles (owned lattice tiles), tiles_skipped, tiles_with_surface, bytes"""
        out = (C.c_uint64 * 4)()
        self._ck(self._L.tsdf_mesh_slab_stats(self._c, out))
        return dict(tiles=int(out[0]), tiles_skipped=int(out[1]), tiles_with_surface=int(out[2]), bytes=int(out[3]))

    # ------------------------------------------------------------------ the components of a Z-slab's part (no counterpart in the reference)
    def mesh_slab_components(self):
        """Step 1 (tsdf_mesh_slab_components): label the linked part alone and build its seam lists -> dict(local_components, down, up, roots): the
        local component count and the three lists' lengths"""
        out = (C.c_uint64 * 4)()
        self._mesh_slab_cc = None
        self._ck(self._L.tsdf_mesh_slab_components(self._c, out))
        self._mesh_slab_cc = dict(local_components=int(out[0]), down=int(out[1]), up=int(out[2]), roots=int(out[3]), owned=None)
        return {k: v for k, v in self._mesh_slab_cc.items() if k != "owned"}

    def _mesh_slab_cc_sizes(self):
        if getattr(self, "_mesh_slab", None) is None or getattr(self, "_mesh_slab_cc", None) is None:   # (no sizes: nothing may be copied into a buffer of this binding's)
            raise TsdfError(-4, "no components of the slab's part (mesh_slab_components after mesh_slab_link)")
        return self._mesh_slab_cc

    def mesh_slab_component_seam(self):
        """dict(down, up (MESH_SEAM_VERTEX_DTYPE), roots (MESH_SEAM_ROOT_DTYPE)): the three lists of the last mesh_slab_components, global indices"""
        n = self._mesh_slab_cc_sizes()
        out = dict(down=np.zeros(n["down"], MESH_SEAM_VERTEX_DTYPE), up=np.zeros(n["up"], MESH_SEAM_VERTEX_DTYPE), roots=np.zeros(n["roots"], MESH_SEAM_ROOT_DTYPE))
        self._ck(self._L.tsdf_mesh_slab_component_seam(self._c, *[out[k].ctypes.data_as(C.c_void_p) for k in ("down", "up", "roots")]))
        return out

    def mesh_slab_link_components(self, component_base, links):
        """Step 3 (tsdf_mesh_slab_link_components): component_base and links = this slab's entries of merge_mesh_component_seams -> the components
        whose representative this part owns (the rows of its table)"""
        n = self._mesh_slab_cc_sizes()
        links = np.ascontiguousarray(links, MESH_COMPONENT_LINK_DTYPE).reshape(-1)
        owned = C.c_uint64()
        self._ck(self._L.tsdf_mesh_slab_link_components(self._c, C.c_uint64(int(component_base)), links.ctypes.data_as(C.c_void_p) if len(links) else None,
                                                        C.c_uint64(len(links)), C.byref(owned)))
        n["owned"] = int(owned.value)
        return n["owned"]

    def mesh_slab_download_components(self):
        """dict(vertex_component [the part's V] uint32, triangle_component [T] uint32 -- GLOBAL numbers --, table [owned] (MESH_COMPONENT_DTYPE, the whole
        components' counts)): concatenated in slab order, what mesh_download_components of a whole-volume context gives"""
        n = self._mesh_slab_cc_sizes()
        if n["owned"] is None:
            raise TsdfError(-4, "the part's components have no global numbers yet (mesh_slab_link_components)")
        nv, nt = self._mesh_slab[:2]
        out = dict(vertex_component=np.zeros(nv, np.uint32), triangle_component=np.zeros(nt, np.uint32), table=np.zeros(n["owned"], MESH_COMPONENT_DTYPE))
        self._ck(self._L.tsdf_mesh_slab_download_components(self._c, *[out[k].ctypes.data_as(C.c_void_p) for k in ("vertex_component", "triangle_component", "table")]))
        return out

    def mesh_slab_component_stats(self):
        """dict: local_components, owned (0 before mesh_slab_link_components), seam_records (down + up), roots_removed (local roots under a smaller final root)"""
        out = (C.c_uint64 * 4)()
        self._ck(self._L.tsdf_mesh_slab_component_stats(self._c, out))
        return dict(local_components=int(out[0]), owned=int(out[1]), seam_records=int(out[2]), roots_removed=int(out[3]))

    # ------------------------------------------------------------------ mesh components (no counterpart in the reference)
    def mesh_components(self):
        """Label the connected components of the current mesh (tsdf_mesh_components: connectivity by index, numbered by smallest vertex) -> their number"""
        n = C.c_uint64()
        self._ck(self._L.tsdf_mesh_components(self._c, C.byref(n)))
        return int(n.value)

    def mesh_download_components(self):
        """dict of the last mesh_components: vertex_component [V] uint32, triangle_component [T] uint32, table [C] (MESH_COMPONENT_DTYPE)"""
        self._ck(self._L.tsdf_mesh_download_components(self._c, None, None, None))      # (TsdfError, code -4, without components of the current mesh)
        nv, nt = self._mesh_counts
        out = dict(vertex_component=np.zeros(nv, np.uint32), triangle_component=np.zeros(nt, np.uint32),
                   table=np.zeros(self.mesh_component_stats()["components"], MESH_COMPONENT_DTYPE))
        self._ck(self._L.tsdf_mesh_download_components(self._c, *[out[k].ctypes.data_as(C.c_void_p) for k in ("vertex_component", "triangle_component", "table")]))
        return out

    def _mesh_kept(self, call):
        nv, nt = C.c_uint64(), C.c_uint64()
        self._ck(call(C.byref(nv), C.byref(nt)))
        self._mesh_counts = (nv.value, nt.value)                         # download_mesh / write_ply / mesh_stats serve the filtered mesh from here on
        return self._mesh_counts

    def mesh_keep(self, keep):
        """Drop every component c of the current mesh with keep[c] == 0 (tsdf_mesh_keep_components; keep: one flag per component) -> (vertices,
        triangles) left.  The components and the mesh's texture taps are gone afterwards: mesh_components() labels the new mesh."""
        self._ck(self._L.tsdf_mesh_download_components(self._c, None, None, None))
        flags = np.ascontiguousarray(np.asarray(keep) != 0, np.uint8)
        if flags.shape != (self.mesh_component_stats()["components"],):
            raise ValueError(f"keep has shape {flags.shape}, the mesh has {self.mesh_component_stats()['components']} components")
        return self._mesh_kept(lambda nv, nt: self._L.tsdf_mesh_keep_components(self._c, flags.ctypes.data_as(C.c_void_p), nv, nt))

    def mesh_filter(self, min_triangles):
        """mesh_keep of the components with at least min_triangles triangles, decided on the device (tsdf_mesh_filter_components)"""
        return self._mesh_kept(lambda nv, nt: self._L.tsdf_mesh_filter_components(self._c, C.c_uint32(int(min_triangles)), nv, nt))

    def mesh_keep_largest(self, k=1):
        """mesh_keep of the k components with the most triangles (ties: the lower component index first)"""
        n_triangles = self.mesh_download_components()["table"]["n_triangles"]
        keep = np.zeros(len(n_triangles), np.uint8)
        keep[np.argsort(-n_triangles.astype(np.int64), kind="stable")[:max(int(k), 0)]] = 1
        return self.mesh_keep(keep)

    def mesh_component_stats(self):
        """dict: components and largest_triangles of the last mesh_components of the current mesh (0 before it and after a keep / filter),
        vertices_removed and triangles_removed by the last keep / filter of this extract"""
        out = (C.c_uint64 * 4)()
        self._ck(self._L.tsdf_mesh_component_stats(self._c, out))
        return dict(components=int(out[0]), largest_triangles=int(out[1]), vertices_removed=int(out[2]), triangles_removed=int(out[3]))

    # ------------------------------------------------------------------ mesh component measures (no counterpart in the reference)
    def _measure_grid(self, g):
        return dict(unit=float(g["unit"][0]), origin=g["origin"][0].copy(), bits=int(g["bits"][0]))

    def mesh_measure_grid(self):
        """dict(unit, origin [3] float32, bits): the measure grid of this context's box (tsdf_mesh_measure_grid_info; needs no mesh)"""
        g = np.zeros(1, MESH_MEASURE_GRID_DTYPE)
        self._ck(self._L.tsdf_mesh_measure_grid_info(self._c, g.ctypes.data_as(C.c_void_p)))
        return self._measure_grid(g)

    def mesh_component_measures(self):
        """Measure every component of the labelled mesh on the device (tsdf_mesh_component_measures: exact integer area, volume, bounds and vertex
        sum on the measure grid) -> the grid, as mesh_measure_grid()"""
        g = np.zeros(1, MESH_MEASURE_GRID_DTYPE)
        self._ck(self._L.tsdf_mesh_component_measures(self._c, g.ctypes.data_as(C.c_void_p)))
        return self._measure_grid(g)

    def mesh_download_component_measures(self):
        """[C] rows of MESH_COMPONENT_MEASURE_DTYPE of the last mesh_component_measures (mesh_measures_si converts them)"""
        rows = np.zeros(max(self.mesh_component_stats()["components"], 1), MESH_COMPONENT_MEASURE_DTYPE)
        self._ck(self._L.tsdf_mesh_download_component_measures(self._c, rows.ctypes.data_as(C.c_void_p)))
        return rows[:self.mesh_component_stats()["components"]]

    def mesh_measure_rule(self, min_triangles=0, min_extent_m=0.0, min_area_m2=0.0, min_volume_m3=0.0, positive_volume=False):
        """A keep rule for mesh_filter_measured on this context's measure grid: mesh_measure_rule_for(unit, ...)"""
        return mesh_measure_rule_for(self.mesh_measure_grid()["unit"], min_triangles, min_extent_m, min_area_m2, min_volume_m3, positive_volume)

    def mesh_filter_measured(self, rule):
        """mesh_keep of the components for which every clause of the rule holds, decided on the device from the measures
        (tsdf_mesh_filter_components_measured; rule: mesh_measure_rule(...)) -> (vertices, triangles) left"""
        r = np.ascontiguousarray(np.asarray(rule, MESH_MEASURE_RULE_DTYPE).reshape(1))
        return self._mesh_kept(lambda nv, nt: self._L.tsdf_mesh_filter_components_measured(self._c, r.ctypes.data_as(C.c_void_p), nv, nt))

    # ------------------------------------------------------------------ mesh streaming (no counterpart in the reference)
    def mesh_stream_config(self, normals=False, colours=False, max_vertices=1 << 20, max_triangles=1 << 21, max_surface_tiles=1 << 14, slots=3, level=0,
                           min_triangles=0, index_format=0, part=False, taps=False):
        """flags, the three capacities and the slot count of the mesh ring (tsdf_mesh_stream_config); the first mesh_stream after it allocates.
        level 1 / 2 (tsdf_mesh_stream_config_lod): every frame is that level's mesh, max_surface_tiles counts its 8^3 lattice tiles.
        min_triangles >= 1 (tsdf_mesh_stream_config_filter): every frame leaves the device without its components of fewer triangles; n_* in a frame's
        info are the filtered counts, needed_* and the capacities those of the unfiltered mesh.
        index_format MESH_INDEX_TILE16 (tsdf_mesh_stream_config_compact): 6-byte tile-local triangles and a tile table instead of uint32 indices.
        part=True (tsdf_mesh_stream_config_part): every frame is this context's PART of the tile-local frame -- the one ring a Z-slab context streams
        through; the capacities are per part, join_mesh_parts joins the slabs' frames.  It has no filter and no uint32 form (ValueError).
        taps=True (tsdf_mesh_stream_config_taps, called after the config): every frame carries its packed texture taps, PACKED_TAP_DTYPE [V][N]."""
        flags = (MESH_NORMALS if normals else 0) | (MESH_COLOURS if colours else 0)
        caps = (C.c_uint32(int(max_vertices)), C.c_uint32(int(max_triangles)), C.c_uint32(int(max_surface_tiles)), C.c_uint32(int(slots)))
        if part:
            if min_triangles or index_format not in (0, MESH_INDEX_TILE16):
                raise ValueError("a part ring has no filter and streams tile-local triangles only")
            self._ck(self._L.tsdf_mesh_stream_config_part(self._c, C.c_uint32(flags), C.c_uint32(int(level)), *caps))
        elif index_format:
            self._ck(self._L.tsdf_mesh_stream_config_compact(self._c, C.c_uint32(flags), C.c_uint32(int(level)), C.c_uint32(int(min_triangles)),
                                                             C.c_uint32(int(index_format)), *caps))
        elif min_triangles:
            self._ck(self._L.tsdf_mesh_stream_config_filter(self._c, C.c_uint32(flags), C.c_uint32(int(level)), C.c_uint32(int(min_triangles)), *caps))
        elif level:
            self._ck(self._L.tsdf_mesh_stream_config_lod(self._c, C.c_uint32(flags), C.c_uint32(int(level)), *caps))
        else:
            self._ck(self._L.tsdf_mesh_stream_config(self._c, C.c_uint32(flags), *caps))
        self._mesh_stream_filtered = bool(min_triangles)                 # (behind the checks: a refused config leaves the ring as it was)
        self._mesh_stream_part = bool(part)
        self._mesh_stream_taps = False                                   # (every config entry turns the taps off)
        if taps:
            self.mesh_stream_config_taps(True)

    def mesh_stream_config_taps(self, taps=True):
        """turn the tap block of the current mesh ring configuration on or off (tsdf_mesh_stream_config_taps; `taps` may be the raw flag word)"""
        self._ck(self._L.tsdf_mesh_stream_config_taps(self._c, C.c_uint32(MESH_STREAM_TAPS if taps is True else int(taps))))
        self._mesh_stream_taps = bool(taps)

    def mesh_stream_tap_flags(self):
        """the tap flags of the mesh ring (tsdf_mesh_stream_tap_flags): MESH_STREAM_TAPS or 0"""
        flags = C.c_uint32()
        self._ck(self._L.tsdf_mesh_stream_tap_flags(self._c, C.byref(flags)))
        return int(flags.value)

    def mesh_stream_frame_taps(self):
        """the packed texture taps of the frame held now (tsdf_mesh_stream_frame_taps): a VIEW of the slot's pinned buffer, PACKED_TAP_DTYPE [V][N];
        TsdfError, code -4, when no frame is held or the ring carries no taps"""
        m = MeshTaps()
        self._ck(self._L.tsdf_mesh_stream_frame_taps(self._c, C.byref(m)))
        nv, n = int(m.n_vertices), int(m.n_streams)
        assert m.taps and int(m.tap_bytes) == PACKED_TAP_DTYPE.itemsize
        if not nv:
            return np.zeros((0, n), PACKED_TAP_DTYPE)
        return np.ctypeslib.as_array(C.cast(m.taps, C.POINTER(C.c_uint16)), shape=(nv * n, 4)).view(PACKED_TAP_DTYPE).reshape(nv, n)

    def mesh_stream_frame_part(self):
        """dict: layers (L0, L1), level, top, seam_tiles of the frame held now (tsdf_mesh_stream_frame_part); TsdfError, code -4, when no frame is held
        or the ring does not stream parts"""
        p = MeshPart()
        self._ck(self._L.tsdf_mesh_stream_frame_part(self._c, C.byref(p)))
        return dict(layers=(int(p.layers[0]), int(p.layers[1])), level=int(p.level), top=bool(p.top), seam_tiles=int(p.seam_tiles))

    def mesh_stream_index_format(self):
        """the index format of the last mesh_stream_config (tsdf_mesh_stream_index_format)"""
        fmt = C.c_uint32()
        self._ck(self._L.tsdf_mesh_stream_index_format(self._c, C.byref(fmt)))
        return int(fmt.value)

    def mesh_stream_frame_compact(self, n_triangles):
        """(table, codes, tiles, level) of the frame held now (tsdf_mesh_stream_frame_compact): VIEWS of the slot's pinned buffer, MESH_TILE_ROW_DTYPE [R]
        and uint16 [n_triangles][3]; TsdfError, code -4, when no frame is held or the ring streams uint32 indices"""
        m = MeshCompact()
        self._ck(self._L.tsdf_mesh_stream_frame_compact(self._c, C.byref(m)))
        rows = int(m.n_tile_rows)
        table = (np.ctypeslib.as_array(C.cast(m.table, C.POINTER(C.c_uint32)), shape=(rows, 4)).view(MESH_TILE_ROW_DTYPE).reshape(rows)
                 if rows else np.zeros(0, MESH_TILE_ROW_DTYPE))
        codes = np.ctypeslib.as_array(m.triangles, shape=(n_triangles, 3)) if n_triangles else np.zeros((0, 3), np.uint16)
        return table, codes, tuple(int(x) for x in m.tiles), int(m.level)

    def mesh_stream_level(self):
        """the level of the last mesh_stream_config (tsdf_mesh_stream_level)"""
        level = C.c_uint32()
        self._ck(self._L.tsdf_mesh_stream_level(self._c, C.byref(level)))
        return int(level.value)

    def mesh_stream_min_triangles(self):
        """min_triangles of the last mesh_stream_config (tsdf_mesh_stream_min_triangles); 0: the ring has no filter"""
        n = C.c_uint32()
        self._ck(self._L.tsdf_mesh_stream_min_triangles(self._c, C.byref(n)))
        return int(n.value)

    def mesh_stream_frame_filter(self):
        """dict: components (of the unfiltered mesh), kept, vertices_removed, triangles_removed of the frame held now (tsdf_mesh_stream_frame_filter);
        TsdfError, code -4, when no frame is held or the ring has no filter"""
        out = (C.c_uint64 * 4)()
        self._ck(self._L.tsdf_mesh_stream_frame_filter(self._c, out))
        return dict(components=int(out[0]), kept=int(out[1]), vertices_removed=int(out[2]), triangles_removed=int(out[3]))

    def mesh_stream(self, tag=0):
        """queue count, scan, emit and the copy of the current surface into the next ring slot; never blocks (TsdfError, code -4, when every slot is taken)"""
        self._ck(self._L.tsdf_mesh_stream(self._c, C.c_uint64(int(tag))))

    def mesh_stream_acquire(self, wait=True):
        """the oldest streamed frame not yet released as (vertices, triangles, info), still held until mesh_stream_release(); None while it is not
        complete on the host (wait=False).  vertices: a VIEW of the slot's pinned buffer, uint16 [V][4] (qx, qy, qz, 0) with stride 8, uint8 [V][16] with
        stride 16 (unpack_mesh_vertices splits it); triangles: a view, uint32 [T][3]; info: dict of the tsdf_mesh_frame fields.
        On a ring of MESH_INDEX_TILE16 triangles is the uint16 [T][3] corner codes and info["compact"] = dict(table, tiles, level): unpack_mesh_triangles(
        table, triangles, tiles) gives the uint32 array."""
        f, ready = MeshFrame(), C.c_int32()
        self._ck(self._L.tsdf_mesh_stream_acquire(self._c, C.c_int32(1 if wait else 0), C.byref(f), C.byref(ready)))
        if not ready.value:
            return None
        nv, nt, stride = int(f.n_vertices), int(f.n_triangles), int(f.vertex_stride)
        raw = np.ctypeslib.as_array(C.cast(f.vertices, C.POINTER(C.c_uint8)), shape=(nv * stride,)) if nv else np.zeros(0, np.uint8)
        vertices = raw.view(np.uint16).reshape(nv, 4) if stride == 8 else raw.reshape(nv, 16)
        compact = self.mesh_stream_index_format() == MESH_INDEX_TILE16
        if not compact:
            triangles = np.ctypeslib.as_array(f.triangles, shape=(nt, 3)) if nt else np.zeros((0, 3), np.uint32)
        info = dict(n_vertices=nv, n_triangles=nt, needed_vertices=int(f.needed_vertices), needed_triangles=int(f.needed_triangles),
                    needed_tiles=int(f.needed_tiles), tag=int(f.tag), flags=int(f.flags), vertex_stride=stride, overflow=int(f.overflow),
                    res=tuple(int(x) for x in f.res), bbox_min=np.array(f.bbox_min[:], np.float32), bbox_max=np.array(f.bbox_max[:], np.float32))
        if compact:
            table, triangles, tiles, level = self.mesh_stream_frame_compact(nt)
            info["compact"] = dict(table=table, tiles=tiles, level=level, triangles_null=not f.triangles)   # (the C frame's uint32 pointer: NULL here)
        return vertices, triangles, info

    def mesh_stream_release(self):
        self._ck(self._L.tsdf_mesh_stream_release(self._c))

    def mesh_stream_take(self, wait=True):
        """acquire, COPY, release: (vertices, triangles, info) as numpy arrays of the caller's own, or None (wait=False, frame not complete).
        With a filter configured info["filter"] is the frame's mesh_stream_frame_filter(), on a part ring info["part"] its mesh_stream_frame_part(),
        with taps configured info["taps"] a copy of its mesh_stream_frame_taps()."""
        got = self.mesh_stream_acquire(wait)
        if got is None:
            return None
        out = (got[0].copy(), got[1].copy(), got[2])
        if "compact" in out[2]:
            out[2]["compact"]["table"] = out[2]["compact"]["table"].copy()
        if getattr(self, "_mesh_stream_filtered", False):
            out[2]["filter"] = self.mesh_stream_frame_filter()
        if getattr(self, "_mesh_stream_part", False):
            out[2]["part"] = self.mesh_stream_frame_part()
        if getattr(self, "_mesh_stream_taps", False):
            # (copied as 8-byte words: numpy copies a structured array record by record, 20 times slower than the words -- 35 ms for c2's 6.7 M taps)
            out[2]["taps"] = self.mesh_stream_frame_taps().view(np.uint64).copy().view(PACKED_TAP_DTYPE)
        self.mesh_stream_release()
        return out

    def mesh_stream_stats(self):
        """dict: frames (queued since the config), overflowed, payload_bytes (copied to the host, tap blocks included, headers not counted),
        device_bytes (held)"""
        out = (C.c_uint64 * 4)()
        self._ck(self._L.tsdf_mesh_stream_stats(self._c, out))
        return dict(frames=int(out[0]), overflowed=int(out[1]), payload_bytes=int(out[2]), device_bytes=int(out[3]))

    # ------------------------------------------------------------------ ray queries (no counterpart in the reference)
    def cast_rays(self, rays, normals=False, colours=False, unit_cube=False):
        """Cast rays into the fused volume (tsdf_cast_rays).  rays: RAY_DTYPE records, or floats [n][8] = origin, t_min, dir, t_max; world coordinates
        unless unit_cube.  -> hits (RAY_HIT_DTYPE [n]), or (hits, surface (RAY_SURFACE_DTYPE [n])) when normals or colours are asked for."""
        rays = as_rays(rays)
        n = len(rays)
        flags = (RAYS_UNIT_CUBE if unit_cube else 0) | (RAY_NORMALS if normals else 0) | (RAY_COLOURS if colours else 0)
        hits = np.zeros(n, RAY_HIT_DTYPE)
        surface = np.zeros(n, RAY_SURFACE_DTYPE) if (normals or colours) else None
        self._ck(self._L.tsdf_cast_rays(self._c, rays.ctypes.data_as(C.c_void_p), C.c_uint64(n), C.c_uint32(flags), hits.ctypes.data_as(C.c_void_p),
                                        surface.ctypes.data_as(C.c_void_p) if surface is not None else None))
        return hits if surface is None else (hits, surface)

    def cast_rays_dev(self, rays_ptr, n, hits_ptr, surface_ptr=0, normals=False, colours=False, unit_cube=False):
        """tsdf_cast_rays_dev: raw device pointers (e.g. torch tensors' data_ptr()) to n 32-byte records each; queued on the context's stream, no host wait.
        The arrays must stay alive until a later sync()."""
        flags = (RAYS_UNIT_CUBE if unit_cube else 0) | (RAY_NORMALS if normals else 0) | (RAY_COLOURS if colours else 0)
        self._ck(self._L.tsdf_cast_rays_dev(self._c, C.c_void_p(int(rays_ptr)), C.c_uint64(int(n)), C.c_uint32(flags), C.c_void_p(int(hits_ptr)),
                                            C.c_void_p(int(surface_ptr)) if surface_ptr else None))

    # ... on Z-slab contexts: every slab casts the same rays and answers for the samples it owns; the parts merge per ray (header: "ray queries: slab parts")
    def cast_rays_part(self, rays, normals=False, colours=False, unit_cube=False):
        """This context's part of a cast (tsdf_cast_rays_part): arguments and results as cast_rays.  Works on any context; on a slab the halo must be
        current, as for a draw.  merge_ray_parts / merge_ray_parts_dev join the parts of contiguous slabs into the whole-volume answer."""
        rays = as_rays(rays)
        n = len(rays)
        flags = (RAYS_UNIT_CUBE if unit_cube else 0) | (RAY_NORMALS if normals else 0) | (RAY_COLOURS if colours else 0)
        hits = np.zeros(n, RAY_HIT_DTYPE)
        surface = np.zeros(n, RAY_SURFACE_DTYPE) if (normals or colours) else None
        self._ck(self._L.tsdf_cast_rays_part(self._c, rays.ctypes.data_as(C.c_void_p), C.c_uint64(n), C.c_uint32(flags), hits.ctypes.data_as(C.c_void_p),
                                             surface.ctypes.data_as(C.c_void_p) if surface is not None else None))
        return hits if surface is None else (hits, surface)

    def cast_rays_part_dev(self, rays_ptr, n, hits_ptr, surface_ptr=0, normals=False, colours=False, unit_cube=False):
        """tsdf_cast_rays_part_dev: raw device pointers to n 32-byte records each; queued on the context's stream, no host wait.  The arrays must stay
        alive until a later sync()."""
        flags = (RAYS_UNIT_CUBE if unit_cube else 0) | (RAY_NORMALS if normals else 0) | (RAY_COLOURS if colours else 0)
        self._ck(self._L.tsdf_cast_rays_part_dev(self._c, C.c_void_p(int(rays_ptr)), C.c_uint64(int(n)), C.c_uint32(flags), C.c_void_p(int(hits_ptr)),
                                                 C.c_void_p(int(surface_ptr)) if surface_ptr else None))

    def merge_ray_parts_dev(self, hit_parts_ptr, surface_parts_ptr, parts, n, stride_records, hits_ptr, surface_ptr=0):
        """tsdf_merge_ray_parts_dev: part k's n records start stride_records records behind part k - 1's (the surface parts alike, or 0 for none);
        queued on the context's stream, no host wait.  Needs no volume: any context merges."""
        self._ck(self._L.tsdf_merge_ray_parts_dev(self._c, C.c_void_p(int(hit_parts_ptr)) if hit_parts_ptr else None,
                                                  C.c_void_p(int(surface_parts_ptr)) if surface_parts_ptr else None, C.c_uint32(int(parts)), C.c_uint64(int(n)),
                                                  C.c_uint64(int(stride_records)), C.c_void_p(int(hits_ptr)) if hits_ptr else None,
                                                  C.c_void_p(int(surface_ptr)) if surface_ptr else None))

    def view_rays(self, mv, proj, rect=None):
        """The draw's own rays (tsdf_view_rays) of the pixel rectangle rect = (x0, y0, w, h), default the whole view: RAY_DTYPE [h * w], row-major,
        unit-cube coordinates -- cast them with unit_cube=True."""
        x0, y0, w, h = rect if rect is not None else (0, 0, self.view[0], self.view[1])
        rays = np.zeros(max(int(w), 0) * max(int(h), 0), RAY_DTYPE)
        self._ck(self._L.tsdf_view_rays(self._c, _fp(_f32(mv).reshape(-1)), _fp(_f32(proj).reshape(-1)), C.c_int32(int(x0)), C.c_int32(int(y0)),
                                        C.c_int32(int(w)), C.c_int32(int(h)), rays.ctypes.data_as(C.c_void_p)))
        return rays

    def pick(self, mv, proj, x, y, colours=True):
        """What is under pixel (x, y) of the view (tsdf_view_rays for the pixel, then tsdf_cast_rays): dict(hit, position (world, vol_to_world of the
        hit's unit-cube position `unit`), t, n_samples, status, normal (world), rgba (zeros with colours=False)); hit=False: n_samples and status only."""
        ray = self.view_rays(mv, proj, (int(x), int(y), 1, 1))
        hits, surface = self.cast_rays(ray, normals=True, colours=colours, unit_cube=True)
        return self.pick_result(hits[0], surface[0])

    def pick_result(self, h, s):
        """pick()'s dict from one unit-cube hit record and its surface record (SlabDriver.pick builds it from the merged parts)"""
        if not (int(h["status"]) & RAY_HIT):
            return dict(hit=False, n_samples=int(h["n_samples"]), status=int(h["status"]))
        lo, hi = self._bbox
        return dict(hit=True, position=(lo + h["pos"] * (hi - lo)).astype(np.float32), unit=h["pos"].copy(), t=float(h["t"]), n_samples=int(h["n_samples"]),
                    status=int(h["status"]), normal=s["normal"].copy(), rgba=s["rgba"].copy())

    def ray_stats(self):
        """dict of the last cast: rays, hits, samples (the definition's, skipped or fetched), fetched (samples whose voxels were read)"""
        out = (C.c_uint64 * 4)()
        self._ck(self._L.tsdf_ray_stats(self._c, out))
        return dict(rays=int(out[0]), hits=int(out[1]), samples=int(out[2]), fetched=int(out[3]))

    # ------------------------------------------------------------------ texture taps (no counterpart in the reference)
    def texture_taps(self, points, unit_cube=False, sensor=False):
        """Per point and stream where the stream's colour image is read and the two numbers blendColors weights the read with (tsdf_texture_taps).
        points: floats [n][3], world coordinates unless unit_cube.  -> taps (TEXTURE_TAP_DTYPE [n][N]), or (taps, sensor records (SENSOR_TAP_DTYPE
        [n][N])) with sensor=True.  blend_from_taps(taps, colour images) is the receiver's rule."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = len(pts)
        flags = (TAPS_UNIT_CUBE if unit_cube else 0) | (TAPS_SENSOR if sensor else 0)
        taps = np.zeros((n, self.n), TEXTURE_TAP_DTYPE)
        sens = np.zeros((n, self.n), SENSOR_TAP_DTYPE) if sensor else None
        self._ck(self._L.tsdf_texture_taps(self._c, pts.ctypes.data_as(C.c_void_p), C.c_uint64(n), C.c_uint32(flags), taps.ctypes.data_as(C.c_void_p),
                                           sens.ctypes.data_as(C.c_void_p) if sens is not None else None))
        return taps if sens is None else (taps, sens)

    def texture_taps_dev(self, points_ptr, n, taps_ptr, sensor_ptr=0, unit_cube=False):
        """tsdf_texture_taps_dev: raw device pointers (e.g. torch tensors' data_ptr()) to n points of 3 floats and n x N 16-byte records; sensor records
        exactly when sensor_ptr is given.  Queued on the context's stream, no host wait; the arrays must stay alive until a later sync()."""
        flags = (TAPS_UNIT_CUBE if unit_cube else 0) | (TAPS_SENSOR if sensor_ptr else 0)
        self._ck(self._L.tsdf_texture_taps_dev(self._c, C.c_void_p(int(points_ptr)), C.c_uint64(int(n)), C.c_uint32(flags), C.c_void_p(int(taps_ptr)),
                                               C.c_void_p(int(sensor_ptr)) if sensor_ptr else None))

    def mesh_texture_taps(self, sensor=False, download=True):
        """Texture taps at the vertices of the last extract_mesh (tsdf_mesh_texture_taps: on the device, over the mesh's stored world positions, with the
        frame slot current NOW) -> taps (TEXTURE_TAP_DTYPE [n_vertices][N]), or (taps, sensor records) with sensor=True; download=False: the counts
        (n_vertices, n_streams) only, the results stay on the device (mesh_download_texture_taps)."""
        nv, ns = C.c_uint64(), C.c_uint32()
        self._ck(self._L.tsdf_mesh_texture_taps(self._c, C.c_uint32(TAPS_SENSOR if sensor else 0), C.byref(nv), C.byref(ns)))
        if not download:
            return int(nv.value), int(ns.value)
        return self.mesh_download_texture_taps(int(nv.value), sensor)

    def mesh_download_texture_taps(self, n_vertices, sensor=False):
        """tsdf_mesh_download_texture_taps for a mesh of n_vertices (what extract_mesh / mesh_texture_taps(download=False) returned)"""
        taps = np.zeros((int(n_vertices), self.n), TEXTURE_TAP_DTYPE)
        sens = np.zeros((int(n_vertices), self.n), SENSOR_TAP_DTYPE) if sensor else None
        self._ck(self._L.tsdf_mesh_download_texture_taps(self._c, taps.ctypes.data_as(C.c_void_p), sens.ctypes.data_as(C.c_void_p) if sens is not None else None))
        return taps if sens is None else (taps, sens)

    def texture_tap_stats(self):
        """dict of the last texture tap call: points, streams, with_quality ((point, stream) pairs with quality > 0), not_evaluated (pairs)"""
        out = (C.c_uint64 * 4)()
        self._ck(self._L.tsdf_texture_tap_stats(self._c, out))
        return dict(points=int(out[0]), streams=int(out[1]), with_quality=int(out[2]), not_evaluated=int(out[3]))

    # ------------------------------------------------------------------ timers / multi-GPU hooks
    def enable_timers(self, on=True): self._ck(self._L.tsdf_enable_timers(self._c, int(on)))

    def timer_ms(self, name):
        ms = C.c_float()
        self._ck(self._L.tsdf_timer_ms(self._c, name.encode(), C.byref(ms)))
        return ms.value

    def set_timer_filter(self, names=None):
        self._ck(self._L.tsdf_set_timer_filter(self._c, (",".join(names)).encode() if names else None))

    def sparse_pool_stats(self):
        need, cap = C.c_uint32(), C.c_uint32()
        self._ck(self._L.tsdf_sparse_pool_stats(self._c, C.byref(need), C.byref(cap)))
        return need.value, cap.value

    def integrate_stats(self):
        """dict of the last integrate() launch: work items (tiles), tiles served from the projection cache, (tile, stream) pairs of those
        evaluated per voxel, tiles taken by the LUT kernel, cache slots in use / capacity (all 0 without the cache)"""
        out = (C.c_uint32 * 6)()
        self._ck(self._L.tsdf_integrate_stats(self._c, out))
        return dict(zip(("items", "cached", "full_pairs", "lut_items", "slots_used", "slots"), [int(v) for v in out]))

    def fill_stats(self):
        """(hole-filling passes so far, of them restricted to the dirty screen tiles)"""
        out = (C.c_uint64 * 2)()
        self._ck(self._L.tsdf_fill_stats(self._c, out))
        return int(out[0]), int(out[1])

    def timer_reserve(self, name, n): self._ck(self._L.tsdf_timer_reserve(self._c, name.encode(), int(n)))

    def timer_begin(self, name): self._ck(self._L.tsdf_timer_begin(self._c, name.encode()))
    def timer_end(self, name): self._ck(self._L.tsdf_timer_end(self._c, name.encode()))
    def timer_end_after_fill(self, name): self._ck(self._L.tsdf_timer_end_after_fill(self._c, name.encode()))
    def set_stage_overlap(self, on): self._ck(self._L.tsdf_set_stage_overlap(self._c, int(bool(on))))

    def timer_samples(self, name, capacity=8192):
        out, n = np.zeros(capacity, np.float32), C.c_uint32()
        self._ck(self._L.tsdf_timer_samples(self._c, name.encode(), _fp(out), capacity, C.byref(n)))
        return out[:n.value].copy()

    def timer_spans(self, name, origin, capacity=8192):
        """(begin, end) in ms after the first begin of timer `origin`, for every invocation of `name` since the last reset"""
        b, e, n = np.zeros(capacity, np.float32), np.zeros(capacity, np.float32), C.c_uint32()
        self._ck(self._L.tsdf_timer_spans(self._c, name.encode(), origin.encode(), _fp(b), _fp(e), capacity, C.byref(n)))
        return b[:n.value].copy(), e[:n.value].copy()

    def timer_stats(self, name):
        n, ms = C.c_uint32(), C.c_float()
        self._ck(self._L.tsdf_timer_stats(self._c, name.encode(), C.byref(n), C.byref(ms)))
        return n.value, ms.value

    # ------------------------------------------------------------------ native RCCL exchange (comm.cpp): one communicator per context
    @staticmethod
    def comm_unique_id():
        """128 bytes made by rank 0 (ncclGetUniqueId); the caller carries them to the other ranks"""
        L = load_library()
        buf = (C.c_uint8 * 128)()
        rc = L.tsdf_comm_unique_id(buf)
        if rc != 0:
            raise TsdfError(rc, "RCCL is not available in this process")
        return bytes(buf)

    def comm_init(self, unique_id, rank, world, dedicated_compositor=False):
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._ck(self._L.tsdf_comm_init(self._c, buf, int(rank), int(world), 1 if dedicated_compositor else 0))

    def comm_destroy(self): self._ck(self._L.tsdf_comm_destroy(self._c))

    def broadcast_frame(self, root, scene=None, dev_ptrs=None):
        """on the root the frame as it arrived -- scene: host arrays, or dev_ptrs: (depth, quality, silhouette, colour) device pointers --, elsewhere nothing"""
        if dev_ptrs is not None:
            self._ck(self._L.tsdf_broadcast_frame(self._c, int(root), *[C.c_void_p(int(p)) for p in dev_ptrs]))
            return
        if scene is None:
            self._ck(self._L.tsdf_broadcast_frame(self._c, int(root), None, None, None, None))
            return
        col = np.ascontiguousarray(scene["color"], np.uint8)
        self._ck(self._L.tsdf_broadcast_frame(self._c, int(root), _fp(_f32(scene["depth"])), _fp(_f32(scene["quality"])), _fp(_f32(scene["silhouette"])),
                                              col.ctypes.data_as(C.POINTER(C.c_uint8))))

    def halo_exchange(self): self._ck(self._L.tsdf_halo_exchange(self._c))
    def composite_gather(self): self._ck(self._L.tsdf_composite_gather(self._c))

    def composite_finish(self):
        r = C.c_uint32()
        self._ck(self._L.tsdf_composite_finish(self._c, C.byref(r)))
        return bool(r.value)

    def comm_set_capacity_limits(self, min_records, max_records=0): self._ck(self._L.tsdf_comm_set_capacity_limits(self._c, int(min_records), int(max_records)))

    def comm_frame_status(self, frame):
        """True: frame `frame` of the native compact composite was built from truncated record lists and not repaired (tsdf_comm_frame_status)"""
        t = C.c_int32()
        self._ck(self._L.tsdf_comm_frame_status(self._c, C.c_uint64(int(frame)), C.byref(t)))
        return bool(t.value)

    def comm_stats(self):
        a, b = C.c_uint32(), C.c_uint32()
        self._ck(self._L.tsdf_comm_stats(self._c, C.byref(a), C.byref(b)))
        return {"regathers": a.value, "overflowed_frames": b.value}

    def halo_info(self):
        layers, nbytes = C.c_uint32(), C.c_uint64()
        self._ck(self._L.tsdf_halo_info(self._c, C.byref(layers), C.byref(nbytes)))
        return layers.value, nbytes.value

    def halo_pack_dev(self, lo_ptr, hi_ptr):
        self._ck(self._L.tsdf_halo_pack_dev(self._c, C.c_void_p(lo_ptr), C.c_void_p(hi_ptr)))

    def halo_unpack_dev(self, below_ptr, above_ptr):
        self._ck(self._L.tsdf_halo_unpack_dev(self._c, C.c_void_p(below_ptr), C.c_void_p(above_ptr)))

    def export_partial_dev(self, dst_ptr):
        self._ck(self._L.tsdf_export_partial_dev(self._c, C.c_void_p(dst_ptr)))

    def export_hits_dev(self, dst_ptr, capacity):
        self._ck(self._L.tsdf_export_hits_dev(self._c, C.c_void_p(dst_ptr), C.c_uint32(capacity)))

    def composite_hits_dev(self, gathered_ptr, n, stride_bytes):
        self._ck(self._L.tsdf_composite_hits_dev(self._c, C.c_void_p(gathered_ptr), C.c_uint32(n), C.c_uint64(stride_bytes)))

    def composite_dev(self, gathered_ptr, n):
        self._ck(self._L.tsdf_composite_dev(self._c, C.c_void_p(gathered_ptr), int(n)))
