"""numpy restatement of the streamed mesh's packed vertex (include/rgbd_recon_hip.h, "mesh streaming"), on top of tests/mesh_reference.py:
float32 throughout, every operation in the order the header gives.  The inputs are the arrays of the extraction's definition -- the UNIT-CUBE
positions, the world normals, the blendColors values -- so packing the reference's arrays and packing a device's own tsdf_mesh_extract normals and colours go
through the same code.  (The unit-cube positions cannot be recovered from fp32 world positions: a test that packs a device's extract takes them
from mesh_reference.extract of that device's volume, whose world positions it first checks to be bit-equal to the device's.)"""
import numpy as np

import mesh_reference as M

f32 = np.float32


def _rint_i(x):
    """round to nearest, half-way cases to even (np.rint), as an integer"""
    return np.rint(x).astype(np.int64)


def quantise_position(unit):
    """[V][3] unit-cube coordinates -> uint16 [V][4]: (qx, qy, qz, 0), q = rint(min(max(u, 0), 1) * 65535.0f) with the product in fp32"""
    u = np.asarray(unit, f32).reshape(-1, 3)
    q = _rint_i(np.minimum(np.maximum(u, f32(0.0)), f32(1.0)) * f32(65535.0))
    out = np.zeros((len(u), 4), np.uint16)
    out[:, :3] = q
    return out


def dequantise_position(q, bbox_min, bbox_max):
    """what the receiver does: world = bbox_min + (q / 65535) * (bbox_max - bbox_min), in float64 (the receiver's choice)"""
    lo, hi = np.asarray(bbox_min, np.float64), np.asarray(bbox_max, np.float64)
    return lo[None, :] + (np.asarray(q)[:, :3].astype(np.float64) / 65535.0) * (hi - lo)[None, :]


def _sg(x):
    return np.where(x >= 0, f32(1.0), f32(-1.0)).astype(f32)


def encode_normal(n):
    """[V][3] world normals -> int16 [V][2], octahedral; a NaN component: (-32768, -32768)"""
    n = np.asarray(n, f32).reshape(-1, 3)
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(all="ignore"):
        s = ((np.abs(nx) + np.abs(ny)).astype(f32) + np.abs(nz)).astype(f32)
        px, py = (nx / s).astype(f32), (ny / s).astype(f32)
        fx = ((f32(1.0) - np.abs(py)).astype(f32) * _sg(px)).astype(f32)          # the old values on the right
        fy = ((f32(1.0) - np.abs(px)).astype(f32) * _sg(py)).astype(f32)
        fold = nz < 0                                                             # (-0 is not below 0)
        px, py = np.where(fold, fx, px).astype(f32), np.where(fold, fy, py).astype(f32)
        nan = np.isnan(n).any(axis=1)
        code = lambda p: _rint_i(np.where(nan, f32(0.0), np.minimum(np.maximum(p, f32(-1.0)), f32(1.0)) * f32(32767.0)))
        out = np.stack([code(px), code(py)], -1)
    out[nan] = -32768
    return out.astype(np.int16)


def decode_normal(o):
    """int16 [V][2] -> float64 unit normals [V][3] (the NaN code decodes to NaN)"""
    o = np.asarray(o, np.int16).reshape(-1, 2)
    p = o.astype(np.float64) / 32767.0
    z = 1.0 - np.abs(p[:, 0]) - np.abs(p[:, 1])
    sg = lambda x: np.where(x >= 0, 1.0, -1.0)
    fx, fy = (1.0 - np.abs(p[:, 1])) * sg(p[:, 0]), (1.0 - np.abs(p[:, 0])) * sg(p[:, 1])
    x, y = np.where(z < 0, fx, p[:, 0]), np.where(z < 0, fy, p[:, 1])
    v = np.stack([x, y, z], -1)
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    v[(o == -32768).all(axis=1)] = np.nan
    return v


def encode_colour(rgba):
    """[V][4] blendColors values -> uint8 [V][4] by tsdf_present's RGBA8 rule: NaN -> 0, clamp, rint(v * 255.0f) (fallback alpha -1 -> 0, valid +1 -> 255)"""
    v = np.asarray(rgba, f32).reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        c = np.minimum(np.maximum(np.where(np.isnan(v), f32(0.0), v), f32(0.0)), f32(1.0)).astype(f32)
    return _rint_i(c * f32(255.0)).astype(np.uint8)


def pack(unit, normal=None, colour=None):
    """the vertex array of a streamed frame: uint16 [V][4] (stride 8) without attributes, uint8 [V][16] (stride 16) with one or both; an absent one is 0"""
    q = quantise_position(unit)
    if normal is None and colour is None:
        return q
    out = np.zeros((len(q), 16), np.uint8)
    out[:, :8] = q.view(np.uint8).reshape(len(q), 8)
    if normal is not None:
        out[:, 8:12] = encode_normal(normal).view(np.uint8).reshape(len(q), 4)
    if colour is not None:
        out[:, 12:16] = encode_colour(colour)
    return out


def pack_volume(vol, limit, bbox_min, bbox_max, scene=None, normals=False, colours=False):
    """extract + pack: (vertices, triangles, the extraction dict)"""
    m = M.extract(vol, limit, bbox_min, bbox_max)
    n = M.normals(vol, limit, bbox_min, bbox_max, m["unit"]) if normals else None
    c = M.colours(scene, limit, m["unit"]) if colours else None
    return pack(m["unit"], n, c), m["triangles"], m
