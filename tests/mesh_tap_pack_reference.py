"""numpy restatement of the streamed frame's packed texture taps (include/rgbd_recon_hip.h, "mesh streaming: texture taps in the frame"), on top of
tests/texture_tap_reference.py (the tap's four values) and tests/mesh_pack_reference.py (the position's 16-bit rule): float32 throughout, every
operation in the order the header gives.

The packed tap is 8 bytes, little endian: u, v as uint16 by the position's rule, quality and dist as IEEE binary16.  The taps of a frame are taken at
u_q = q / 65535.0f, the position the receiver reconstructs from the vertex's three codes."""
import numpy as np

import mesh_pack_reference as P
import texture_tap_reference as T

f32 = np.float32
PACKED_TAP_DTYPE = np.dtype([("u", "<u2"), ("v", "<u2"), ("quality_h", "<u2"), ("dist_h", "<u2")])
HALF_NAN = 0x7E00


def pack_coordinate(x):
    """(uint16) rint(min(max(x, 0), 1) * 65535.0f): product in fp32, half-way cases to even; a NaN packs as 0 (max(NaN, 0) = 0, as fmaxf)"""
    x = np.asarray(x, f32)
    with np.errstate(invalid="ignore"):
        c = np.fmin(np.fmax(x, f32(0.0)), f32(1.0)).astype(f32)        # (fmax / fmin return the other operand for a NaN)
    return np.rint((c * f32(65535.0)).astype(f32)).astype(np.uint16)


def pack_half(x):
    """fp32 -> the bits of IEEE binary16: round to nearest even, overflow to +-inf, subnormals kept; every NaN becomes 0x7E00"""
    x = np.asarray(x, f32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        h = x.astype(np.float16).view(np.uint16)
    return np.where(np.isnan(x), np.uint16(HALF_NAN), h).astype(np.uint16)


def pack_taps(taps):
    """TEXTURE_TAP_DTYPE [...] -> PACKED_TAP_DTYPE [...]"""
    taps = np.asarray(taps)
    out = np.zeros(taps.shape, PACKED_TAP_DTYPE)
    out["u"], out["v"] = pack_coordinate(taps["u"]), pack_coordinate(taps["v"])
    out["quality_h"], out["dist_h"] = pack_half(taps["quality"]), pack_half(taps["dist"])
    return out


def unpack_taps(packed):
    """the receiver's unpacking: u = code / 65535.0f, the halfs widened to fp32 -> TEXTURE_TAP_DTYPE [...]"""
    packed = np.asarray(packed)
    out = np.zeros(packed.shape, T.TEXTURE_TAP_DTYPE)
    out["u"] = (packed["u"].astype(f32) / f32(65535.0)).astype(f32)
    out["v"] = (packed["v"].astype(f32) / f32(65535.0)).astype(f32)
    out["quality"] = np.ascontiguousarray(packed["quality_h"]).view(np.float16).astype(f32)
    out["dist"] = np.ascontiguousarray(packed["dist_h"]).view(np.float16).astype(f32)
    return out


def vertex_codes(packed_vertices):
    """the three uint16 position codes of a frame's vertex array (uint16 [V][4] at stride 8, uint8 [V][16] at stride 16) -> uint16 [V][3]"""
    v = np.ascontiguousarray(packed_vertices)
    if v.dtype == np.uint16:
        return v.reshape(-1, 4)[:, :3]
    v = v.reshape(-1, 16)
    return np.ascontiguousarray(v[:, :8]).view("<u2").reshape(-1, 4)[:, :3]


def unit_of_codes(q):
    """u_q = (float) q / 65535.0f per axis: one fp32 division"""
    return (np.asarray(q).astype(f32) / f32(65535.0)).astype(f32)


def frame_taps_f32(scene, limit, packed_vertices):
    """the fp32 taps at the frame's own vertex codes: TEXTURE_TAP_DTYPE [V][N]"""
    return T.taps(scene, limit, unit_of_codes(vertex_codes(packed_vertices)), unit_cube=True)


def frame_taps(scene, limit, packed_vertices):
    """the tap block of a frame, from the frame's own vertex codes: PACKED_TAP_DTYPE [V][N]"""
    return pack_taps(frame_taps_f32(scene, limit, packed_vertices))
