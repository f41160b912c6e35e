"""CPU: the packed texture tap of a streamed frame (include/rgbd_recon_hip.h, "mesh streaming: texture taps in the frame") as
tests/mesh_tap_pack_reference.py restates it: the coordinate's 16-bit rule, the binary16 rule, the claim that clamping a coordinate to [0, 1] does not
change a LINEAR, CLAMP_TO_EDGE fetch, and what 16 bits a field cost the receiver's colour on the two scenes of tests/test_gpu_texture_taps.py."""
import numpy as np
import pytest

import main_path_reference as R
import mesh_pack_reference as P
import mesh_reference as M
import mesh_tap_pack_reference as TP
import texture_tap_reference as T

f32 = np.float32
LIMIT = 0.04
RES = (37, 43, 35)
SCENES = {"3-streams": dict(n_streams=3, lut_res=24, inv_res=32), "5-streams": dict(n_streams=5, lut_res=32, inv_res=24)}
# The receiver's rule on unpack(pack(taps)) against the rule on the fp32 taps at the same points, largest channel difference over all vertices, in
# 8-bit steps.  Measured with this file: "3-streams" maximum 0.187 / 255, mean 0.020 / 255 (5 108 vertices); "5-streams" maximum 0.148 / 255, mean
# 0.018 / 255 (5 090 vertices; below 0.25 / 255, so the bound stands).  The bound is half an 8-bit step: 2.7 times the larger measured maximum.  The branch (alpha) must never differ.
COLOUR_BOUND = 0.5 / 255.0


def test_coordinate_rule_clamps_rounds_half_to_even_and_packs_nan_as_zero():
    x = np.array([-0.0, 0.0, 1.0, -1.0e-9, -3.5, -np.inf, 1.0000001, 7.0, np.inf, np.nan, -np.nan, 0.5, 1.0 / 65535.0], f32)
    got = TP.pack_coordinate(x)
    assert got.dtype == np.uint16
    assert got.tolist() == [0, 0, 65535, 0, 0, 0, 65535, 65535, 65535, 0, 0, 32768, 1]
    # half-way products: x * 65535.0f lands exactly on k + 0.5 in fp32 -> the even neighbour (0.5 is one: 32767.5 -> 32768)
    halves = []
    for k in (0, 1, 2, 3, 100, 101, 32766, 32767, 65533, 65534):
        x = f32(f32(k + 0.5) / f32(65535.0))
        for c in (x, np.nextafter(x, f32(0)), np.nextafter(x, f32(2))):   # the quotient or a neighbour: whichever multiplies back to k + 0.5 exactly
            if f32(c * f32(65535.0)) == f32(k + 0.5):
                halves.append((k, c))
                break
    assert len(halves) >= 6, halves
    for k, c in halves:
        assert int(TP.pack_coordinate(c)) == (k if k % 2 == 0 else k + 1), (k, c)
    # it is the position's rule
    u = np.random.default_rng(5).uniform(-0.2, 1.2, (4096, 3)).astype(f32)
    assert TP.pack_coordinate(u).tobytes() == np.ascontiguousarray(P.quantise_position(u)[:, :3]).tobytes()


def test_binary16_rule_keeps_subnormals_overflows_to_infinity_and_has_one_nan():
    bits = lambda *v: TP.pack_half(np.array(v, f32)).tolist()
    assert bits(0.0, -0.0, 1.0, -1.0, 0.5, 65504.0) == [0x0000, 0x8000, 0x3C00, 0xBC00, 0x3800, 0x7BFF]
    # subnormals: 2^-24 is the smallest, 2^-25 is half-way to 0 (even: 0), just above it rounds up; the largest subnormal and the smallest normal
    assert bits(2.0 ** -24, 2.0 ** -25, np.nextafter(f32(2.0 ** -25), f32(1)), 3 * 2.0 ** -24, -(2.0 ** -24), 1023 * 2.0 ** -24, 2.0 ** -14) == \
        [0x0001, 0x0000, 0x0001, 0x0003, 0x8001, 0x03FF, 0x0400]
    # round to nearest even at 11 bits: 1 + 2^-11 is half-way between 1 and 1 + 2^-10 -> even (1); 1 + 3 * 2^-11 -> 1 + 2^-9 (even mantissa 2)
    assert bits(1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, np.nextafter(f32(1.0 + 2.0 ** -11), f32(2))) == [0x3C00, 0x3C02, 0x3C01]
    # overflow: 65520 is half-way between 65504 and 2^16 -> infinity; below it stays finite
    assert bits(65519.996, 65520.0, 1.0e9, -65520.0, np.inf, -np.inf) == [0x7BFF, 0x7C00, 0x7C00, 0xFC00, 0x7C00, 0xFC00]
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0x7FA55AA5, 0xFFC12345], np.uint32).view(f32)
    assert np.isnan(nans).all() and (TP.pack_half(nans) == 0x7E00).all()
    # the round trip of what binary16 holds is exact
    every = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    finite = every[~np.isnan(every.view(np.float16))]
    assert (TP.pack_half(finite.view(np.float16).astype(f32)) == finite).all()


def test_pack_and_unpack_records():
    taps = np.zeros((2, 3), T.TEXTURE_TAP_DTYPE)
    taps["u"], taps["v"], taps["quality"], taps["dist"] = f32(0.25), f32(1.5), f32(0.75), f32(3.0e-6)
    taps[1, 2] = (np.nan, -2.0, np.nan, np.inf)
    p = TP.pack_taps(taps)
    assert p.dtype == TP.PACKED_TAP_DTYPE and p.dtype.itemsize == 8 and p.shape == (2, 3)
    assert p[0, 0].tolist() == (16384, 65535, 0x3A00, 0x0032) and p[1, 2].tolist() == (0, 0, 0x7E00, 0x7C00)
    assert p.tobytes()[:8] == bytes([0x00, 0x40, 0xFF, 0xFF, 0x00, 0x3A, 0x32, 0x00])            # little endian, u v quality dist
    back = TP.unpack_taps(p)
    assert back.dtype == T.TEXTURE_TAP_DTYPE and back["u"][0, 0] == f32(16384) / f32(65535.0) and back["v"][0, 0] == 1.0
    assert back["quality"][0, 0] == 0.75 and back["dist"][0, 0] == f32(50 * 2.0 ** -24)
    assert np.isnan(back["quality"][1, 2]) and np.isinf(back["dist"][1, 2])
    assert TP.pack_taps(back).tobytes() == p.tobytes()
    q = np.array([[0, 65535, 32768, 0], [1, 2, 3, 0]], np.uint16)
    assert TP.vertex_codes(q).tolist() == [[0, 65535, 32768], [1, 2, 3]]
    wide = np.zeros((2, 16), np.uint8)
    wide[:, :8] = q.view(np.uint8).reshape(2, 8)
    wide[:, 8:] = 0xEE
    assert TP.vertex_codes(wide).tolist() == TP.vertex_codes(q).tolist()
    assert TP.unit_of_codes(q[:, :3])[0].tolist() == [0.0, 1.0, float(f32(32768) / f32(65535.0))]


def test_clamping_a_coordinate_does_not_change_a_linear_clamp_to_edge_fetch():
    """for coordinates outside [0, 1] the oracle's LINEAR fetch at x and at clamp(x) agree bit for bit"""
    from oracle import oracle as orc
    rng = np.random.default_rng(11)
    img = rng.uniform(0, 1, (2, 13, 17, 3)).astype(f32)
    outside = np.concatenate([-rng.uniform(1e-7, 3, 40), 1 + rng.uniform(1e-7, 3, 40), [-1e-9, 1.0000001, -1234.5, 99999.0, -0.0, 0.0, 1.0]]).astype(f32)
    inside = rng.uniform(0, 1, len(outside)).astype(f32)
    n = 0
    for x, y in list(zip(outside, inside)) + list(zip(inside, outside)) + list(zip(outside, outside[::-1])):
        a = np.asarray(orc.tex2d_linear(img, 1, x, y), f32)
        b = np.asarray(orc.tex2d_linear(img, 1, np.clip(x, f32(0), f32(1)), np.clip(y, f32(0), f32(1))), f32)
        assert a.tobytes() == b.tobytes(), (x, y)
        n += 1
    assert n == 3 * len(outside)


_CASES = {}


def case(name):
    """per scene, once: the reference mesh of the integrated volume at RES, its packed vertices and the fp32 taps at the vertices' own codes"""
    if name not in _CASES:
        import rgbd_recon_amd as rr
        scene = rr.scene.make_scene(color_width=96, color_height=80, **SCENES[name])
        vol, _ = R.integrate(scene, RES, f32(LIMIT))
        mesh = M.extract(vol, LIMIT, scene["bbox_min"], scene["bbox_max"])
        packed = P.pack(mesh["unit"])
        _CASES[name] = dict(scene=scene, mesh=mesh, packed=packed, taps=TP.frame_taps_f32(scene, LIMIT, packed))
    return _CASES[name]


@pytest.mark.parametrize("name", list(SCENES))
def test_sixteen_bits_a_field_cost_less_than_half_an_8_bit_step_of_colour(name):
    K = case(name)
    taps = K["taps"]
    packed = TP.pack_taps(taps)
    exact, got = T.combine(K["scene"], taps), T.combine(K["scene"], TP.unpack_taps(packed))
    assert (exact[:, 3] == got[:, 3]).all()                              # the branch never differs
    with np.errstate(invalid="ignore"):
        channels = np.abs(exact[:, :3].astype(np.float64) - got[:, :3].astype(np.float64))
    diff = channels.max(axis=1)
    assert not np.isnan(diff).any()
    sub = int(((packed["dist_h"] & 0x7C00) == 0).sum() + (((packed["quality_h"] & 0x7C00) == 0) & ((packed["quality_h"] & 0x3FF) != 0)).sum())
    print(f"{name}: {len(taps)} vertices, colour difference max {diff.max() * 255:.3f} / 255, mean {channels.mean() * 255:.3f} / 255; "
          f"fallback vertices {int((exact[:, 3] < 0).sum())}, pairs with quality {(taps['quality'] > 0).mean():.2f}, binary16-subnormal or zero fields {sub}")
    assert len(taps) > 4000 and (taps["quality"] > 0).mean() > 0.2 and (exact[:, 3] < 0).sum() > 50 and sub > 50   # the scene exercises both branches and subnormals
    assert diff.max() <= COLOUR_BOUND


def test_frame_taps_are_the_taps_at_the_codes_not_at_the_exact_position():
    K = case("3-streams")
    q = TP.vertex_codes(K["packed"])
    u_q = TP.unit_of_codes(q)
    assert u_q.dtype == f32 and u_q.min() >= 0 and u_q.max() <= 1
    assert np.abs(u_q.astype(np.float64) - K["mesh"]["unit"].astype(np.float64)).max() <= 0.5 / 65535 + 1e-7
    assert TP.frame_taps(K["scene"], LIMIT, K["packed"][:200]).tobytes() == TP.pack_taps(K["taps"][:200]).tobytes()
    wide = np.zeros((200, 16), np.uint8)
    wide[:, :8] = K["packed"][:200].view(np.uint8).reshape(200, 8)
    assert TP.frame_taps(K["scene"], LIMIT, wide).tobytes() == TP.pack_taps(K["taps"][:200]).tobytes()
    assert (K["taps"]["dist"] >= 0).all()                                # every pair is evaluated: the not-evaluated record cannot occur
