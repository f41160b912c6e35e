"""CPU: the numpy restatement of the streamed mesh's packed vertex (tests/mesh_pack_reference.py) against what the packing promises the receiver:
positions within half a code step, normals within the octahedral code's resolution, the rule's corner cases, the colour rule."""
import numpy as np

import mesh_pack_reference as P
import mesh_reference as M

f32 = np.float32
LIMIT = 0.04
BBOX = (np.array([-1.0, 0.1, -1.2], f32), np.array([1.0, 2.3, 0.8], f32))


def random_volume(res=(20, 22, 19), seed=7):
    rng = np.random.default_rng(seed)
    vol = rng.uniform(-LIMIT, LIMIT, res[::-1]).astype(f32)
    vol[rng.random(vol.shape) < 0.10] = 0.0
    return vol


def test_dequantised_positions_lie_within_half_a_step():
    """Bound per axis, with E the extent and A = max(|bbox_min|, |bbox_max|):
      half a code step, 0.5 / 65535 * E;
    + the fp32 product u * 65535 is off by at most 2^-24 * 65535 = 0.004 steps before it is rounded, which can move a near-tie to the other code;
    + the fp32 world position it is compared with carries two roundings (the product u * E and the sum with bbox_min), each at most 2^-24 * A
      (|u * E| <= E <= 2 A).  Together: (0.5 + 0.004) / 65535 * E + 4 * 2^-24 * A."""
    for vol in (random_volume(), M.sphere_volume((24, 16, 16), limit=LIMIT)):
        m = M.extract(vol, LIMIT, *BBOX)
        assert len(m["position"]) > 1000
        q = P.quantise_position(m["unit"])
        assert q.dtype == np.uint16 and q.shape == (len(m["unit"]), 4) and (q[:, 3] == 0).all()
        ext = (BBOX[1] - BBOX[0]).astype(np.float64)
        amax = np.maximum(np.abs(BBOX[0]), np.abs(BBOX[1])).astype(np.float64)
        tol = (0.5 + 0.004) / 65535.0 * ext + 4 * 2.0 ** -24 * amax
        err = np.abs(P.dequantise_position(q, *BBOX) - m["position"].astype(np.float64))
        print("max position error / bound per axis:", err.max(axis=0) / tol)
        assert (err <= tol[None, :]).all()
        assert (err.max(axis=0) > 0.3 / 65535.0 * ext).all()          # (the bound is not slack by an order of magnitude)


def test_quantiser_clamps_and_rounds_half_to_even():
    u = np.array([[-0.5, 0.0, 1.0], [1.5, 0.5, 2.5 / 65535.0], [-0.0, 1.5 / 65535.0, 3.5 / 65535.0]], f32)
    q = P.quantise_position(u)
    assert q[0].tolist() == [0, 0, 65535, 0] and q[1, 0] == 65535
    # 0.5f * 65535.0f = 32767.5 exactly -> 32768 (even); (k + .5) / 65535 in fp32 times 65535 need not be a tie again: restate in fp32
    assert q[1, 1] == 32768
    for i, j in ((1, 2), (2, 1), (2, 2)):
        assert q[i, j] == int(np.rint(f32(u[i, j]) * f32(65535.0)))


def random_unit_normals(n=20000, seed=11):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v[: n // 20, 2] *= 1e-4                                            # some close to the fold's seam, both sides
    v[: n // 20] /= np.linalg.norm(v[: n // 20], axis=1, keepdims=True)
    return v.astype(f32)


def test_octahedral_codes_decode_to_the_normal():
    """half a code step is 1.5e-5 in the octahedral plane, under 1e-4 rad on the sphere: 1 - cos < 1e-8; the rest (1e-6) is fp32 noise of the input's own
    normalisation"""
    n = random_unit_normals()
    o = P.encode_normal(n)
    assert o.dtype == np.int16 and o.shape == (len(n), 2) and (o > -32768).all()
    d = P.decode_normal(o)
    n64 = n.astype(np.float64)
    n64 /= np.linalg.norm(n64, axis=1, keepdims=True)
    dot = np.einsum("ij,ij->i", d, n64)
    print("min dot:", dot.min())
    assert (dot >= 1 - 1e-6).all()


def test_octahedral_rule_on_its_corner_cases():
    enc = lambda *n: P.encode_normal(np.array([n], f32))[0].tolist()
    assert enc(1, 0, 0) == [32767, 0] and enc(-1, 0, 0) == [-32767, 0]
    assert enc(0, 1, 0) == [0, 32767] and enc(0, -1, 0) == [0, -32767]
    assert enc(0, 0, 1) == [0, 0]
    assert enc(0, 0, -1) == [32767, 32767]                             # the fold of (0, 0): sg(0) = +1 on both axes
    assert enc(0.6, 0.8, -0.0) == enc(0.6, 0.8, 0.0)                   # -0 is not below 0: no fold
    # nz < 0 with px = 0: sg(0) = +1, so the code lands on the +x side: (1 - |py|, 1) with py = 0.6 / 1.4
    py = f32(0.6) / (f32(0.6) + f32(0.8))
    want_x = int(np.rint((f32(1.0) - py) * f32(32767.0)))
    assert enc(0.0, 0.6, -0.8) == [want_x, 32767] and want_x > 0
    assert enc(-0.0, 0.6, -0.8) == [want_x, 32767]                     # (-0 >= 0 too)
    for bad in ((np.nan, 0, 0), (0, np.nan, 1), (0.6, 0.8, np.nan), (np.nan,) * 3):
        assert enc(*bad) == [-32768, -32768]
    assert np.isnan(P.decode_normal(np.array([[-32768, -32768]], np.int16))).all()
    six = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f32)
    assert np.allclose(P.decode_normal(P.encode_normal(six)), six, atol=1e-12)


def test_colour_rule():
    c = np.array([[np.nan, np.inf, -np.inf, -1.0], [1.0, 0.5, 0.25, 1.0], [2.0, -0.0, 1.5 / 255.0, 0.999]], f32)
    got = P.encode_colour(c)
    assert got.dtype == np.uint8
    assert got[0].tolist() == [0, 255, 0, 0]                           # NaN, +inf, -inf, the fallback alpha
    assert got[1].tolist() == [255, 128, 64, 255]                      # 127.5 -> 128 and 63.75 -> 64; the valid alpha
    assert got[2, 0] == 255 and got[2, 1] == 0 and got[2, 3] == 255
    assert got[2, 2] == int(np.rint(f32(1.5 / 255.0) * f32(255.0)))


def test_pack_layout():
    unit = np.array([[0.0, 0.5, 1.0], [0.25, 0.25, 0.25]], f32)
    nrm = np.array([[0, 0, 1], [np.nan, 0, 0]], f32)
    col = np.array([[1, 0, 0.5, 1], [0, 0, 0, -1]], f32)
    bare = P.pack(unit)
    assert bare.dtype == np.uint16 and bare.shape == (2, 4) and bare.tobytes() == P.quantise_position(unit).tobytes()
    full = P.pack(unit, nrm, col)
    assert full.dtype == np.uint8 and full.shape == (2, 16)
    assert full[:, :8].tobytes() == bare.tobytes()
    assert full[:, 8:12].copy().view(np.int16).tolist() == [[0, 0], [-32768, -32768]]
    assert full[:, 12:].tolist() == [[255, 0, 128, 255], [0, 0, 0, 0]]
    assert (P.pack(unit, nrm, None)[:, 12:] == 0).all() and P.pack(unit, nrm, None)[:, :12].tobytes() == full[:, :12].tobytes()
    assert (P.pack(unit, None, col)[:, 8:12] == 0).all() and P.pack(unit, None, col)[:, 12:].tobytes() == full[:, 12:].tobytes()
    assert int.from_bytes(bare.tobytes()[2:4], "little") == 32768       # little endian uint16, qy of vertex 0
