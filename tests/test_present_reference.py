"""CPU: the numpy restatement of the frame read-out (tests/present_reference.py, the definition in include/rgbd_recon_hip.h) pinned by hand-worked
answers, by the library's own DXT1 decoder (orc.decode_dxt, itself pinned to the reference's squish in test_oracle_ingest.py), and -- for quality --
against the reference's own codec: squish's blocks of two pictures (oracle/_ref/ref_wire_tool compress dxt1; cluster fit is its default) are
recorded in tests/golden/present_squish.npz; where the tool is built it runs and must agree with the recording (RR_RECORD_PRESENT_SQUISH=1 rewrites it).

G, the PSNR the min/max + diagonal encoder may lose against squish, was measured once on the CPU when this test was written and rounded up to the
next 0.5 dB (both encoders are deterministic, so G guards the algorithm, not noise):

    picture                ours      squish    gap     G        ours without the diagonal selection
    picture(64, 48, 1)     32.14 dB  33.30 dB  1.16    1.5 dB   31.81 dB
    render-like 96 x 64    30.57 dB  33.51 dB  2.94    3.0 dB   15.23 dB
"""
import os
import subprocess

import numpy as np
import pytest

import present_reference as P
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "oracle", "_ref", "ref_wire_tool")
GOLDEN = os.path.join(ROOT, "tests", "golden", "present_squish.npz")
F = np.float32
G = {"picture": 1.5, "render": 3.0}


# ------------------------------------------------------------------ RGBA8
def _conv(values):
    fb = np.zeros((1, len(values), 4), np.float32)
    fb[0, :, 0] = values
    return P.to_rgba8(fb)[0, :, 0].tolist()


def test_rgba8_by_hand():
    assert _conv([-0.0, 0.0, 1.0, 1.5, -3.0, np.nan, np.inf, -np.inf]) == [0, 0, 255, 255, 0, 0, 255, 0]
    assert _conv([0.25, 0.75, 1.0 / 255.0, 0.999]) == [64, 191, 1, 255]          # 63.75, 191.25, 1.0, 254.745


def test_rgba8_half_way_products_round_to_even():
    # 0.5 * 255 = 127.5 exactly -> 128; 0.1f * 255 = 25.5 exactly in fp32 (0.1f = 0.100000001490116, the product rounds to 25.5) -> 26;
    # 0.7f * 255 = 178.5 exactly in fp32 (0.7f = 0.699999988079071, the product 178.49999696 is nearer to 178.5 than to its neighbours) -> 178, DOWN:
    # round-half-up would give 179
    for v, prod, want in ((0.5, 127.5, 128), (0.1, 25.5, 26), (0.7, 178.5, 178)):
        assert F(v) * F(255.0) == F(prod)
        assert _conv([v]) == [want]


def test_alpha_converts_like_colour_and_fallback_alpha_becomes_zero():
    fb = np.zeros((2, 3, 4), np.float32)
    fb[..., 3] = [[-1.0, 1.0, 0.5], [2.0, np.nan, 0.1]]
    assert P.to_rgba8(fb)[..., 3].tolist() == [[0, 255, 128], [255, 0, 26]]


def test_row_order():
    fb = np.zeros((3, 2, 4), np.float32)
    fb[:, :, 0] = np.array([0.0, 0.2, 0.4], np.float32)[:, None]                  # window rows 0 (bottom), 1, 2
    assert P.to_rgba8(fb)[:, 0, 0].tolist() == [0, 51, 102]
    assert P.to_rgba8(fb, top_down=True)[:, 0, 0].tolist() == [102, 51, 0]
    assert P.present(fb, P.RGBA8, P.TOP_DOWN).shape == (24,) and P.size_bytes(2, 3, P.RGBA8) == 24
    assert P.size_bytes(22, 9, P.DXT1) == 6 * 3 * 8


# ------------------------------------------------------------------ DXT1 blocks by hand
def _block(b):
    b = np.asarray(b, np.uint8)
    return int(b[0]) | int(b[1]) << 8, int(b[2]) | int(b[3]) << 8, int(b[4]) | int(b[5]) << 8 | int(b[6]) << 16 | int(b[7]) << 24


def test_flat_block_has_equal_endpoints_and_index_zero():
    img = np.zeros((4, 4, 4), np.uint8)
    img[..., :3] = (200, 100, 50)
    c0, c1, word = _block(P.encode_dxt1(img))
    assert c0 == c1 == (200 >> 3) << 11 | (100 >> 2) << 5 | (50 >> 3) and word == 0


def test_c0_equal_c1_after_quantisation_gives_index_zero():
    img = np.zeros((4, 4, 4), np.uint8)
    img[..., :3] = (200, 100, 50)
    img[1, 2, :3] = (203, 101, 53)                                               # differs, but inside the same 565 cell
    c0, c1, word = _block(P.encode_dxt1(img))
    assert c0 == c1 and word == 0


def test_two_colour_block_by_hand():
    # left half black, right half white: lo = 0, hi = 255, inset = 15 -> endpoints 240 and 15 -> 565 (30, 60, 30) and (1, 3, 1); cov > 0, no swap.
    # palette: p0 = (247, 243, 247), p1 = (8, 12, 8), p2 = (167, 166, 167), p3 = (87, 89, 87): white -> 0, black -> 1
    img = np.zeros((4, 4, 4), np.uint8)
    img[:, 2:, :3] = 255
    c0, c1, word = _block(P.encode_dxt1(img))
    assert c0 == (30 << 11 | 60 << 5 | 30) and c1 == (1 << 11 | 3 << 5 | 1)
    row = 1 | 1 << 2                                                              # texels x = 0, 1 -> index 1; x = 2, 3 -> index 0
    assert word == row | row << 8 | row << 16 | row << 24
    # a mid grey (127) in one texel: 40^2 + 39^2 + 40^2 = 4721 from p2, 40^2 + 38^2 + 40^2 = 4644 from p3 -> index 3
    img[0, 0, :3] = 127
    assert _block(P.encode_dxt1(img))[2] == (word & ~3) | 3


def test_negative_covariance_swaps_the_red_ends():
    # red against green, 8 texels each: cov(r, g) < 0.  r: lo' = 15, hi' = 240, g likewise; A = (r lo', g hi') = green, B = red
    img = np.zeros((4, 4, 4), np.uint8)
    img[:, :2, 0] = 255
    img[:, 2:, 1] = 255
    c0, c1, word = _block(P.encode_dxt1(img))
    green, red = 1 << 11 | 60 << 5, 30 << 11 | 3 << 5
    assert (c0, c1) == (red, green)                                              # (A565 < B565: step 5 swaps them)
    row = 1 << 4 | 1 << 6                                                         # red texels -> c0 (index 0), green texels -> c1 (index 1)
    assert word == row | row << 8 | row << 16 | row << 24
    # without the selection both ends are grey-yellow (240, 240, 0) / (15, 15, 0): neither red nor green is on the palette's line
    n0, n1, _ = _block(P.encode_dxt1(img, diagonal=False))
    assert (n0, n1) == (30 << 11 | 60 << 5, 1 << 11 | 3 << 5)


def test_partial_block_replicates_the_last_column_and_row():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (3, 2, 4), dtype=np.uint8)
    full = np.zeros((4, 4, 4), np.uint8)
    for y in range(4):
        for x in range(4):
            full[y, x] = img[min(y, 2), min(x, 1)]
    np.testing.assert_array_equal(P.encode_dxt1(img), P.encode_dxt1(full))
    assert P.encode_dxt1(rng.integers(0, 256, (9, 22, 4), dtype=np.uint8)).size == 6 * 3 * 8


def test_block_order_and_orientation():
    # 8 x 8: four flat blocks of different colours; blocks are row-major in OUTPUT order, so top-down reverses the block rows
    fb = np.zeros((8, 8, 4), np.float32)
    fb[:4, :4, 0], fb[:4, 4:, 1], fb[4:, :4, 2], fb[4:, 4:, :3] = 1.0, 1.0, 1.0, 1.0
    heads = lambda b: [_block(b[8 * k: 8 * k + 8])[0] for k in range(4)]
    assert heads(P.present(fb, P.DXT1, 0)) == [0xF800, 0x07E0, 0x001F, 0xFFFF]
    assert heads(P.present(fb, P.DXT1, P.TOP_DOWN)) == [0x001F, 0xFFFF, 0xF800, 0x07E0]


# ------------------------------------------------------------------ against the library's decoder and the reference's codec
def picture(w, h, seed=0):
    """test_oracle_ingest.py's generator: smooth gradients + an edge + noise (blocks of every kind), alpha 255"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) % 256, 255 * ((x // 8 + y // 8) % 2)], -1).astype(np.int32)
    img[h // 3: h // 2] += rng.integers(-40, 40, (h // 2 - h // 3, w, 4))
    img[:, w // 2:, :3] = img[:, w // 2:, :3] // 3
    img = np.clip(img, 0, 255).astype(np.uint8)
    img[..., 3] = 255
    return img


def render_like(w=96, h=64):
    """what a frame looks like: black background, a shaded disc that carries a red / green checker of 3-pixel squares (blocks that straddle two
    squares hold red AGAINST green: the case the diagonal selection is for)"""
    y, x = np.mgrid[0:h, 0:w]
    r2 = ((x - w / 2 + 0.5) / (0.42 * w)) ** 2 + ((y - h / 2 + 0.5) / (0.45 * h)) ** 2
    shade = np.sqrt(np.clip(1.0 - r2, 0.0, 1.0))
    red = ((x // 3 + y // 3) % 2) == 0
    img = np.zeros((h, w, 4), np.float64)
    img[..., 0] = np.where(red, 230.0, 25.0) * shade
    img[..., 1] = np.where(red, 30.0, 215.0) * shade
    img[..., 2] = 20.0 * shade
    img[r2 >= 1.0, :3] = 0.0
    out = np.rint(img).astype(np.uint8)
    out[..., 3] = 255
    return out


PICTURES = {"picture": lambda: picture(64, 48, seed=1), "render": render_like}


def squish_blocks(name, img, tmp_path):
    rec = None
    if os.path.exists(GOLDEN):
        with np.load(GOLDEN, allow_pickle=False) as z:
            rec = z[name] if name in z.files else None
    if os.path.exists(TOOL):
        h, w = img.shape[:2]
        (tmp_path / "in.rgba").write_bytes(img.tobytes())
        subprocess.check_call([TOOL, "compress", "dxt1", str(tmp_path / "in.rgba"), str(w), str(h), str(tmp_path / "b.dxt")])
        got = np.fromfile(tmp_path / "b.dxt", np.uint8)
        if os.environ.get("RR_RECORD_PRESENT_SQUISH") == "1":
            old = {}
            if os.path.exists(GOLDEN):
                with np.load(GOLDEN, allow_pickle=False) as z:
                    old = {k: z[k] for k in z.files}
            old[name] = got
            np.savez_compressed(GOLDEN, **old)
            rec = got
        assert rec is not None, "tests/golden/present_squish.npz lacks this picture: record it with RR_RECORD_PRESENT_SQUISH=1"
        np.testing.assert_array_equal(got, rec, "the reference's squish no longer gives the recorded blocks")
        return got
    assert rec is not None, "ref_wire_tool is not built here and tests/golden/present_squish.npz lacks this picture"
    return rec


@pytest.mark.parametrize("name", sorted(PICTURES))
def test_decoded_blocks_hold_palette_colours_only(name):
    img = PICTURES[name]()
    h, w = img.shape[:2]
    blocks = P.encode_dxt1(img)
    dec = orc.decode_dxt(blocks, w, h, 1)
    assert (dec[..., 3] == 255).all()                                            # opaque four-colour mode only: never the transparent index
    b = blocks.reshape(h // 4, w // 4, 8).astype(np.int64)
    c0, c1 = b[..., 0] | b[..., 1] << 8, b[..., 2] | b[..., 3] << 8
    assert (c0 >= c1).all()
    assert (b[..., 4:][c0 == c1] == 0).all()
    p0, p1 = P._expand565(c0), P._expand565(c1)
    pal = np.stack([p0, p1, (2 * p0 + p1) // 3, (p0 + 2 * p1) // 3], 2)           # [nby][nbx][4][3]
    tex = dec[..., :3].reshape(h // 4, 4, w // 4, 4, 3).transpose(0, 2, 1, 3, 4).reshape(h // 4, w // 4, 16, 1, 3).astype(np.int64)
    on_palette = (tex == pal[:, :, None]).all(-1).any(-1)
    assert on_palette.all()
    # ... and each texel got the palette entry nearest to its source colour
    src = P._blocks(img)[:, :, :, None, :]
    d = ((src - pal[:, :, None]) ** 2).sum(-1)
    chosen = ((tex - src) ** 2).sum(-1)[..., 0]
    np.testing.assert_array_equal(chosen, d.min(-1))


@pytest.mark.parametrize("name", sorted(PICTURES))
def test_quality_against_the_reference_squish(name, tmp_path):
    img = PICTURES[name]()
    h, w = img.shape[:2]
    ref = squish_blocks(name, img, tmp_path)
    rgb = img[..., :3]
    ours = P.psnr(orc.decode_dxt(P.encode_dxt1(img), w, h, 1)[..., :3], rgb)
    plain = P.psnr(orc.decode_dxt(P.encode_dxt1(img, diagonal=False), w, h, 1)[..., :3], rgb)
    squish = P.psnr(orc.decode_dxt(ref, w, h, 1)[..., :3], rgb)
    print(f"{name}: ours {ours:.2f} dB, squish {squish:.2f} dB, gap {squish - ours:.2f} dB, without the diagonal selection {plain:.2f} dB")
    assert ours >= squish - G[name]
    if name == "render":
        assert ours > plain
