"""Case builders for the pre-processing passes (tsdf_process_textures) away from the suite's one image shape, 160 x 120 with colour size = depth size.
Plain numpy over rr.scene.make_scene; tests/test_preprocess_cases.py asserts with the oracle alone that every case is worth running,
tests/test_gpu_preprocess_shapes.py runs them on the device.

  tiny     depth 12 x 10, colour 7 x 5: smaller than the 13 x 13 window and than one 16 x 16 block -- every tap clamps on both sides; a plane with
           two holes (morph fill) and, in the last stream, a depth step (boundary candidates: the Lab tile is larger than the image)
  odd      depth 100 x 75, colour 50 x 37: partial in x and in y for the 16-blocks (4, 11), the 8-cells (4, 3) and the 64 x 4 strips (36, 3);
           3 * 50 * 37 = 5 550 = 2 (mod 4) colour pixels, so the colour layer ends in a partial quad
  sensor   depth 512 x 424 (the reference's depth sensor: 26.5 blocks high), colour 320 x 270
  edge_depths(odd)  NaN, +-inf, negative, subnormal and the limits 0.5 / 4.5 themselves planted in the raw depth (only behind the morph pass)
  compressed(odd)   the 8-bit path's sqrt-coded depth with a different setDepthCompression per stream
"""
import numpy as np

import rgbd_recon_amd as rr

f32 = np.float32
BRICKS = [2.0 / 8, 2.2 / 8, 2.0 / 8]
# volume and view per case: small enough that the oracle's integrate + draw stay well under a second
KW = dict(tiny=dict(res=(32, 32, 32), brick_size=BRICKS, limit=0.04, view=(96, 64)),
          odd=dict(res=(64, 64, 64), brick_size=BRICKS, limit=0.04, view=(96, 64)),
          sensor=dict(res=(64, 64, 64), brick_size=BRICKS, limit=0.04, view=(160, 90)))
ALL_FLAGS = [dict(filter_textures=f, processed_depth=p, refine=r) for f in (True, False) for p in (True, False) for r in (True, False)]
TWO_FLAGS = [dict(), dict(processed_depth=False, refine=False)]
LONE_FLAGS = dict(filter_textures=False, processed_depth=False)   # unfiltered and not dilated by the morph pass: the lone cells of plant_edges stay exactly one cell

TINY_HOLE_1 = (0, 4, 5)                                     # (stream, y, x): one pixel -- filled with the mean of its eight neighbours
TINY_HOLE_9 = (1, slice(3, 6), slice(6, 9))                 # 3 x 3: the rim is filled, the centre sees no valid neighbour and stays empty


def tiny():
    sc = rr.scene.make_scene(n_streams=3, width=12, height=10, color_width=7, color_height=5, lut_res=16, inv_res=16)
    # make_scene's own content has no silhouette pixel at this size: a plane through the box's centre instead (its outer columns leave the box)
    sc["depth_raw"][:] = 2.5
    sc["depth_raw"][TINY_HOLE_1] = 0.0
    sc["depth_raw"][TINY_HOLE_9] = 0.0
    sc["depth_raw"][2, :, 6:] = 2.8                         # a depth step wider than the bilateral range (0.35 * 2.5 / 4.5 m): boundary candidates along it
    return sc


LONE_ROWS = (1, 5)                                           # cell rows of the lone cells at x < 8


def lone_cells(sc):
    """(stream, cell row, first cell column, cell columns) of the lone patches plant_edges plants: where k_pre_quality's blocks -- 2 x 2 cells each -- reach
    past the cell grid in x (W % 16 in 1..8: odd), stream 0's cells (cy, 0); where they reach past it in y (H % 16 in 1..8: sensor), a strip in cell row 0
    of every later stream (as wide as it takes to cover a few voxels: W / 128 cells)"""
    w, h = sc["width"], sc["height"]
    cells = [(0, cy, 0, 1) for cy in LONE_ROWS] if 1 <= w % 16 <= 8 else []
    if 1 <= h % 16 <= 8:
        cells += [(l, 0, w // 16, max(1, w // 128)) for l in range(1, sc["n"])]
    return cells


def plant_edges(sc):
    """make_scene's sphere and box stay in the middle of the image (odd: x 27..79, y 0..54), so every partial block, cell and strip of these shapes would hold
    background only and a wrong range cell or clamped tap there would change nothing.  Flat patches in the raw depth reach the image's borders while their
    world positions stay inside the bounding box: a band along the bottom edge in every stream (2.3 m: the box's full height is in view at that depth), and for
    stream 0 -- the only camera that faces a side of the box squarely, the box ends short of the other cameras' left and right image borders at every depth --
    a band down the right edge into the bottom right corner and one in the bottom left corner (1.65 m: |lateral| <= 0.56 * 1.65 m < 1 m).

    Lone cells (lone_cells): 8 x 8-pixel range cells full of depth with background all around.  They are where a range-cell store that runs past its row or
    its stream lands: k_pre_quality's blocks cover
    2 * ceil(W / 16) cell columns and 2 * ceil(H / 16) cell rows, one more than (W + 7) / 8 = 13 at W = 100 and than (H + 7) / 8 = 53 at H = 424, and an unguarded
    store of cell (cy, 13) goes to ((l * rch + cy) * 13 + 13) = cell (cy + 1, 0), one of cell (53, cx) to cell (0, cx) of stream l + 1 -- the empty range of a
    wave without a pixel.  An empty range drops out of k_pair_masks' min / max over a tile's cells, so with the lone cell lost its tiles see background only
    and are carved where the surface should be integrated (tests/test_preprocess_cases.py::test_a_lost_lone_cell_carves_its_voxels).  A LIMIT: the cell has
    its rightful writer in the same launch, and the last store wins.  The stray wave holds no pixel -- no taps, no powf, its store comes right after the block's
    barrier -- while the rightful wave is full of depth and does all of that first, so the likely order is stray, then rightful, and the cell is repaired: the
    lone cells make such a store visible only when it lands last, they do not pin the guard reliably.  (With filter_textures the bilateral window turns a patch this small into rejected candidates, so
    the cells are uniform -- silhouette 1 -- only when the frame is processed unfiltered.)"""
    w, h, raw = sc["width"], sc["height"], sc["depth_raw"]
    raw[:, int(0.77 * h):, int(0.3 * w):int(0.7 * w)] = 2.3
    raw[0, int(0.27 * h):, int(0.84 * w):] = 1.65
    raw[0, int(0.75 * h):, :int(0.1 * w)] = 1.65
    for l, cy, cx, n in lone_cells(sc):
        raw[l, max(8 * cy - 8, 0):8 * cy + 16, max(8 * cx - 8, 0):8 * (cx + n) + 8] = 0.0
        raw[l, 8 * cy:8 * cy + 8, 8 * cx:8 * (cx + n)] = 1.65 if l == 0 else 2.3
    return sc


def odd(**moved):
    return plant_edges(rr.scene.make_scene(n_streams=3, width=100, height=75, color_width=50, color_height=37, lut_res=16, inv_res=16, **moved))


def sensor():
    return plant_edges(rr.scene.make_scene(n_streams=2, width=512, height=424, color_width=320, color_height=270, lut_res=32, inv_res=32))


# what edge_depths plants, by kind.  pre_morph.fs keeps a depth only if it lies STRICTLY inside (0.5, 4.5): every kind but the two "inside" ones is "no return"
EDGE_KINDS = [("nan", f32(np.nan)), ("+inf", f32(np.inf)), ("-inf", f32(-np.inf)), ("negative", f32(-1.0)), ("min itself", f32(0.5)), ("max itself", f32(4.5)),
              ("inside min", np.nextafter(f32(0.5), f32(1.0))), ("inside max", np.nextafter(f32(4.5), f32(0.0))), ("subnormal", f32(1e-40))]
EDGE_KEPT = ("inside min", "inside max")


def edge_depths(scene, seed=99):
    """-> a copy of `scene` with 1 / 40 of its raw depth pixels replaced, and scene["planted"] = index into EDGE_KINDS per pixel (-1: untouched).
    For processed_depth=True only: without the morph pass non-finite depths reach GLSL min / max, which the language leaves open."""
    sc = dict(scene)
    rng = np.random.default_rng(seed)
    raw = scene["depth_raw"].copy()
    kind = np.where(rng.random(raw.shape) < 1.0 / 40.0, rng.integers(0, len(EDGE_KINDS), raw.shape), -1).astype(np.int8)
    for k, (_, v) in enumerate(EDGE_KINDS):
        raw[kind == k] = v
    sc["depth_raw"], sc["planted"] = raw, kind
    return sc


COMPRESSION = [(1, 0.5, 4.5), (0, 0.5, 4.5), (1, 0.3, 3.0)]  # setDepthCompression(stream, *COMPRESSION[stream])


def depth_codes(d):
    """the 8-bit path's code of a depth in metres, sqrt((d - 0.5) / 4) in [0, 1]; 0 (no return) stays 0"""
    return np.where(d > 0, np.sqrt(np.clip((d - f32(0.5)) / f32(4.0), 0.0, 1.0)), 0.0).astype(f32)


def compressed(scene, coded=None):
    """-> a copy of `scene` whose raw depth is depth_codes() in the streams `coded` (default: those COMPRESSION declares compressed);
    scene["depth_compression"] = COMPRESSION.  Stream 2 decodes the codes with another near / far pair than they were made with (its surfaces move
    towards the camera and stay inside the box).  Stream 1 is declared uncompressed and keeps its metres: codes taken for metres are at most 1 m from
    the camera, outside the bounding box, and leave the stream without a single pixel to compare (coded=(0, 1, 2): tests/test_preprocess_cases.py)."""
    sc = dict(scene)
    d = scene["depth_raw"]
    coded = [i for i, c in enumerate(COMPRESSION) if c[0]] if coded is None else coded
    sc["depth_raw"] = np.stack([depth_codes(d[i]) if i in coded else d[i] for i in range(len(COMPRESSION))])
    sc["depth_compression"] = COMPRESSION
    return sc


def process(recon, scene, flags=None):
    """the raw frame through the passes of `recon` (either side: the HIP context or the oracle)"""
    recon.upload_raw_frame(scene)
    for i, c in enumerate(scene.get("depth_compression", ())):
        recon.setDepthCompression(i, *c)
    recon.setPreprocess(**(flags or {}))
    recon.clearOccupiedBricks()
    recon.processTextures()


def counts(pp, counters):
    """what the boundary pass had to decide, from the oracle's products"""
    rg, db = pp["depth_rg"], pp["depth_b"]
    cand = (rg[..., 0] > 0) & ~(rg[..., 1] > 0.65)          # valid_range, pre_boundary.fs:27-30
    n, h, w = cand.shape
    pad = np.zeros((n, -(-h // 16) * 16, -(-w // 16) * 16), bool)
    pad[:, :h, :w] = cand
    blocks = pad.reshape(n, pad.shape[1] // 16, 16, pad.shape[2] // 16, 16).any(axis=(2, 4))
    return dict(candidates=int(cand.sum()), candidate_blocks=int(blocks.sum()), kept=int((cand & (db[..., 1] == 1.0)).sum()),
                rejected=int((cand & (db[..., 0] == -1.0)).sum()), silhouette=int((pp["silhouette"] > 0).sum()),
                quality=int((pp["quality"] > 0).sum()), bricks=int((np.asarray(counters) > 0).sum()))


def processed_scene(scene, pp):
    """the processed-frame scene (what upload_frame takes) made of a context's own pre-processing products"""
    sc = dict(scene)
    sc.update(depth=np.ascontiguousarray(pp["depth_b"]), quality=np.ascontiguousarray(pp["quality"]), silhouette=np.ascontiguousarray(pp["silhouette"]),
              normals=np.ascontiguousarray(pp["normals"]))
    return sc
