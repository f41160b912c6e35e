"""-m gpu: hole filling -- the pyramid levels of k_inpaint_level / k_inpaint_tail and the pull of k_colorfill -- against the float64 reference
of tests/fill_reference.py, which performs the reference's literal two-atlas sequence and shares no code, no precision and no formulation
with the kernels or the oracle.

Every case holds the kernel AND the oracle to the reference of their own levels (the chain is cut, tests/fill_cases.py), under the one
acceptance rule and the tolerances measured there on the CPU: a failure names the side.  tests/test_fill_reference.py is the half of
this that runs without a GPU.  All contexts go through the C ABI (rr.ReconIntegrationHip).
"""
import numpy as np
import pytest

import fill_cases as C
from oracle.oracle import OracleRecon

pytestmark = pytest.mark.gpu


def pair(rr, **extra):
    return lambda scene, **kw: {"kernel": rr.ReconIntegrationHip(scene, **kw, **extra), "oracle": OracleRecon(scene, **kw)}


@pytest.mark.parametrize("size", list(C.SIZES), ids=lambda s: "x".join(map(str, s)))
def test_fill_uploaded_image(rr, size):
    """5x3: two levels; 16x16: every coordinate product an exact integer; 48x32: every level in k_inpaint_tail; 61x45, 173x99: odd sizes
    (173x99: levels 1 and 2 in k_inpaint_level, the rest in the tail); 1280x720: fp32 and exact inpaint coordinates differ"""
    C.upload_case(pair(rr), size)


@pytest.mark.parametrize("mask", [1, 2])
def test_fill_colour_mask_over_a_kept_framebuffer(rr, mask):
    C.upload_case(pair(rr), C.MASK_SIZE, mask)


def test_fill_past_the_level_tables(rr):
    """no level has alpha > 0 under the surface: the pull reads uniform slots past num_lods, which GL leaves undefined -- kernel and oracle
    must still agree with one another bit for bit, and the reference must exclude exactly those pixels"""
    res = C.past_tables_case(pair(rr))
    for a, b in zip(res["kernel"][0] + res["kernel"][1], res["oracle"][0] + res["oracle"][1]):
        assert C.same_bits(a, b).all()


def test_fill_draw_sequence_by_tiles_and_in_full(rr, monkeypatch):
    """two full fills, then three by dirty tiles under a moving camera, against a context that fills every tile (RR_FILL_TILES=0, read when a
    context is created) and the oracle, which fills every pixel: each one's final atlas and framebuffer against the reference"""
    def make(scene, **kw):
        out = {"kernel by tiles": rr.ReconIntegrationHip(scene, **kw)}
        monkeypatch.setenv("RR_FILL_TILES", "0")
        out["kernel every tile"] = rr.ReconIntegrationHip(scene, **kw)
        monkeypatch.delenv("RR_FILL_TILES")
        out["oracle"] = OracleRecon(scene, **kw)
        return out
    _, objs = C.sequence_case(make)
    assert objs["kernel by tiles"].fill_stats() == (C.SEQ_FRAMES, C.SEQ_FRAMES - 2)          # a condition of the case, not a measurement
    assert objs["kernel every tile"].fill_stats() == (C.SEQ_FRAMES, 0)


@pytest.mark.parametrize("lanes,overlap", [(True, True), (True, False), (False, True)], ids=["lanes-overlap", "lanes-one_after_the_other", "one_stream"])
def test_fill_draw_sequence_fill_lane_and_stage_overlap(rr, lanes, overlap):
    """the fill lane (hole filling of draw f beside what follows, csrc/draw_lanes.hpp) and the stage overlap, on and off"""
    _, objs = C.sequence_case(pair(rr, lane_flags=0 if lanes else rr.LANES_ONE_STREAM), prepare=lambda side, o: o.set_stage_overlap(overlap) if side == "kernel" else None)
    fills, by_tiles = objs["kernel"].fill_stats()
    assert fills == C.SEQ_FRAMES and by_tiles >= 3


def test_fill_by_tiles_with_content_tight_against_the_dirty_tiles(rr):
    """512 x 256, a camera that stands still: levels 1 to 3 go by dirty tiles, and the case itself asserts that content lies in tiles which
    only the parents 2T - 1 / 2T + 2 make dirty, and in the last tile row of level 3 which only the forced row computes"""
    _, objs = C.tile_border_case(pair(rr))
    assert objs["kernel"].fill_stats() == (C.TILE_DRAWS, C.TILE_DRAWS - 2)
