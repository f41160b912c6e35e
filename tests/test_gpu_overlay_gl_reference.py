"""-m gpu: the overlay kernels (k_overlay.hip) and their fp32 twins against the float64 GL reference tests/overlay_gl_reference.py, on the cases
and by the acceptance rule of tests/overlay_gl_cases.py.  A failure names the side that disagrees.  One context per test; the references are
cached per input and shared with tests/test_overlay_gl_reference.py; nothing here reads anything but the repository."""
import pytest

import overlay_gl_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def seen():
    """print, per draw and side, the largest deviations from the reference on the compared pixels (shown with -s, or when the test fails)"""
    C.SEEN.clear()
    yield
    for (kind, side), (d, c) in sorted(C.SEEN.items()):
        t = C.TABLE[kind]
        print(f"{kind} {side}: depth within {d:.3g} (tolerance {t['depth']:g}), colour within {c:.3g} (tolerance {t['colour']:g})")


def both(rr, kind="small", **kw):
    """the sides of a case: the library (one context on scene(kind)) and the twins"""
    hip = rr.ReconIntegrationHip(C.scene(kind), **{**C.kw_of(kind), **kw})
    return {"kernel": C.Kernels(hip), "twin": C.Twins()}, hip


@pytest.mark.parametrize("draw", ["frustums", "bbox", "bricks"])
def test_line_draws(rr, draw):
    sides, _ = both(rr)
    case = {"frustums": C.frustums_case, "bbox": C.bbox_case, "bricks": C.bricks_case}[draw]
    for eye, fb in C.LINE_CASES:
        n, share = case(sides, eye, fb)
        print(f"{draw} eye {eye} over {fb}: {n} touched pixels compared, {share:.2%} excluded")


def test_bricks_shorter_than_a_pixel(rr):
    sides, _ = both(rr, brick_size=C.KW_TINY["brick_size"])
    n, share = C.bricks_case(sides, *C.TINY_CASE)
    print(f"bricks {C.TINY_CASE}: {n} touched pixels compared, {share:.2%} excluded")


@pytest.mark.parametrize("kind", ["small", "grid16"])
def test_calibvis(rr, kind):
    sides, _ = both(rr, kind)
    for c in C.CALIBVIS_CASES:
        if c[0] == kind:
            n, share = C.calibvis_case(sides, *c)
            print(f"calibvis {c}: {n} touched pixels compared, {share:.2%} excluded")


def test_texture_view_both_units(rr):
    sides, hip = both(rr)
    mv, pr = C.matrices(C.BLIT_EYE)
    hip.clearOccupiedBricks(); hip.markBricks(); hip.updateOccupiedBricks(); hip.integrate(); hip.drawF(mv, pr)     # the atlas and the depth-limit image
    for which in (0, 1):
        n, _ = C.blit_case(sides, which)
        assert n == 129 * 49


def processed(rr, kind):
    sc = C.scene(kind)
    sides, hip = both(rr, kind)
    hip.upload_raw_frame(sc)
    hip.clearOccupiedBricks()
    hip.processTextures()
    p, col = hip.preprocessed(), hip.raw_frame()[1]

    def layers_of(side, stream):
        """the library's own products for both sides: the window shows them, and tests/test_gpu_preprocess.py pins them to the oracle's"""
        return {0: col[stream], 1: p["depth_b"][stream], 2: p["quality"][stream], 3: p["normals"][stream], 4: p["silhouette"][stream],
                5: p["depth2"][stream], 6: p["lab"][stream]}
    return sides, layers_of


def test_sensor_windows(rr):
    sides, layers_of = processed(rr, "small")
    for name in C.SENSOR_CASES:
        C.sensor_case(sides, layers_of, name)
    C.sensor_two_windows_case(sides, layers_of)


def test_sensor_windows_with_colour_at_another_resolution(rr):
    sides, layers_of = processed(rr, "colour")
    assert layers_of("kernel", 0)[0].shape[:2] == (88, 200) and layers_of("kernel", 0)[5].shape == (120, 160)
    C.sensor_case(sides, layers_of, "all types", "colour")
