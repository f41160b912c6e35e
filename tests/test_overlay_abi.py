"""CPU: the overlay entry points (tsdf_draw_calibvis, tsdf_set_active_kinect, tsdf_draw_frustums, tsdf_upload_framebuffer,
tsdf_calibvis_stats) are declared and exported, a NULL context is an error code, not a crash, and the bindings have the calls."""
import ctypes as C

import numpy as np

NAMES = ["tsdf_draw_calibvis", "tsdf_set_active_kinect", "tsdf_draw_frustums", "tsdf_upload_framebuffer", "tsdf_calibvis_stats"]


def test_overlay_entries_are_declared_and_exported(rr):
    syms = rr.declared_symbols()
    lib = rr.load_library()
    for name in NAMES:
        assert name in syms, name
        assert hasattr(lib, name), name


def test_overlay_entries_reject_a_null_context(rr):
    lib = rr.load_library()
    m = np.eye(4, dtype=np.float32).reshape(16)
    fp = m.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.tsdf_draw_calibvis(None, fp, fp) != 0
    assert lib.tsdf_draw_frustums(None, fp, fp) != 0
    assert lib.tsdf_set_active_kinect(None, C.c_uint32(0)) != 0
    assert lib.tsdf_upload_framebuffer(None, fp, fp) != 0
    assert lib.tsdf_calibvis_stats(None, (C.c_uint64 * 2)()) != 0


def test_python_binding_has_the_overlay_calls(rr):
    H = rr.ReconIntegrationHip
    assert all(callable(getattr(H, n)) for n in ("drawCalibVis", "setActiveKinect", "drawFrustums", "set_framebuffer", "calibvis_stats"))
