"""CPU: the MVT back-end's C entry points (tsdf_draw_mvt, tsdf_download_mvt_vertices) are declared and exported, and a NULL
context is an error code, not a crash."""
import ctypes as C

import numpy as np

NAMES = ["tsdf_draw_mvt", "tsdf_download_mvt_vertices"]


def test_mvt_entries_are_declared_and_exported(rr):
    syms = rr.declared_symbols()
    lib = rr.load_library()
    for name in NAMES:
        assert name in syms, name
        assert hasattr(lib, name), name


def test_mvt_entries_reject_a_null_context(rr):
    lib = rr.load_library()
    m = np.eye(4, dtype=np.float32).reshape(16)
    fp = m.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.tsdf_draw_mvt(None, fp, fp) != 0
    out = np.zeros(16, np.float32)
    assert lib.tsdf_download_mvt_vertices(None, out.ctypes.data_as(C.POINTER(C.c_float))) != 0


def test_python_binding_has_the_mvt_calls(rr):
    assert callable(rr.ReconIntegrationHip.drawMVT) and callable(rr.ReconIntegrationHip.mvt_vertices)
