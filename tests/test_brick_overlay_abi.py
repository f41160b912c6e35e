"""CPU: the occupied-brick wireframe entries (tsdf_draw_bricks, tsdf_set_draw_bricks) are declared and exported, a NULL context is an
error code, the Python binding and the C++ adapter have the calls, and the adapter compiles against the header."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "rgbd-recon_amd", "host")
NAMES = ["tsdf_draw_bricks", "tsdf_set_draw_bricks"]


def test_brick_overlay_entries_are_declared_and_exported(rr):
    syms = rr.declared_symbols()
    lib = rr.load_library()
    for name in NAMES:
        assert name in syms, name
        assert hasattr(lib, name), name


def test_brick_overlay_entries_reject_a_null_context(rr):
    lib = rr.load_library()
    m = np.eye(4, dtype=np.float32).reshape(16)
    fp = m.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.tsdf_draw_bricks(None, fp, fp) != 0
    assert lib.tsdf_set_draw_bricks(None, C.c_int32(1)) != 0


def test_python_binding_has_the_brick_overlay_calls(rr):
    H = rr.ReconIntegrationHip
    assert callable(getattr(H, "setDrawBricks")) and callable(getattr(H, "drawOccupiedBricks"))


def test_adapter_draws_the_occupied_bricks():
    text = open(os.path.join(HOST, "recon_integration_hip.hpp")).read()
    assert not re.search(r"drawOccupiedBricks\(\)\s*const\s*\{\s*\}", text), "drawOccupiedBricks() is still empty"
    assert "tsdf_draw_bricks(" in text and "tsdf_set_draw_bricks(" in text
    assert "reference draws nothing" not in text
    gl = open(os.path.join(HOST, "recon_integration_hip_gl.hpp")).read()
    assert not re.search(r"drawOccupiedBricks\(\)\s*const\s*\{\s*\}", gl)
    assert "reference draws nothing" not in gl


def test_adapter_compiles_with_the_brick_overlay(tmp_path):
    src = tmp_path / "use_brick_overlay.cpp"
    src.write_text('#include "recon_integration_hip.hpp"\n'
                   'void frame(kinect::ReconIntegrationHip& recon) {\n'
                   '  recon.setDrawBricks(true);\n'
                   '  recon.drawF();\n'
                   '  recon.drawOccupiedBricks();\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + HOST, str(src)])
