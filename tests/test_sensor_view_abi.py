"""CPU: the sensor texture window entries (tsdf_draw_sensor_texture, tsdf_sensor_view_size) are declared and exported, a NULL context is an
error code, the Python binding and the C++ adapter have the calls, and a snippet that forwards the reference's TexInfo compiles."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "rgbd-recon_amd", "host")
NAMES = ["tsdf_draw_sensor_texture", "tsdf_sensor_view_size"]


def test_sensor_view_entries_are_declared_and_exported(rr):
    syms = rr.declared_symbols()
    lib = rr.load_library()
    for name in NAMES:
        assert name in syms, name
        assert hasattr(lib, name), name


def test_sensor_view_entries_reject_a_null_context(rr):
    lib = rr.load_library()
    rect = np.array([1, 1, 9, 9], np.float32)
    fp = rect.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.tsdf_draw_sensor_texture(None, C.c_uint32(0), C.c_uint32(0), fp, None) != 0
    assert lib.tsdf_draw_sensor_texture(None, C.c_uint32(6), C.c_uint32(0), fp, fp) != 0
    out = (C.c_float * 2)()
    assert lib.tsdf_sensor_view_size(None, C.c_float(480.0), out) != 0


def test_python_binding_has_the_sensor_view_calls(rr):
    H = rr.ReconIntegrationHip
    assert callable(getattr(H, "drawSensorTexture")) and callable(getattr(H, "sensorViewSize"))


def test_adapter_has_the_sensor_view_class_and_the_texture_unit_accessors():
    text = open(os.path.join(HOST, "recon_integration_hip.hpp")).read()
    for cls, methods in (("NetKinectArrayHip", ("getStartTextureUnit", "setStartTextureUnit")), ("SensorTextureViewHip", ("draw", "imageSize"))):
        body = text[text.index("class " + cls):]
        body = body[:body.index("\n};")]
        for m in methods:
            assert m + "(" in body, (cls, m)
    harness = open(os.path.join(HOST, "frame_harness.cpp")).read()
    assert "--sensor-view" in harness and "SensorTextureViewHip" in harness


def test_adapter_compiles_with_a_forwarded_texinfo(tmp_path):
    src = tmp_path / "use_sensor_view.cpp"
    src.write_text('#include <cstdint>\n'
                   '#include <cstring>\n'
                   '#include "recon_integration_hip.hpp"\n'
                   'struct TexInfo { std::uint16_t unit; std::int16_t layer; };\n'                       # imgui_impl_glfw_glb.h:28-40
                   'struct ImVec4 { float x, y, z, w; };\n'
                   'struct ImDrawCmd { unsigned ElemCount; ImVec4 ClipRect; void* TextureId; };\n'
                   'void window(kinect::NetKinectArrayHip& nka, const ImDrawCmd& cmd, const float p_min[2], const float p_max[2]) {\n'
                   '  kinect::SensorTextureViewHip view(nka);\n'
                   '  TexInfo info;\n'
                   '  std::memcpy(&info, &cmd.TextureId, sizeof(info));\n'
                   '  if (info.layer < 0) view.draw(info, p_min, p_max, &cmd.ClipRect.x);\n'
                   '}\n'
                   'float height(kinect::NetKinectArrayHip& nka, int type, int sensor, TexInfo* out) {\n'
                   '  nka.setStartTextureUnit(40);\n'
                   '  *out = TexInfo{(std::uint16_t)(nka.getStartTextureUnit() + type), (std::int16_t)(-sensor - 1)};\n'
                   '  return kinect::SensorTextureViewHip(nka).imageSize(480.0f)[1];\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + HOST, str(src)])
