"""CPU: the texture tap entries (tsdf_texture_taps / tsdf_texture_taps_dev / tsdf_mesh_texture_taps / tsdf_mesh_download_texture_taps /
tsdf_texture_tap_stats) are declared and exported, a NULL context is an error code, the two records are 16 bytes with the same offsets in C and in the
ctypes and numpy mirrors, the header states the definition, the Python binding and the C++ adapter have the calls, and a snippet that textures a mesh
through the adapter compiles."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "rgbd-recon_amd", "host")
CSRC = os.path.join(ROOT, "rgbd-recon_amd", "csrc")
NAMES = ["tsdf_texture_taps", "tsdf_texture_taps_dev", "tsdf_mesh_texture_taps", "tsdf_mesh_download_texture_taps", "tsdf_texture_tap_stats"]


def test_texture_tap_entries_are_declared_and_exported(rr):
    syms = rr.declared_symbols()
    lib = rr.load_library()
    for name in NAMES:
        assert name in syms, name
        assert hasattr(lib, name), name
    text = open(rr.HEADER_PATH).read()
    for macro, value in (("TSDF_TAPS_UNIT_CUBE", "1u"), ("TSDF_TAPS_SENSOR", "2u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (macro, value), text), macro
    assert (rr.TAPS_UNIT_CUBE, rr.TAPS_SENSOR) == (1, 2)


def test_texture_tap_entries_reject_a_null_context(rr):
    lib = rr.load_library()
    p, tap, sen, out = (C.c_float * 3)(), rr.TextureTap(), rr.SensorTap(), (C.c_uint64 * 4)()
    nv, ns = C.c_uint64(), C.c_uint32()
    assert lib.tsdf_texture_taps(None, p, C.c_uint64(1), C.c_uint32(0), C.byref(tap), None) == -1
    assert lib.tsdf_texture_taps_dev(None, p, C.c_uint64(1), C.c_uint32(0), C.byref(tap), None) == -1
    assert lib.tsdf_mesh_texture_taps(None, C.c_uint32(0), C.byref(nv), C.byref(ns)) == -1
    assert lib.tsdf_mesh_download_texture_taps(None, C.byref(tap), C.byref(sen)) == -1
    assert lib.tsdf_texture_tap_stats(None, out) == -1


def test_records_are_16_bytes_in_c_and_in_the_mirrors(rr, tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rgbd_recon_hip.h"\n'
                   '_Static_assert(sizeof(tsdf_texture_tap) == 16 && sizeof(tsdf_sensor_tap) == 16, "16-byte records");\n'
                   'int main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(tsdf_texture_tap), offsetof(tsdf_texture_tap, u), offsetof(tsdf_texture_tap, v),\n'
                   '         offsetof(tsdf_texture_tap, quality), offsetof(tsdf_texture_tap, dist));\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(tsdf_sensor_tap), offsetof(tsdf_sensor_tap, x), offsetof(tsdf_sensor_tap, y), offsetof(tsdf_sensor_tap, z),\n'
                   '         offsetof(tsdf_sensor_tap, depth));\n'
                   '  printf("%u %u\\n", TSDF_TAPS_UNIT_CUBE, TSDF_TAPS_SENSOR);\n'
                   '  return 0;\n}\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    rows = [[int(v) for v in line.split()] for line in subprocess.check_output([exe], text=True).splitlines()]
    T, S = rr.TextureTap, rr.SensorTap
    assert rows[0] == [C.sizeof(T), T.u.offset, T.v.offset, T.quality.offset, T.dist.offset] == [16, 0, 4, 8, 12]
    assert rows[1] == [C.sizeof(S), S.x.offset, S.y.offset, S.z.offset, S.depth.offset] == [16, 0, 4, 8, 12]
    assert rows[2] == [1, 2]
    for dt, names in ((rr.TEXTURE_TAP_DTYPE, ("u", "v", "quality", "dist")), (rr.SENSOR_TAP_DTYPE, ("x", "y", "z", "depth"))):
        assert dt.itemsize == 16 and dt.names == names
        assert [dt.fields[name][1] for name in dt.names] == [0, 4, 8, 12], dt


def test_header_states_the_definition(rr):
    text = open(rr.HEADER_PATH).read()
    doc = text[text.index("texture taps: per-stream colour coordinates and blend weights at caller-given points"):text.index("#define TSDF_TAPS_UNIT_CUBE")]
    for cite in ("tsdf_raymarch.fs:295-330", "recon_integration.cpp:66-72", "no counterpart", "u = (p - bbox_min) / e", "the difference, then the division",
                 "u = p", "1.0e6f", "{0, 0, 0, -1}", "dist == -1", "pc = texture(cv_xyz_inv[i], u).xyz", "pcol = texture(cv_uv[i], pc).xy", "NEAREST depth",
                 "dist = |depth - pc.z|", "quality = dist < limit", "A NaN stays a NaN", "unclamped", "LINEAR, CLAMP_TO_EDGE",
                 "tw = sum_i quality_i / (dist_i + 0.01f)", "(sum_i col_i / dist_i) / (sum_i 1.0f / dist_i)", "left to right, in stream order",
                 "{x, y, z, depth}", "[n][N], point-major", "allocates nothing", "Z-slab", "before the first tsdf_integrate", "not at the extract",
                 "TSDF_TAPS_UNIT_CUBE is TSDF_ERR_INVALID_ARGUMENT", "pairs not evaluated", "2^40", "texture_taps", "tests/texture_tap_reference.py"):
        assert cite in doc, cite


def test_python_binding_has_the_texture_tap_calls(rr):
    H = rr.ReconIntegrationHip
    for name in ("texture_taps", "texture_taps_dev", "mesh_texture_taps", "mesh_download_texture_taps", "texture_tap_stats"):
        assert callable(getattr(H, name)), name
    assert callable(rr.blend_from_taps)


def test_adapter_has_the_texture_tap_calls_and_says_the_reference_has_none():
    text = open(os.path.join(HOST, "recon_integration_hip.hpp")).read()
    body = text[text.index("class ReconIntegrationHip"):]
    body = body[:body.index("\n};")]
    for m in ("textureTaps", "meshTextureTaps", "textureTapStats"):
        assert re.search(r"\b%s\s*\(" % m, body), m
    at = body.index("textureTaps(")
    assert "The reference has no counterpart" in body[:at].rsplit("\n  // ----", 1)[1]


def test_adapter_compiles_with_a_textured_mesh(tmp_path):
    src = tmp_path / "use_taps.cpp"
    src.write_text('#include <cstdint>\n'
                   '#include "recon_integration_hip.hpp"\n'
                   '// what travels per frame beside the mesh: 16 * N bytes per vertex\n'
                   'std::size_t textured_mesh(kinect::ReconIntegrationHip& recon, std::vector<unsigned char>& wire) {\n'
                   '  kinect::ReconIntegrationHip::TextureTaps t;\n'
                   '  recon.meshTextureTaps(t, true);\n'
                   '  wire.assign((const unsigned char*)t.taps.data(), (const unsigned char*)(t.taps.data() + t.taps.size()));\n'
                   '  const kinect::ReconIntegrationHip::TextureTapStats s = recon.textureTapStats();\n'
                   '  return (std::size_t)(s.points * s.streams - s.not_evaluated) + t.sensor.size();\n'
                   '}\n'
                   'float best_stream(kinect::ReconIntegrationHip& recon, float x, float y, float z) {\n'
                   '  kinect::ReconIntegrationHip::TextureTaps t;\n'
                   '  recon.textureTaps(std::vector<float>{x, y, z}, t);\n'
                   '  float best = -1.0f;\n'
                   '  for (tsdf_texture_tap const& k : t.taps) if (k.dist >= 0.0f && k.quality > best) best = k.quality;\n'
                   '  recon.textureTaps(std::vector<float>{0.5f, 0.5f, 0.5f}, t, true, true);\n'
                   '  return best + t.sensor[0].depth;\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + HOST, str(src)])


def test_kernel_file_is_built_into_the_library():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "k_texture_taps.o" in mk and os.path.exists(os.path.join(CSRC, "k_texture_taps.hip"))
    assert "texture_taps.hpp" in mk and os.path.exists(os.path.join(CSRC, "texture_taps.hpp"))
