"""CPU: the ray query entries (tsdf_cast_rays / tsdf_cast_rays_dev / tsdf_view_rays / tsdf_ray_stats) are declared and exported, a NULL context is
an error code, the three records are 32 bytes in C and in the ctypes and numpy mirrors, the header states the definition, the Python binding and the C++
adapter have the calls, and a snippet that picks through the adapter compiles."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "rgbd-recon_amd", "host")
NAMES = ["tsdf_cast_rays", "tsdf_cast_rays_dev", "tsdf_view_rays", "tsdf_ray_stats"]


def test_ray_entries_are_declared_and_exported(rr):
    syms = rr.declared_symbols()
    lib = rr.load_library()
    for name in NAMES:
        assert name in syms, name
        assert hasattr(lib, name), name
    text = open(rr.HEADER_PATH).read()
    for macro, value in (("TSDF_RAYS_UNIT_CUBE", "1u"), ("TSDF_RAY_NORMALS", "2u"), ("TSDF_RAY_COLOURS", "4u"), ("TSDF_RAY_HIT", "1u"), ("TSDF_RAY_OUTSIDE", "2u"),
                         ("TSDF_RAY_INVALID", "4u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (macro, value), text), macro
    assert (rr.RAYS_UNIT_CUBE, rr.RAY_NORMALS, rr.RAY_COLOURS) == (1, 2, 4)
    assert (rr.RAY_HIT, rr.RAY_OUTSIDE, rr.RAY_INVALID) == (1, 2, 4)


def test_ray_entries_reject_a_null_context(rr):
    lib = rr.load_library()
    ray, hit, out = rr.Ray(), rr.RayHit(), (C.c_uint64 * 4)()
    m = (C.c_float * 16)(*([0.0] * 16))
    assert lib.tsdf_cast_rays(None, C.byref(ray), C.c_uint64(1), C.c_uint32(0), C.byref(hit), None) == -1
    assert lib.tsdf_cast_rays_dev(None, C.byref(ray), C.c_uint64(1), C.c_uint32(0), C.byref(hit), None) == -1
    assert lib.tsdf_view_rays(None, m, m, 0, 0, 1, 1, C.byref(ray)) == -1
    assert lib.tsdf_ray_stats(None, out) == -1


def test_records_are_32_bytes_in_c_and_in_the_mirrors(rr, tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rgbd_recon_hip.h"\n'
                   '_Static_assert(sizeof(tsdf_ray) == 32 && sizeof(tsdf_ray_hit) == 32 && sizeof(tsdf_ray_surface) == 32, "32-byte records");\n'
                   'int main(void) {\n'
                   '  printf("%zu %zu %zu %zu\\n", sizeof(tsdf_ray), offsetof(tsdf_ray, t_min), offsetof(tsdf_ray, dir), offsetof(tsdf_ray, t_max));\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(tsdf_ray_hit), offsetof(tsdf_ray_hit, t), offsetof(tsdf_ray_hit, n_samples), offsetof(tsdf_ray_hit, status),\n'
                   '         offsetof(tsdf_ray_hit, pad));\n'
                   '  printf("%zu %zu %zu\\n", sizeof(tsdf_ray_surface), offsetof(tsdf_ray_surface, pad), offsetof(tsdf_ray_surface, rgba));\n'
                   '  return 0;\n}\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    rows = [[int(v) for v in line.split()] for line in subprocess.check_output([exe], text=True).splitlines()]
    R, H, S = rr.Ray, rr.RayHit, rr.RaySurface
    assert rows[0] == [C.sizeof(R), R.t_min.offset, R.dir.offset, R.t_max.offset] == [32, 12, 16, 28]
    assert rows[1] == [C.sizeof(H), H.t.offset, H.n_samples.offset, H.status.offset, H.pad.offset] == [32, 12, 16, 20, 24]
    assert rows[2] == [C.sizeof(S), S.pad.offset, S.rgba.offset] == [32, 12, 16]
    for dt, row in ((rr.RAY_DTYPE, rows[0]), (rr.RAY_HIT_DTYPE, rows[1]), (rr.RAY_SURFACE_DTYPE, rows[2])):
        assert dt.itemsize == 32
        assert [dt.fields[name][1] for name in dt.names[1:]] == row[1:], dt


def test_header_states_the_definition(rr):
    text = open(rr.HEADER_PATH).read()
    doc = text[text.index("ray queries: cast"):text.index("#define TSDF_RAYS_UNIT_CUBE")]
    for cite in ("tsdf_raymarch.fs:363-374", ":62-114", ":140-149", ":295-330", "recon_integration.cpp:66-72", "no counterpart", "Z-slab",
                 "o_u = (o - bbox_min) / e", "d_u = d / e", "per = len / sd", "s_min = t_min * per", "max_n = ceil(|t1 - t_near|)", "prev = -limit",
                 "(pos - step) - step * (prev / (dens - prev))", "chained additions", "skipped or fetched", "bit for bit", "tests/ray_reference.py",
                 "UN-normalised", "rays_march", "rays_surface"):
        assert cite in doc, cite


def test_python_binding_has_the_ray_calls(rr):
    H = rr.ReconIntegrationHip
    for name in ("cast_rays", "cast_rays_dev", "view_rays", "pick", "ray_stats"):
        assert callable(getattr(H, name)), name


def test_adapter_has_the_ray_calls_and_says_the_reference_has_none():
    text = open(os.path.join(HOST, "recon_integration_hip.hpp")).read()
    body = text[text.index("class ReconIntegrationHip"):]
    body = body[:body.index("\n};")]
    for m in ("castRays", "viewRays", "pick", "rayStats"):
        assert re.search(r"\b%s\s*\(" % m, body), m
    at = body.index("castRays(")
    assert "The reference has no counterpart" in body[:at].rsplit("\n  // ----", 1)[1]


def test_adapter_compiles_with_a_pick_and_a_range_sensor(tmp_path):
    src = tmp_path / "use_rays.cpp"
    src.write_text('#include <cstdint>\n'
                   '#include "recon_integration_hip.hpp"\n'
                   'float measure(kinect::ReconIntegrationHip& recon, int x0, int y0, int x1, int y1) {\n'
                   '  const kinect::ReconIntegrationHip::Pick a = recon.pick(x0, y0), b = recon.pick(x1, y1, false);\n'
                   '  if (!a.hit || !b.hit) return -1.0f;\n'
                   '  float d = 0.0f;\n'
                   '  for (int k = 0; k < 3; ++k) d += (a.position[k] - b.position[k]) * (a.position[k] - b.position[k]);\n'
                   '  return d;\n'
                   '}\n'
                   'std::uint64_t range_sensor(kinect::ReconIntegrationHip& recon, std::vector<tsdf_ray> const& beams, std::vector<float>& range) {\n'
                   '  kinect::ReconIntegrationHip::RayResults out;\n'
                   '  recon.castRays(beams, out, true);\n'
                   '  range.clear();\n'
                   '  for (tsdf_ray_hit const& h : out.hits) range.push_back((h.status & TSDF_RAY_HIT) ? h.t : -1.0f);\n'
                   '  std::vector<tsdf_ray> view = recon.viewRays(0, 0, 4, 4);\n'
                   '  recon.castRays(view, out, false, false, true);\n'
                   '  const kinect::ReconIntegrationHip::RayStats s = recon.rayStats();\n'
                   '  return s.rays + s.hits + s.samples + s.fetched + out.surface.size();\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + HOST, str(src)])


def test_kernel_file_is_built_into_the_library():
    mk = open(os.path.join(ROOT, "rgbd-recon_amd", "csrc", "Makefile")).read()
    assert "k_rays.o" in mk and os.path.exists(os.path.join(ROOT, "rgbd-recon_amd", "csrc", "k_rays.hip"))
    for header in ("ray_dev.hpp", "ray_staging.hpp"):
        assert header in mk and os.path.exists(os.path.join(ROOT, "rgbd-recon_amd", "csrc", header))
