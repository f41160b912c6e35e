"""CPU: the mesh extraction entries (tsdf_mesh_extract / _download / _write_ply / _stats) are declared and exported, a NULL context is an error
code, the Python binding and the C++ adapter have the calls, a snippet that saves a capture through the adapter compiles, the harness knows
--mesh, and the PLY writer's bytes are what the header says."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "rgbd-recon_amd", "host")
NAMES = ["tsdf_mesh_extract", "tsdf_mesh_download", "tsdf_mesh_write_ply", "tsdf_mesh_stats"]


def test_mesh_entries_are_declared_and_exported(rr):
    syms = rr.declared_symbols()
    lib = rr.load_library()
    for name in NAMES:
        assert name in syms, name
        assert hasattr(lib, name), name
    text = open(rr.HEADER_PATH).read()
    for macro, value in (("TSDF_MESH_NORMALS", "1u"), ("TSDF_MESH_COLOURS", "2u")):
        assert re.search(r"#define\s+%s\s+%s\b" % (macro, value), text), macro
    assert (rr.MESH_NORMALS, rr.MESH_COLOURS) == (1, 2)


def test_header_cites_what_the_entries_are_built_on(rr):
    text = open(rr.HEADER_PATH).read()
    doc = text[text.index("mesh extraction"):text.index("#define TSDF_MESH_NORMALS")]
    for cite in ("tsdf_raymarch.fs:96", ":140-149", ":295-330", "recon_integration.cpp:66-72,199", "Z-slab", "no counterpart"):
        assert cite in doc, cite


def test_mesh_entries_reject_a_null_context(rr):
    lib = rr.load_library()
    nv, nt, out = C.c_uint64(), C.c_uint64(), (C.c_uint64 * 4)()
    assert lib.tsdf_mesh_extract(None, C.c_uint32(3), C.byref(nv), C.byref(nt)) != 0
    assert lib.tsdf_mesh_download(None, None, None, None, None) != 0
    assert lib.tsdf_mesh_write_ply(None, b"/dev/null") != 0
    assert lib.tsdf_mesh_stats(None, out) != 0


def test_python_binding_has_the_mesh_calls(rr):
    H = rr.ReconIntegrationHip
    for name in ("extract_mesh", "download_mesh", "write_ply", "mesh_stats"):
        assert callable(getattr(H, name)), name


def test_adapter_has_the_mesh_calls_and_says_the_reference_has_none():
    text = open(os.path.join(HOST, "recon_integration_hip.hpp")).read()
    body = text[text.index("class ReconIntegrationHip"):]
    body = body[:body.index("\n};")]
    for m in ("extractMesh", "downloadMesh", "writeMeshPly"):
        assert re.search(r"\b%s\s*\(" % m, body), m
    at = body.index("extractMesh(")
    assert "The reference has no counterpart" in body[:at].rsplit("\n  // ----", 1)[1]


def test_adapter_compiles_with_a_capture_saved(tmp_path):
    src = tmp_path / "use_mesh.cpp"
    src.write_text('#include <cstdint>\n'
                   '#include "recon_integration_hip.hpp"\n'
                   'std::uint64_t save(kinect::ReconIntegrationHip& recon, const char* path, double* area) {\n'
                   '  const kinect::ReconIntegrationHip::MeshCounts n = recon.extractMesh(true, false);\n'
                   '  kinect::ReconIntegrationHip::Mesh m;\n'
                   '  recon.downloadMesh(m);\n'
                   '  *area = 0.0;\n'
                   '  for (std::size_t t = 0; t + 2 < m.triangles.size(); t += 3) *area += m.position[3 * m.triangles[t]] * m.normal[3 * m.triangles[t + 1]];\n'
                   '  recon.writeMeshPly(path);\n'
                   '  return n.vertices + n.triangles + m.colour.size();\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + HOST, str(src)])


def test_harness_accepts_the_mesh_option(tmp_path):
    exe = str(tmp_path / "frame_harness")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(HOST, "frame_harness.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "rgbd-recon_amd"), "-lrgbd_recon_hip", "-Wl,-rpath," + os.path.join(ROOT, "rgbd-recon_amd")])
    bad = subprocess.run([exe, "--mesh"], capture_output=True, text=True)
    assert bad.returncode == 1 and "--mesh FILE.ply" in bad.stderr               # the usage line
    ply = tmp_path / "harness.ply"
    p = subprocess.run([exe, "--mesh", str(ply)], capture_output=True, text=True)
    assert "usage" not in p.stderr, p.stderr                                     # parsed: the run gets as far as the device
    if p.returncode == 0:
        assert "mesh: 0 vertices, 0 triangles" in p.stdout                       # (the harness scene's TSDF is positive everywhere)
        assert ply.read_bytes().startswith(b"ply\nformat binary_little_endian 1.0\n") and ply.read_bytes().endswith(b"end_header\n")
    else:
        assert p.returncode == 3 and "no HIP device" in p.stderr


def test_kernel_file_is_built_into_the_library():
    mk = open(os.path.join(ROOT, "rgbd-recon_amd", "csrc", "Makefile")).read()
    assert "k_mesh.o" in mk and os.path.exists(os.path.join(ROOT, "rgbd-recon_amd", "csrc", "k_mesh.hip"))
