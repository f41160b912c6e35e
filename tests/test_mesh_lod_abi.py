"""CPU: the level-of-detail entries of the mesh path (tsdf_mesh_extract_lod, tsdf_mesh_stream_config_lod, tsdf_mesh_stream_level) are declared and
exported, the calls that need no device fail the way the header says, tsdf_mesh_frame kept its size, and the binding, the adapter, the harness and the
timing tools have their parts."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "rgbd-recon_amd", "host")
NAMES = ["tsdf_mesh_extract_lod", "tsdf_mesh_stream_config_lod", "tsdf_mesh_stream_level"]


def test_lod_entries_are_declared_and_exported(rr):
    syms = rr.declared_symbols()
    lib = rr.load_library()
    for name in NAMES:
        assert name in syms, name
        assert hasattr(lib, name), name
    text = re.sub(r"/\*.*?\*/", "", open(rr.HEADER_PATH).read(), flags=re.S)
    flat = re.sub(r"\s+", " ", text)
    assert "int32_t tsdf_mesh_extract_lod(tsdf_ctx* ctx, uint32_t flags, uint32_t level, uint64_t* n_vertices, uint64_t* n_triangles);" in flat
    assert ("int32_t tsdf_mesh_stream_config_lod(tsdf_ctx* ctx, uint32_t flags, uint32_t level, uint32_t max_vertices, uint32_t max_triangles, "
            "uint32_t max_surface_tiles, uint32_t slots);") in flat
    assert "int32_t tsdf_mesh_stream_level(tsdf_ctx* ctx, uint32_t* level);" in flat
    # the level-0 entries keep their signatures
    assert "int32_t tsdf_mesh_extract(tsdf_ctx* ctx, uint32_t flags, uint64_t* n_vertices, uint64_t* n_triangles);" in flat
    assert ("int32_t tsdf_mesh_stream_config(tsdf_ctx* ctx, uint32_t flags, uint32_t max_vertices, uint32_t max_triangles, uint32_t max_surface_tiles, "
            "uint32_t slots);") in flat


def test_header_states_the_definition(rr):
    text = open(rr.HEADER_PATH).read()
    doc = text[text.index("mesh level of detail"):text.index("int32_t tsdf_mesh_extract_lod")]
    for words in ("s = 1 << L", "point sample, not a filter", "cr = ceil(r / s)", "descent to a voxel edge", "bit-identical to a vertex of the level-0 mesh",
                  "vol[::s, ::s, ::s]", "(s + 1)^3", "wholly between lattice", "TSDF_ERR_INVALID_ARGUMENT"):
        assert words in doc, words


def test_lod_entries_reject_a_null_context_and_null_outputs(rr):
    lib = rr.load_library()
    nv, nt, level = C.c_uint64(), C.c_uint64(), C.c_uint32(9)
    for lv in (0, 1, 2, 3):
        assert lib.tsdf_mesh_extract_lod(None, C.c_uint32(0), C.c_uint32(lv), C.byref(nv), C.byref(nt)) == -1
        assert lib.tsdf_mesh_stream_config_lod(None, C.c_uint32(0), C.c_uint32(lv), C.c_uint32(1), C.c_uint32(1), C.c_uint32(1), C.c_uint32(3)) == -1
    assert lib.tsdf_mesh_stream_level(None, C.byref(level)) == -1
    assert lib.tsdf_mesh_stream_level(None, None) == -1
    assert level.value == 9


def test_frame_struct_is_unchanged(rr, tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "rgbd_recon_hip.h"\nint main(void) { printf("%zu\\n", sizeof(tsdf_mesh_frame)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.dirname(rr.HEADER_PATH), str(src), "-o", exe])
    assert int(subprocess.check_output([exe], text=True)) == C.sizeof(rr.MeshFrame) == 112


def test_python_binding_has_the_level(rr):
    H = rr.ReconIntegrationHip
    assert callable(H.mesh_stream_level)
    for name in ("extract_mesh", "mesh_stream_config"):
        p = inspect.signature(getattr(H, name)).parameters
        assert "level" in p and p["level"].default == 0, name


def test_adapter_overloads_compile(tmp_path):
    text = open(os.path.join(HOST, "recon_integration_hip.hpp")).read()
    body = text[text.index("class ReconIntegrationHip"):]
    body = body[:body.index("\n};")]
    assert len(re.findall(r"\bextractMesh\s*\(bool", body)) == 2 and len(re.findall(r"\bvoid configureMeshStream\s*\(", body)) == 2
    assert re.search(r"\bmeshStreamLevel\s*\(", body)
    src = tmp_path / "use_lod.cpp"
    src.write_text('#include <cstdint>\n'
                   '#include "recon_integration_hip.hpp"\n'
                   'std::uint64_t thin_client(kinect::ReconIntegrationHip& recon, std::uint64_t f) {\n'
                   '  const kinect::ReconIntegrationHip::MeshCounts full = recon.extractMesh(true, false);\n'
                   '  const kinect::ReconIntegrationHip::MeshCounts coarse = recon.extractMesh(true, false, 2u);\n'
                   '  recon.configureMeshStream(false, false, 4096, 8192, 64);\n'
                   '  recon.configureMeshStream(false, false, 1u, 4096, 8192, 64, 3);\n'
                   '  if (recon.meshStreamLevel() != 1u || !recon.streamMesh(f)) return 0;\n'
                   '  return full.vertices - coarse.vertices;\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + HOST, str(src)])


def test_harness_accepts_the_level_option(tmp_path):
    exe = str(tmp_path / "frame_harness")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(HOST, "frame_harness.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "rgbd-recon_amd"), "-lrgbd_recon_hip", "-Wl,-rpath," + os.path.join(ROOT, "rgbd-recon_amd")])
    for bad in (["--mesh-level"], ["--mesh-level", "3"], ["--mesh-level", "x"]):
        p = subprocess.run([exe] + bad, capture_output=True, text=True)
        assert p.returncode == 1 and "[--mesh-level 0|1|2]" in p.stderr, bad
    ply = tmp_path / "lod.ply"
    p = subprocess.run([exe, "--mesh-level", "2", "--mesh", str(ply), "--mesh-stream"], capture_output=True, text=True)
    assert "usage" not in p.stderr, p.stderr                                     # parsed: the run gets as far as the device
    if p.returncode == 0:
        assert "mesh: 0 vertices, 0 triangles" in p.stdout and "5 mesh frames streamed, 5 picked up in order, 0 mismatches" in p.stdout
    else:
        assert p.returncode == 3 and "no HIP device" in p.stderr


def test_timing_tools_take_a_level():
    for tool in ("mesh_timing.py", "mesh_stream_timing.py"):
        text = open(os.path.join(ROOT, "tools", tool)).read()
        assert '"--level"' in text and "level=L" in text, tool
