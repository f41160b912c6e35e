"""CPU: the filtered mesh stream's entries (tsdf_mesh_stream_config_filter / _min_triangles / _frame_filter) are declared and exported, a NULL context
and a NULL out are error codes, tsdf_mesh_frame is still 112 bytes, the header states the definition, the Python binding and the C++ adapter have the
calls, a snippet that streams a filtered surface through the adapter compiles, and the harness takes the option."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "rgbd-recon_amd", "host")
CSRC = os.path.join(ROOT, "rgbd-recon_amd", "csrc")
NAMES = ["tsdf_mesh_stream_config_filter", "tsdf_mesh_stream_min_triangles", "tsdf_mesh_stream_frame_filter"]


def test_filter_entries_are_declared_and_exported(rr):
    syms = rr.declared_symbols()
    lib = rr.load_library()
    for name in NAMES:
        assert name in syms, name
        assert hasattr(lib, name), name


def test_filter_entries_reject_a_null_context_and_a_null_out(rr):
    lib = rr.load_library()
    n, out = C.c_uint32(), (C.c_uint64 * 4)()
    u = C.c_uint32
    assert lib.tsdf_mesh_stream_config_filter(None, u(0), u(0), u(100), u(1), u(1), u(1), u(3)) == -1
    assert lib.tsdf_mesh_stream_min_triangles(None, C.byref(n)) == -1
    assert lib.tsdf_mesh_stream_frame_filter(None, out) == -1
    # TSDF_ERR_INVALID_ARGUMENT is -1 as well; a NULL out on a live context is checked where a context exists (test_gpu_mesh_stream_filter.py)
    invalid = int(re.search(r"TSDF_ERR_INVALID_ARGUMENT\s*=\s*(-?\d+)", open(rr.HEADER_PATH).read()).group(1))
    assert invalid == -1
    assert lib.tsdf_mesh_stream_frame_filter(None, None) == invalid and lib.tsdf_mesh_stream_min_triangles(None, None) == invalid


def test_frame_struct_is_still_112_bytes(rr, tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include "rgbd_recon_hip.h"\n_Static_assert(sizeof(tsdf_mesh_frame) == 112, "the frame keeps its layout");\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I" + os.path.dirname(rr.HEADER_PATH), str(src), "-o", str(tmp_path / "size")])
    assert C.sizeof(rr.MeshFrame) == 112


def test_header_states_the_definition(rr):
    text = open(rr.HEADER_PATH).read()
    doc = text[text.index("mesh streaming: the filtered frame"):text.index("int32_t tsdf_mesh_stream_config_filter")]
    for cite in ("min_triangles == 0", "1 keeps every component", "n_triangles < min_triangles", "pack(keep(mesh)) == pack(mesh)[kept]", "112-byte layout",
                 "FILTERED counts", "UNFILTERED", "bound the unfiltered mesh", "zero counts, overflow == 0", "no fourth overflow bit", "components kept",
                 "all four 0 for an overflowed frame", "draw_done", "\"mesh_stream_filter\"", "tests/mesh_stream_filter_reference.py", "No counterpart"):
        assert cite in doc, cite
    comps = text[text.index("mesh components: label the mesh's islands"):text.index("typedef struct tsdf_mesh_component")]
    out_of_scope = comps[comps.index("Out of scope."):]
    assert "streamed ring" not in out_of_scope and "tsdf_mesh_stream" not in out_of_scope


def test_python_binding_has_the_filter_calls(rr):
    H = rr.ReconIntegrationHip
    for name in ("mesh_stream_min_triangles", "mesh_stream_frame_filter"):
        assert callable(getattr(H, name)), name
    p = inspect.signature(H.mesh_stream_config).parameters
    assert "min_triangles" in p and p["min_triangles"].default == 0


def test_adapter_has_the_filter_calls_and_compiles(tmp_path):
    text = open(os.path.join(HOST, "recon_integration_hip.hpp")).read()
    body = text[text.index("class ReconIntegrationHip"):]
    body = body[:body.index("\n};")]
    for m in ("meshStreamMinTriangles", "meshStreamFrameFilter"):
        assert re.search(r"\b%s\s*\(" % m, body), m
    assert "tsdf_mesh_stream_config_filter" in body
    src = tmp_path / "use_filtered_stream.cpp"
    src.write_text('#include <cstdint>\n'
                   '#include "recon_integration_hip.hpp"\n'
                   '// every frame leaves without its blobs of fewer than 200 triangles; bytes sent and triangles the filter saved\n'
                   'std::uint64_t per_frame(kinect::ReconIntegrationHip& recon, std::uint64_t f, std::uint64_t& saved) {\n'
                   '  if (f == 0) recon.configureMeshStream(true, false, 0u, 200u, 1u << 20, 1u << 21, 1u << 14, 3u);\n'
                   '  if (recon.meshStreamMinTriangles() != 200u) return 0;\n'
                   '  recon.drawF();\n'
                   '  std::uint64_t sent = 0;\n'
                   '  if (!recon.streamMesh(f)) return 0;\n'
                   '  tsdf_mesh_frame fr;\n'
                   '  if (recon.acquireMeshFrame(fr, false)) {\n'
                   '    const kinect::ReconIntegrationHip::MeshFrameFilter ff = recon.meshStreamFrameFilter();\n'
                   '    if (!fr.overflow) sent = fr.n_vertices * fr.vertex_stride + fr.n_triangles * 12;\n'
                   '    saved += ff.triangles_removed + ff.vertices_removed + (ff.components - ff.kept);\n'
                   '    recon.releaseMeshFrame();\n'
                   '  }\n'
                   '  return sent;\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + HOST, str(src)])


def test_harness_accepts_the_filter_option(tmp_path):
    exe = str(tmp_path / "frame_harness")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(HOST, "frame_harness.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "rgbd-recon_amd"), "-lrgbd_recon_hip", "-Wl,-rpath," + os.path.join(ROOT, "rgbd-recon_amd")])
    bad = subprocess.run([exe, "--mesh-stream-min-triangles"], capture_output=True, text=True)      # the number is missing
    assert bad.returncode == 1 and "[--mesh-stream-min-triangles N]" in bad.stderr and "[--mesh-stream]" in bad.stderr
    for n in ("1", "100000"):
        p = subprocess.run([exe, "--mesh-stream", "--mesh-stream-min-triangles", n], capture_output=True, text=True)
        assert "usage" not in p.stderr, p.stderr
        if p.returncode == 0:
            assert "5 mesh frames streamed, 5 picked up in order, 0 mismatches" in p.stdout
        else:
            assert p.returncode == 3 and "no HIP device" in p.stderr


def test_kernel_file_is_built_into_the_library():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "k_mesh_stream_filter.o" in mk and os.path.exists(os.path.join(CSRC, "k_mesh_stream_filter.hip"))
    assert "mesh_cc_dev.hpp" in mk and os.path.exists(os.path.join(CSRC, "mesh_cc_dev.hpp"))
