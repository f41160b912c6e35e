"""CPU: the mesh component entries (tsdf_mesh_components / _download_components / _keep_components / _filter_components / _component_stats) are declared
and exported, a NULL context is an error code, the table entry is 16 bytes with the same offsets in C and in the numpy mirrors, the header states the
definition and what is out of scope, the Python binding and the C++ adapter have the calls, and a snippet that cleans a mesh through the adapter compiles."""
import ctypes as C
import os
import re
import subprocess

import mesh_component_reference as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "rgbd-recon_amd", "host")
CSRC = os.path.join(ROOT, "rgbd-recon_amd", "csrc")
NAMES = ["tsdf_mesh_components", "tsdf_mesh_download_components", "tsdf_mesh_keep_components", "tsdf_mesh_filter_components", "tsdf_mesh_component_stats"]


def test_component_entries_are_declared_and_exported(rr):
    syms = rr.declared_symbols()
    lib = rr.load_library()
    for name in NAMES:
        assert name in syms, name
        assert hasattr(lib, name), name


def test_component_entries_reject_a_null_context(rr):
    lib = rr.load_library()
    n, out, keep = C.c_uint64(), (C.c_uint64 * 4)(), (C.c_uint8 * 1)(1)
    assert lib.tsdf_mesh_components(None, C.byref(n)) == -1
    assert lib.tsdf_mesh_download_components(None, None, None, None) == -1
    assert lib.tsdf_mesh_keep_components(None, keep, None, None) == -1
    assert lib.tsdf_mesh_filter_components(None, C.c_uint32(1), None, None) == -1
    assert lib.tsdf_mesh_component_stats(None, out) == -1


def test_table_entry_is_16_bytes_in_c_and_in_the_mirrors(rr, tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rgbd_recon_hip.h"\n'
                   '_Static_assert(sizeof(tsdf_mesh_component) == 16, "16-byte entries");\n'
                   'int main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(tsdf_mesh_component), offsetof(tsdf_mesh_component, first_vertex), offsetof(tsdf_mesh_component, n_vertices),\n'
                   '         offsetof(tsdf_mesh_component, n_triangles), offsetof(tsdf_mesh_component, reserved));\n'
                   '  return 0;\n}\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    assert [int(v) for v in subprocess.check_output([exe], text=True).split()] == [16, 0, 4, 8, 12]
    for dt in (rr.MESH_COMPONENT_DTYPE, K.TABLE):
        assert dt.itemsize == 16 and dt.names == ("first_vertex", "n_vertices", "n_triangles", "reserved")
        assert [dt.fields[name][1] for name in dt.names] == [0, 4, 8, 12]


def test_header_states_the_definition_and_what_is_out_of_scope(rr):
    text = open(rr.HEADER_PATH).read()
    doc = text[text.index("mesh components: label the mesh's islands"):text.index("typedef struct tsdf_mesh_component")]
    for cite in ("by index, never by position", "smallest vertex index", "component 0 contains vertex 0", "used by no triangle", "n_triangles = 0",
                 "all three agree", "16 bytes", "keep[c] != 0", "number of kept vertices before", "bit for bit", "NaN payloads", "winding untouched",
                 "empty mesh", "identical bytes", "any\n * level", "sized exactly", "stats[3]", "tile counts stay", "texture taps", "TSDF_ERR_OUT_OF_MEMORY leaves",
                 "\"mesh_components\"", "\"mesh_filter\"", "NULL keep", "tsdf_mesh_stream", "Z-slab", "Welding by position", "area, volume, bounding box",
                 "runs exactly what it ran before", "tests/mesh_component_reference.py", "No counterpart"):
        assert cite in doc, cite


def test_python_binding_has_the_component_calls(rr):
    H = rr.ReconIntegrationHip
    for name in ("mesh_components", "mesh_download_components", "mesh_keep", "mesh_filter", "mesh_keep_largest", "mesh_component_stats"):
        assert callable(getattr(H, name)), name


def test_adapter_has_the_component_calls_and_says_the_reference_has_none():
    text = open(os.path.join(HOST, "recon_integration_hip.hpp")).read()
    body = text[text.index("class ReconIntegrationHip"):]
    body = body[:body.index("\n};")]
    for m in ("meshComponents", "downloadMeshComponents", "keepMeshComponents", "filterMeshComponents", "keepLargestMeshComponents", "meshComponentStats"):
        assert re.search(r"\b%s\s*\(" % m, body), m
    at = body.index("meshComponents(")
    assert "The reference has no counterpart" in body[:at].rsplit("\n  // ----", 1)[1]


def test_adapter_compiles_with_a_cleaned_mesh(tmp_path):
    src = tmp_path / "clean_mesh.cpp"
    src.write_text('#include <cstdint>\n'
                   '#include "recon_integration_hip.hpp"\n'
                   '// the subject alone: extract, label, keep the largest island, write it\n'
                   'std::uint64_t subject(kinect::ReconIntegrationHip& recon, const char* path) {\n'
                   '  recon.extractMesh(true, true);\n'
                   '  if (recon.meshComponents() == 0) return 0;\n'
                   '  const kinect::ReconIntegrationHip::MeshCounts kept = recon.keepLargestMeshComponents(1);\n'
                   '  recon.writeMeshPly(path);\n'
                   '  return kept.triangles + recon.meshComponentStats().triangles_removed;\n'
                   '}\n'
                   'std::size_t without_floaters(kinect::ReconIntegrationHip& recon, kinect::ReconIntegrationHip::Mesh& out) {\n'
                   '  recon.meshComponents();\n'
                   '  kinect::ReconIntegrationHip::MeshComponents comps;\n'
                   '  recon.downloadMeshComponents(comps);\n'
                   '  std::vector<std::uint8_t> keep;\n'
                   '  for (tsdf_mesh_component const& c : comps.table) keep.push_back(c.n_triangles >= 100u && c.reserved == 0u);\n'
                   '  recon.keepMeshComponents(keep);\n'
                   '  recon.meshComponents();\n'
                   '  recon.filterMeshComponents(200u);\n'
                   '  recon.downloadMesh(out);\n'
                   '  return out.triangles.size() / 3 + comps.vertex_component.size() + comps.triangle_component.size();\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + HOST, str(src)])


def test_kernel_file_is_built_into_the_library():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "k_mesh_components.o" in mk and os.path.exists(os.path.join(CSRC, "k_mesh_components.hip"))
    assert "scan_dev.hpp" in mk and os.path.exists(os.path.join(CSRC, "scan_dev.hpp"))
