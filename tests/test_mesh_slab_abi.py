"""CPU: the slab entries of the mesh path (tsdf_mesh_slab_extract, _seam, _link, _download, _stats) are declared and exported, the calls that need no
device fail the way the header says, the header states the definition, the binding, the adapter, the driver and the timing tool have their parts, and
the kernels' private copy of the two tables is k_mesh.hip's."""
import ctypes as C
import inspect
import os
import re
import subprocess
from importlib import import_module

import mesh_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "rgbd-recon_amd", "host")
CSRC = os.path.join(ROOT, "rgbd-recon_amd", "csrc")
NAMES = ["tsdf_mesh_slab_extract", "tsdf_mesh_slab_seam", "tsdf_mesh_slab_link", "tsdf_mesh_slab_download", "tsdf_mesh_slab_stats"]


def test_slab_entries_are_declared_and_exported(rr):
    syms = rr.declared_symbols()
    lib = rr.load_library()
    for name in NAMES:
        assert name in syms and hasattr(lib, name), name
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", open(rr.HEADER_PATH).read(), flags=re.S))
    assert "int32_t tsdf_mesh_slab_extract(tsdf_ctx* ctx, uint32_t flags, uint32_t level, uint64_t* n_vertices, uint64_t* n_triangles);" in flat
    assert "int32_t tsdf_mesh_slab_seam(tsdf_ctx* ctx, uint32_t* out);" in flat
    assert "int32_t tsdf_mesh_slab_link(tsdf_ctx* ctx, uint64_t vertex_base, const uint32_t* above_seam);" in flat
    assert "int32_t tsdf_mesh_slab_download(tsdf_ctx* ctx, float* position_xyz, float* normal_xyz, float* colour_rgba, uint32_t* triangles);" in flat
    assert "int32_t tsdf_mesh_slab_stats(tsdf_ctx* ctx, uint64_t out[4]);" in flat


def test_header_states_the_definition(rr):
    text = open(rr.HEADER_PATH).read()
    doc = text[text.index("mesh extraction on Z-slab contexts"):text.index("int32_t tsdf_mesh_slab_extract")]
    for words in ("concatenation of per-slab parts", "no vertex needs welding", "GLOBAL", "multiple of 8 s", "Level 0 always qualifies", "one-slab case",
                  "voxel planes z1 and z1 + s", "Halo.", "never clamped silently", "vertex_base + n_vertices + above_seam[tile]", "contiguous",
                  "TSDF_ERR_OUT_OF_MEMORY", "rewrites the triangles", "BEFORE it looks at its arguments", "\"mesh_slab_count\", \"mesh_slab_scan\", \"mesh_slab_emit\"", "\"mesh_slab_link\""):
        assert words in doc, words
    assert "welding slab meshes is deliberately out of scope" not in text                     # the old refusals point to the new entries
    assert text.count("tsdf_mesh_slab_extract") >= 4


def test_slab_entries_reject_a_null_context(rr):
    lib = rr.load_library()
    n, out = C.c_uint64(7), (C.c_uint32 * 4)()
    assert lib.tsdf_mesh_slab_extract(None, C.c_uint32(0), C.c_uint32(0), C.byref(n), C.byref(n)) == -1
    assert lib.tsdf_mesh_slab_seam(None, out) == -1
    assert lib.tsdf_mesh_slab_link(None, C.c_uint64(0), None) == -1
    assert lib.tsdf_mesh_slab_download(None, None, None, None, None) == -1
    assert lib.tsdf_mesh_slab_stats(None, (C.c_uint64 * 4)()) == -1
    assert n.value == 7


def test_python_binding_and_driver_have_the_methods(rr):
    H = rr.ReconIntegrationHip
    for name in ("extract_mesh_slab", "mesh_slab_seam", "mesh_slab_link", "mesh_slab_download", "mesh_slab_stats"):
        assert callable(getattr(H, name)), name
    p = inspect.signature(H.extract_mesh_slab).parameters
    assert list(p)[1:] == ["normals", "colours", "level"] and p["level"].default == 0
    assert list(inspect.signature(H.mesh_slab_link).parameters)[1:] == ["vertex_base", "above_seam"]
    mgpu = import_module("rgbd-recon_amd.multigpu")
    assert list(inspect.signature(mgpu.mesh_slabs_on_one_device).parameters) == ["backends", "normals", "colours", "level"]
    assert list(inspect.signature(mgpu.SlabDriver.extract_mesh).parameters)[1:] == ["normals", "colours", "level"]


def test_binding_makes_no_buffer_without_a_part(rr):
    """without the sizes of a successful extract the binding refuses itself: it has no buffer of the right size to hand to the library"""
    import pytest
    hip = object.__new__(rr.ReconIntegrationHip)                         # (no context: the two methods must not get as far as the library)
    hip._c = None
    for state in ("absent", None):
        if state is None:
            hip._mesh_slab = None                                        # what a refused extract_mesh_slab leaves
        for call in (hip.mesh_slab_seam, lambda: hip.mesh_slab_download(False, False)):
            with pytest.raises(rr.TsdfError) as e:
                call()
            assert e.value.code == -4


def test_adapter_methods_compile(tmp_path):
    src = tmp_path / "use_slab_mesh.cpp"
    src.write_text('#include <cstdint>\n#include <vector>\n'
                   '#include "recon_integration_hip.hpp"\n'
                   'std::uint64_t slab_part(kinect::ReconIntegrationHip& recon, std::uint64_t below, const std::vector<std::uint32_t>* above) {\n'
                   '  const kinect::ReconIntegrationHip::MeshCounts n = recon.extractMeshSlab(true, false, 1u);\n'
                   '  std::vector<std::uint32_t> seam;\n'
                   '  recon.meshSlabSeam(seam);\n'
                   '  recon.meshSlabLink(below, above ? above->data() : nullptr);\n'
                   '  kinect::ReconIntegrationHip::Mesh part;\n'
                   '  recon.downloadMeshSlab(part);\n'
                   '  return n.vertices + seam.size() + recon.seamTiles() + recon.meshSlabStats().tiles_with_surface + part.triangles.size();\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + HOST, str(src)])


def test_kernel_file_is_built_and_its_tables_are_the_generated_ones():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "k_mesh_slab.o" in mk and "mesh_dev.hpp" in mk
    src = open(os.path.join(CSRC, "k_mesh_slab.hip")).read()
    m = re.search(r"c_mesh_flip\[6\]\s*=\s*\{([^}]*)\}", src)
    assert m and [int(w, 16) for w in m.group(1).split(",")] == M.winding_table()
    m = re.search(r"c_tet\[6\]\[4\]\s*=\s*\{(.*?)\};", src)
    assert m and tuple(tuple(int(x) for x in g.split(",")) for g in re.findall(r"\{([\d, ]+)\}", m.group(1))) == M.TETS
    for name in ("k_mesh_slab_count", "k_mesh_slab_vertices", "k_mesh_slab_triangles"):
        assert name in src, name
    for name in MESH_SOURCES:                                                                # no atomic decides a position: the bodies are mesh_dev.hpp's
        assert "atomic" not in mesh_code(name), name


MESH_SOURCES = ("mesh_dev.hpp", "k_mesh.hip", "k_mesh_slab.hip")


def mesh_code(name):
    """a mesh source file without its comments"""
    return re.sub(r"//.*", "", open(os.path.join(CSRC, name)).read())


def test_every_mesh_stage_has_one_body_and_the_kernels_are_wrappers():
    """The whole-volume and the slab-part kernels are instantiations of one body per stage (mesh_dev.hpp, on a tile policy).  A stage's identifying
    line stands once in the three files, and a __global__ kernel of the two .hip files is a wrapper of at most six lines -- but for the kernels
    that exist once for both forms and have no body to share: the table, the two headers and the scan's three."""
    text = "".join(mesh_code(name) for name in MESH_SOURCES)
    for line in ("in_layer - t.ty * L.ntx()",                          # the tile of a workgroup
                 "mesh_voxel<kSparse>(V, x << kLevel, y << kLevel, z << kLevel)",   # the corner stage
                 "__syncthreads_or(mixed)",                            # count
                 "p.mask | (p.inside << 7) | (off << 8)",              # the record store
                 "edge[k++] =",                                        # the tile's vertex list
                 "upx + w * (uqx - upx)",                              # a vertex's unit-cube position
                 "corners = ((m & 0x7fu) << 1)",                       # triangles
                 "h.overflow =",                                       # the streamed header
                 "make_uint4(first_tile + (uint32_t)t"):               # the tile table
        assert text.count(line) == 1, (line, text.count(line))
    whole = ("k_mesh_block_sums", "k_mesh_scan_sums", "k_mesh_scan_apply", "k_mesh_stream_table", "k_mesh_stream_header", "k_mesh_part_header")
    seen = []
    for name in ("k_mesh.hip", "k_mesh_slab.hip"):
        src = mesh_code(name)
        for m in re.finditer(r"__global__[^;{]*?\bvoid\s+(k_\w+)\s*\(", src):
            depth, i = 1, m.end()
            while depth:                                               # the end of the argument list ...
                depth += {"(": 1, ")": -1}.get(src[i], 0); i += 1
            start = src.index("{", i)
            depth, i = 1, start + 1
            while depth:                                               # ... and of the body
                depth += {"{": 1, "}": -1}.get(src[i], 0); i += 1
            body = [ln for ln in src[start + 1:i - 1].splitlines() if ln.strip()]
            seen.append(m.group(1))
            assert m.group(1) in whole or len(body) <= 6, (m.group(1), len(body))
    for name in ("k_mesh_count", "k_mesh_vertices", "k_mesh_vertices_packed", "k_mesh_triangles", "k_mesh_triangles_stream", "k_mesh_triangles_stream_compact",
                 "k_mesh_slab_count", "k_mesh_slab_vertices", "k_mesh_slab_triangles", "k_mesh_part_vertices_packed", "k_mesh_part_triangles") + whole:
        assert seen.count(name) == 1, name


def test_timing_tool_has_the_slab_option():
    text = open(os.path.join(ROOT, "tools", "mesh_timing.py")).read()
    assert "--slabs" in text and "mesh_slab_link" in text and "identical_to_whole_volume" in text
