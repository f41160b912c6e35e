"""CPU: the entries of the mesh components on Z-slab contexts (tsdf_mesh_slab_components, _component_seam, _link_components, _download_components,
_component_stats and the host merge tsdf_mesh_merge_component_seams) are declared and exported, their records have the sizes the header states, the
calls that need no device fail the way it says, the header states the definition, the binding, the adapter, the driver and the timing tool have their
parts, and the kernels live in a file of their own that the Makefile builds."""
import ctypes as C
import inspect
import os
import re
import subprocess
from importlib import import_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "rgbd-recon_amd", "host")
CSRC = os.path.join(ROOT, "rgbd-recon_amd", "csrc")
NAMES = ["tsdf_mesh_slab_components", "tsdf_mesh_slab_component_seam", "tsdf_mesh_merge_component_seams", "tsdf_mesh_slab_link_components",
         "tsdf_mesh_slab_download_components", "tsdf_mesh_slab_component_stats"]


def test_entries_are_declared_and_exported(rr):
    syms = rr.declared_symbols()
    lib = rr.load_library()
    for name in NAMES:
        assert name in syms and hasattr(lib, name), name
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", open(rr.HEADER_PATH).read(), flags=re.S))
    for decl in ("int32_t tsdf_mesh_slab_components(tsdf_ctx* ctx, uint64_t out[4]);",
                 "int32_t tsdf_mesh_slab_component_seam(tsdf_ctx* ctx, tsdf_mesh_seam_vertex* down, tsdf_mesh_seam_vertex* up, tsdf_mesh_seam_root* roots);",
                 "int32_t tsdf_mesh_merge_component_seams(const tsdf_mesh_component_seams* slabs, uint32_t n_slabs, uint64_t* component_base, "
                 "tsdf_mesh_component_link* links, uint64_t* n_components);",
                 "int32_t tsdf_mesh_slab_link_components(tsdf_ctx* ctx, uint64_t component_base, const tsdf_mesh_component_link* links, uint64_t n_links, uint64_t* n_owned);",
                 "int32_t tsdf_mesh_slab_download_components(tsdf_ctx* ctx, uint32_t* vertex_component, uint32_t* triangle_component, tsdf_mesh_component* table);",
                 "int32_t tsdf_mesh_slab_component_stats(tsdf_ctx* ctx, uint64_t out[4]);"):
        assert decl in flat, decl


def test_record_sizes(rr, tmp_path):
    assert rr.MESH_SEAM_VERTEX_DTYPE.itemsize == 8 and rr.MESH_SEAM_ROOT_DTYPE.itemsize == 16 and rr.MESH_COMPONENT_LINK_DTYPE.itemsize == 32
    assert C.sizeof(rr.MeshComponentSeams) == 72
    assert rr.MESH_COMPONENT_LINK_DTYPE.names == ("root", "final_root", "component", "reserved0", "n_vertices", "n_triangles", "reserved1", "reserved2")
    src = tmp_path / "sizes.c"                                            # ... and the C header agrees, as C
    src.write_text('#include "rgbd_recon_hip.h"\n'
                   '_Static_assert(sizeof(tsdf_mesh_seam_vertex) == 8 && sizeof(tsdf_mesh_seam_root) == 16 && sizeof(tsdf_mesh_component_link) == 32, "records");\n'
                   '_Static_assert(sizeof(tsdf_mesh_component_seams) == 72, "the merge\'s input");\n')
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_entries_reject_a_null_context(rr):
    lib = rr.load_library()
    out = (C.c_uint64 * 4)(7, 7, 7, 7)
    n = C.c_uint64(7)
    assert lib.tsdf_mesh_slab_components(None, out) == -1
    assert lib.tsdf_mesh_slab_component_seam(None, None, None, None) == -1
    assert lib.tsdf_mesh_slab_link_components(None, C.c_uint64(0), None, C.c_uint64(0), C.byref(n)) == -1
    assert lib.tsdf_mesh_slab_download_components(None, None, None, None) == -1
    assert lib.tsdf_mesh_slab_component_stats(None, out) == -1
    assert list(out) == [7, 7, 7, 7] and n.value == 7


def test_header_states_the_definition(rr):
    text = open(rr.HEADER_PATH).read()
    doc = text[text.index("mesh components on Z-slab contexts: part labels"):text.index("typedef struct tsdf_mesh_seam_vertex")]
    for words in ("GLOBAL component numbers", "WHOLE\n *          component's counts", "byte for byte", "one-slab case", "Every triangle of a part has an own vertex",
                  "corner 0 of its cell is in every Kuhn tetrahedron", "larger than own indices", "through\n *   another slab only", "transitive\n *   over all seams",
                  "no float anywhere", "arrival order decides nothing", "only when slab_z0 > 0", "plane 0 of the first owned lattice tile layer", "ascending by vertex",
                  "ascending by root", "8 bytes", "16 bytes", "(32 bytes)", "pure host function", "the smaller root on top", "component_base + rank - (removed roots",
                  "an up record without its down\n *   record", "not strictly ascending", "a root outside its slab", "a bad index never reaches a\n *   scatter",
                  "final_root <= root", "another exported root of this slab", "the state untouched", "\"mesh_slab_components\"", "\"mesh_slab_components_link\"",
                  "by a new tsdf_mesh_slab_link", "launches nothing and answers zeros", "NULL links with n_links > 0", "TSDF_ERR_OUT_OF_MEMORY leaves",
                  "tsdf_mesh_components keeps answering TSDF_ERR_STATE", "Filtering the parts themselves", "Filtered part rings", "native RCCL exchange",
                  "tests/mesh_slab_component_reference.py", "No counterpart"):
        assert words in doc, words
    # the two older sections no longer send the caller to the host for this
    assert "label that one" not in text and "run them where the concatenated mesh is" not in text


def test_python_binding_and_driver_have_the_methods(rr):
    H = rr.ReconIntegrationHip
    for name in ("mesh_slab_components", "mesh_slab_component_seam", "mesh_slab_link_components", "mesh_slab_download_components", "mesh_slab_component_stats"):
        assert callable(getattr(H, name)), name
    assert list(inspect.signature(H.mesh_slab_link_components).parameters)[1:] == ["component_base", "links"]
    assert list(inspect.signature(rr.merge_mesh_component_seams).parameters) == ["slabs", "native"]
    assert list(inspect.signature(rr.drop_mesh_components).parameters) == ["mesh", "vertex_component", "triangle_component", "keep"]
    mgpu = import_module("rgbd-recon_amd.multigpu")
    assert list(inspect.signature(mgpu.SlabDriver.mesh_components).parameters) == ["self"]
    assert list(inspect.signature(mgpu.mesh_components_on_one_device).parameters)[0] == "backends"


def test_binding_makes_no_buffer_without_labels(rr):
    """without the sizes of a successful step 1 the binding refuses itself: it has no buffer of the right size to hand to the library"""
    import pytest
    hip = object.__new__(rr.ReconIntegrationHip)                         # (no context: the methods must not get as far as the library)
    hip._c = None
    for state in ("absent", None):
        if state is None:
            hip._mesh_slab, hip._mesh_slab_cc = (3, 1, (1, 1)), None     # what a link leaves
        for call in (hip.mesh_slab_component_seam, hip.mesh_slab_download_components, lambda: hip.mesh_slab_link_components(0, [])):
            with pytest.raises(rr.TsdfError) as e:
                call()
            assert e.value.code == -4
    hip._mesh_slab_cc = dict(local_components=1, down=0, up=0, roots=0, owned=None)   # labelled, not linked: no table size yet
    with pytest.raises(rr.TsdfError) as e:
        hip.mesh_slab_download_components()
    assert e.value.code == -4


def test_adapter_methods_compile(tmp_path):
    src = tmp_path / "use_slab_components.cpp"
    src.write_text('#include <cstdint>\n#include <vector>\n'
                   '#include "recon_integration_hip.hpp"\n'
                   'using R = kinect::ReconIntegrationHip;\n'
                   'std::uint64_t slab_components(R& recon, std::uint64_t below, std::uint64_t vertices) {\n'
                   '  const R::MeshSlabComponentCounts n = recon.meshSlabComponents();\n'
                   '  R::MeshSlabSeams mine;\n'
                   '  mine.vertex_base = below; mine.n_vertices = vertices; mine.n_local = n.local_components;\n'
                   '  recon.meshSlabComponentSeam(mine.lists);\n'
                   '  const R::MergedMeshComponents m = R::mergeMeshComponentSeams({mine});\n'
                   '  const std::uint64_t owned = recon.linkMeshSlabComponents(m.component_base[0], m.links[0]);\n'
                   '  R::MeshComponents part;\n'
                   '  recon.downloadMeshSlabComponents(part);\n'
                   '  return owned + m.components + part.table.size() + n.down + n.up + n.roots + mine.lists.roots.size();\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + HOST, str(src)])
    text = open(os.path.join(HOST, "recon_integration_hip.hpp")).read()
    at = text.index("meshSlabComponents()")
    assert "The reference has no counterpart" in text[text.rindex("// ----", 0, at):at]


def test_kernels_have_a_file_of_their_own_that_the_makefile_builds():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "k_mesh_slab_components.o" in mk and "mesh_cc_seams.hpp" in mk
    src = open(os.path.join(CSRC, "k_mesh_slab_components.hip")).read()
    for name in ("k_sc_hook", "k_sc_mark_down", "k_sc_scatter_links", "k_sc_vertex_component", "k_sc_triangle_component", "cc_hook_chunk", "cc_run_add<4>", "block_exclusive_sum"):
        assert name in src, name
    for name in ("k_mesh_slab.hip", "k_mesh.hip"):                       # the extraction's files hold none of it
        assert "k_sc_" not in open(os.path.join(CSRC, name)).read(), name
    seams = open(os.path.join(CSRC, "mesh_cc_seams.hpp")).read()          # the merge's text is free of HIP
    assert "hip/" not in seams and "__device__" not in seams and "merge_component_seams" in seams and "component_links_check" in seams


def test_timing_tool_has_the_components_option():
    text = open(os.path.join(ROOT, "tools", "mesh_timing.py")).read()
    assert "--components" in text and "mesh_slab_components_link" in text and "merge_mesh_component_seams" in text and "identical_to_whole_volume" in text
