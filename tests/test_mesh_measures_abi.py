"""CPU: the mesh component measure entries (tsdf_mesh_component_measures / _download_component_measures / _measure_grid_info /
_filter_components_measured) are declared and exported, a NULL context is an error code, the header states the definition and what is out of scope in a
section behind the existing mesh sections, the Python binding and the C++ adapter have the calls, a snippet that filters by size through the adapter
compiles, and the Makefile builds the new kernel file."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "rgbd-recon_amd", "host")
CSRC = os.path.join(ROOT, "rgbd-recon_amd", "csrc")
NAMES = ["tsdf_mesh_component_measures", "tsdf_mesh_download_component_measures", "tsdf_mesh_measure_grid_info", "tsdf_mesh_filter_components_measured"]


def test_measure_entries_are_declared_and_exported(rr):
    syms = rr.declared_symbols()
    lib = rr.load_library()
    for name in NAMES:
        assert name in syms, name
        assert hasattr(lib, name), name


def test_measure_entries_reject_a_null_context(rr):
    lib = rr.load_library()
    grid, rows, rule = (C.c_uint8 * 24)(), (C.c_uint8 * 80)(), (C.c_uint8 * 32)()
    assert lib.tsdf_mesh_component_measures(None, grid) == -1 and lib.tsdf_mesh_component_measures(None, None) == -1
    assert lib.tsdf_mesh_download_component_measures(None, rows) == -1
    assert lib.tsdf_mesh_measure_grid_info(None, grid) == -1
    assert lib.tsdf_mesh_filter_components_measured(None, rule, None, None) == -1


def test_header_states_the_definition_and_what_is_out_of_scope(rr):
    text = open(rr.HEADER_PATH).read()
    start = text.index("mesh component measures: exact area, volume and bounds per island")
    doc = text[start:text.index("typedef struct tsdf_mesh_component_measure")]
    # behind the existing mesh sections: the first tsdf_mesh_component typedef of the file is still the table entry's
    assert text.index("typedef struct tsdf_mesh_component ") < text.index("mesh streaming: texture taps in the frame") < start
    assert text[text.index("typedef struct tsdf_mesh_component"):].startswith("typedef struct tsdf_mesh_component {")
    for cite in ("ext = bbox_max - bbox_min in fp32", "vol_to_world", "scale = 1048576.0 / (double) E", "unit = 1.0 / scale", "isotropic",
                 "q = rint(d * scale)", "half-way cases to even", "clamped to\n *   [0, 1048576]", "NaN gives 0", "none contracted", "qx | qy << 21 | qz << 42",
                 "e1 = q1 - q0", "c = e1 x e2", "below 2^43", "below 2^88", "a2 = floor(sqrt(n2))", "v6 = det(q0, q1, q2)", "|v6| < 2^63", "80 bytes",
                 "two's-complement 128-bit", "sum_q / n_vertices", "area2 = 0 and volume6 = 0", "normals point into empty space", "volume6 > 0", "volume6 < 0",
                 "OPEN component volume6 depends on the origin", "area2 * unit^2 / 2", "volume6 * unit^3 / 6", "origin + q * unit", "Why 20 bits", "2.1 um",
                 "identical bytes", "\"mesh_component_measures\"", "\"mesh_filter\"", "allocates before it replaces anything", "TSDF_ERR_OUT_OF_MEMORY leaves",
                 "every clause", "min_extent", "min_abs_volume6", "TSDF_MESH_RULE_POSITIVE_VOLUME", "all-zero rule keeps everything", "reserved != 0",
                 "unknown flag", "Z-slab", "keeps its four words", "runs exactly what it ran before", "streamed filter ring", "Area-weighted centroids",
                 "Welding", "tests/mesh_measure_reference.py", "No counterpart"):
        assert cite in doc, cite
    old = text[text.index("mesh components: label the mesh's islands"):text.index("typedef struct tsdf_mesh_component")]
    assert "area, volume, bounding box" in old and "mesh component measures" in old      # the old section points here


def test_python_binding_has_the_measure_calls(rr):
    H = rr.ReconIntegrationHip
    for name in ("mesh_component_measures", "mesh_download_component_measures", "mesh_measure_rule", "mesh_filter_measured", "mesh_measure_grid"):
        assert callable(getattr(H, name)), name
    assert callable(rr.mesh_measures_si) and callable(rr.mesh_measure_rule_for) and rr.MESH_COMPONENT_MEASURE_DTYPE.itemsize == 80


def test_rule_thresholds_round_up_and_refuse_what_the_fields_cannot_hold(rr):
    import pytest
    u = 2.098083541568485e-06                                             # the default box's unit
    r = rr.mesh_measure_rule_for(u, min_triangles=7, min_extent_m=0.05, min_area_m2=0.05, min_volume_m3=1e-4, positive_volume=True)
    assert r.dtype == rr.MESH_MEASURE_RULE_DTYPE and int(r["min_triangles"]) == 7 and int(r["min_extent"]) == 23832 and int(r["flags"]) == 1 and int(r["reserved"]) == 0
    assert (int(r["min_extent"]) - 1) * u < 0.05 <= int(r["min_extent"]) * u
    assert (int(r["min_area2"]) - 1) * u * u / 2 < 0.05 <= int(r["min_area2"]) * u * u / 2 * (1 + 1e-15)
    assert (int(r["min_abs_volume6"]) - 1) * u ** 3 / 6 < 1e-4 <= int(r["min_abs_volume6"]) * u ** 3 / 6 * (1 + 1e-15)
    zero = rr.mesh_measure_rule_for(u)
    assert all(int(zero[k]) == 0 for k in zero.dtype.names)
    assert int(rr.mesh_measure_rule_for(u, min_volume_m3=27.0)["min_abs_volume6"]) > 1 << 63      # the largest volumes still fit ...
    for kw in (dict(min_volume_m3=30.0), dict(min_extent_m=1e4), dict(min_area_m2=-1.0), dict(min_extent_m=float("nan")), dict(min_triangles=1 << 32)):
        with pytest.raises(ValueError, match=next(iter(kw))):                                     # ... and what does not is named, not wrapped
            rr.mesh_measure_rule_for(u, **kw)


def test_adapter_has_the_measure_calls_and_says_the_reference_has_none():
    text = open(os.path.join(HOST, "recon_integration_hip.hpp")).read()
    body = text[text.index("class ReconIntegrationHip"):]
    body = body[:body.index("\n};")]
    for m in ("meshComponentMeasures", "downloadMeshComponentMeasures", "filterMeshComponentsMeasured", "meshMeasureGrid"):
        assert re.search(r"\b%s\s*\(" % m, body), m
    at = body.index("meshComponentMeasures(")
    assert "The reference has no counterpart" in body[:at].rsplit("\n  // ----", 1)[1]


def test_adapter_compiles_with_a_size_filter(tmp_path):
    src = tmp_path / "by_size.cpp"
    src.write_text('#include <cmath>\n#include <cstdint>\n'
                   '#include "recon_integration_hip.hpp"\n'
                   '// drop everything smaller than 5 cm and every closed void; report the subject\'s surface in m^2\n'
                   'double subject_area(kinect::ReconIntegrationHip& recon) {\n'
                   '  recon.extractMesh(false, false);\n'
                   '  if (recon.meshComponents() == 0) return 0.0;\n'
                   '  const tsdf_mesh_measure_grid g = recon.meshComponentMeasures();\n'
                   '  tsdf_mesh_measure_rule rule{};\n'
                   '  rule.min_extent = (std::uint32_t)std::ceil(0.05 / g.unit);\n'
                   '  rule.flags = TSDF_MESH_RULE_POSITIVE_VOLUME;\n'
                   '  recon.filterMeshComponentsMeasured(rule);\n'
                   '  recon.meshComponents();\n'
                   '  recon.meshComponentMeasures();\n'
                   '  std::vector<tsdf_mesh_component_measure> rows;\n'
                   '  recon.downloadMeshComponentMeasures(rows);\n'
                   '  double area = 0.0;\n'
                   '  for (tsdf_mesh_component_measure const& r : rows) area += (double)r.area2 * g.unit * g.unit / 2.0 + (double)(r.reserved + r.q_min[0] - r.q_min[0]);\n'
                   '  return area + (recon.meshMeasureGrid().bits == 20u ? 0.0 : 1.0);\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + HOST, str(src)])


def test_kernel_file_is_built_into_the_library():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "k_mesh_component_measures.o" in mk and os.path.exists(os.path.join(CSRC, "k_mesh_component_measures.hip"))
    assert "mesh_measure.hpp" in mk and os.path.exists(os.path.join(CSRC, "mesh_measure.hpp"))
    assert "-ffp-contract=off" in mk                                       # the three double operations of a coordinate round one by one
    kernel = open(os.path.join(CSRC, "k_mesh_component_measures.hip")).read()
    assert '#include "mesh_measure.hpp"' in kernel and "atomicCAS" not in kernel and "float" not in kernel.split("namespace rr {", 1)[1].replace("const float*", "")
