"""CPU: the slab-part entries of the ray queries (tsdf_cast_rays_part / _dev, tsdf_merge_ray_parts_dev) are declared and exported, a NULL context is an
error code, the header states the ownership formula, the part record, the merge rule and the one-slab case, merge_ray_parts passes known answers, and
the binding, the C++ adapter, the slab driver, the timing tool and the kernel file have their parts."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "rgbd-recon_amd", "host")
CSRC = os.path.join(ROOT, "rgbd-recon_amd", "csrc")
NAMES = ["tsdf_cast_rays_part", "tsdf_cast_rays_part_dev", "tsdf_merge_ray_parts_dev"]


def test_part_entries_are_declared_and_exported(rr):
    syms = rr.declared_symbols()
    lib = rr.load_library()
    for name in NAMES:
        assert name in syms, name
        assert hasattr(lib, name), name


def test_part_entries_reject_a_null_context(rr):
    lib = rr.load_library()
    ray, hit = rr.Ray(), rr.RayHit()
    assert lib.tsdf_cast_rays_part(None, C.byref(ray), C.c_uint64(1), C.c_uint32(0), C.byref(hit), None) == -1
    assert lib.tsdf_cast_rays_part_dev(None, C.byref(ray), C.c_uint64(1), C.c_uint32(0), C.byref(hit), None) == -1
    assert lib.tsdf_merge_ray_parts_dev(None, C.byref(hit), None, C.c_uint32(1), C.c_uint64(1), C.c_uint64(1), C.byref(hit), None) == -1


def test_header_states_the_definition(rr):
    text = open(rr.HEADER_PATH).read()
    assert text.index("ray queries: slab parts") > text.index("int32_t tsdf_ray_stats(")       # behind the ray section
    doc = text[text.index("ray queries: slab parts"):text.index("int32_t tsdf_cast_rays_part(")]
    doc = re.sub(r"\s*\n \*\s*", " ", doc)                                # (the comment's line breaks and indents are not part of the sentences)
    for cite in ("fminf(fmaxf(floorf(pos_k.z * (float)rz), 0.0f), (float)(rz - 1))", "plane >> 3", "[own_tz0, own_tz1)", "a NaN z gives plane 0", "exactly once",
                 "first owned sample with dens > 0", "it is -limit", "from the halo", "n_samples = k + 1", "n_samples = max_n, t = -1", "identical on every slab",
                 "smallest n_samples", "no two parts can tie", "part 0's record", "travels with the winner", "smallest k with dens_k > 0", "monotonic",
                 "one contiguous run", "byte for byte", "exchanged", "recomputed", "one-slab case", "rays_part_march", "rays_part_surface",
                 "hits found in THIS part", "stride_records < n", "parts == 0", "tests/ray_part_reference.py"):
        assert cite in doc, cite
    # the ray section keeps its sentences
    ray = text[text.index("ray queries: cast"):text.index("#define TSDF_RAYS_UNIT_CUBE")]
    assert "on a Z-slab context (a ray crosses slabs: cast on a whole-volume context)" in ray


def test_merge_ray_parts_known_answers(rr):
    h = np.zeros((3, 5), rr.RAY_HIT_DTYPE)
    h["t"] = -1
    h["n_samples"] = 9                                                   # every part's miss: max_n
    h[0]["n_samples"][0], h[0]["status"][0] = 5, 1                       # ray 0: parts 0 and 2 hit, the smaller count wins
    h[2]["n_samples"][0], h[2]["status"][0] = 3, 1
    h[1]["n_samples"][1], h[1]["status"][1] = 9, 1                       # ray 1: a hit at the last sample beats the misses with the same count
    h["status"][:, 3] = 2                                                # ray 3: outside on every slab
    h["status"][:, 4], h["n_samples"][:, 4] = 4, 0                       # ray 4: invalid on every slab
    for k in range(3):
        h[k]["pos"] = k + 1
    s = np.zeros((3, 5), rr.RAY_SURFACE_DTYPE)
    for k in range(3):
        s[k]["rgba"] = 10 + k
    merged = rr.merge_ray_parts(list(h))
    assert merged.dtype == rr.RAY_HIT_DTYPE and merged["n_samples"].tolist() == [3, 9, 9, 9, 0] and merged["status"].tolist() == [1, 1, 0, 2, 4]
    assert merged["pos"][:, 0].tolist() == [3, 2, 1, 1, 1]               # part 0's record where no part hit
    merged2, surf = rr.merge_ray_parts([(h[k], s[k]) for k in range(3)])
    assert merged2.tobytes() == merged.tobytes() and surf["rgba"][:, 0].tolist() == [12, 11, 10, 10, 10]
    one = rr.merge_ray_parts([h[1]])                                     # the one-slab case: the part itself
    assert one.tobytes() == h[1].tobytes()
    # ... and the reference's rule gives the same
    import ray_part_reference as P
    assert P.merge(list(h))[0].tobytes() == merged.tobytes()


def test_binding_driver_and_tool_have_their_parts(rr):
    from importlib import import_module
    H = rr.ReconIntegrationHip
    for name in ("cast_rays_part", "cast_rays_part_dev", "merge_ray_parts_dev", "pick_result"):
        assert callable(getattr(H, name)), name
    assert callable(rr.merge_ray_parts)
    m = import_module("rgbd-recon_amd.multigpu")
    assert callable(m.SlabDriver.cast_rays) and callable(m.SlabDriver.pick) and callable(m.rays_slabs_on_one_device)
    tool = open(os.path.join(ROOT, "tools", "ray_timing.py")).read()
    for word in ("--slabs", "cast_rays_part_dev", "merge_ray_parts_dev", "slowest_part_ms", "merge_ms", "in_front_share"):
        assert word in tool, word


def test_adapter_has_the_part_calls_and_they_compile(tmp_path):
    text = open(os.path.join(HOST, "recon_integration_hip.hpp")).read()
    body = text[text.index("class ReconIntegrationHip"):]
    body = body[:body.index("\n};")]
    for m in ("castRaysPart", "mergeRayParts"):
        assert re.search(r"\b%s\s*\(" % m, body), m
    use = tmp_path / "cast_on_slabs.cpp"
    use.write_text('#include "recon_integration_hip.hpp"\n'
                   'using Recon = kinect::ReconIntegrationHip;\n'
                   'void cast_on_slabs(std::vector<Recon*>& slabs, std::vector<tsdf_ray> const& rays, Recon::RayResults& out) {\n'
                   '  std::vector<Recon::RayResults> parts(slabs.size());\n'
                   '  for (std::size_t k = 0; k < slabs.size(); ++k) slabs[k]->castRaysPart(rays, parts[k], true, true);\n'
                   '  Recon::mergeRayParts(parts, out);\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + HOST, str(use)])
    src = tmp_path / "merge_ray_parts.cpp"                               # the merge is plain C++ and calls nothing of the library: run it on known answers
    src.write_text('#include <cstdio>\n'
                   '#include "recon_integration_hip.hpp"\n'
                   'using Recon = kinect::ReconIntegrationHip;\n'
                   'int main() {\n'
                   '  std::vector<Recon::RayResults> parts(3);\n'
                   '  for (int k = 0; k < 3; ++k) {\n'
                   '    parts[k].hits.assign(3, tsdf_ray_hit{});\n'
                   '    parts[k].surface.assign(3, tsdf_ray_surface{});\n'
                   '    for (int i = 0; i < 3; ++i) { parts[k].hits[i].n_samples = 9; parts[k].hits[i].pos[0] = (float)(k + 1); parts[k].surface[i].rgba[0] = (float)(10 + k); }\n'
                   '  }\n'
                   '  parts[0].hits[0].n_samples = 5; parts[0].hits[0].status = TSDF_RAY_HIT;\n'
                   '  parts[2].hits[0].n_samples = 3; parts[2].hits[0].status = TSDF_RAY_HIT;\n'
                   '  parts[1].hits[1].n_samples = 9; parts[1].hits[1].status = TSDF_RAY_HIT;\n'
                   '  Recon::RayResults out;\n'
                   '  Recon::mergeRayParts(parts, out);\n'
                   '  for (int i = 0; i < 3; ++i) std::printf("%u %u %g %g\\n", out.hits[i].n_samples, out.hits[i].status, out.hits[i].pos[0], out.surface[i].rgba[0]);\n'
                   '  return 0;\n'
                   '}\n')
    exe = str(tmp_path / "merge_ray_parts")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + HOST, str(src), "-o", exe])
    rows = subprocess.check_output([exe], text=True).split("\n")[:3]
    assert rows == ["3 1 3 12", "9 1 2 11", "9 0 1 10"]


def test_kernels_have_their_parts():
    text = open(os.path.join(CSRC, "k_rays.hip")).read()
    assert "template <bool kSparse, bool kPart>" in text and "k_rays_merge" in text and "tex3d_tsdf<kSparse, !kPart>" in text
    merge = text[text.index("void k_rays_merge("):text.index("void launch_rays_march(")]
    assert "atomic" not in merge and "__shared__" not in merge
    assert "sample_owned" in open(os.path.join(CSRC, "ray_dev.hpp")).read()
    march = open(os.path.join(CSRC, "k_raymarch.hip")).read()
    assert "bool sample_owned(" not in march and "sample_owned(V, pos.z)" in march       # the draw and the rays share one text
