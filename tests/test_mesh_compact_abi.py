"""CPU: the compact mesh stream's entries (tsdf_mesh_stream_config_compact / _index_format / _frame_compact) are declared and exported, tsdf_mesh_compact
and the 16-byte tile row agree between a C99 compile and the ctypes mirror, tsdf_mesh_frame is still 112 bytes, a NULL context and a NULL out are error
codes, the header's section states the decode rule and the two bounds, and the Python binding, the C++ adapter (compiled) and the harness option exist."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "rgbd-recon_amd", "host")
NAMES = ["tsdf_mesh_stream_config_compact", "tsdf_mesh_stream_index_format", "tsdf_mesh_stream_frame_compact"]


def test_compact_entries_are_declared_and_exported(rr):
    syms = rr.declared_symbols()
    lib = rr.load_library()
    for name in NAMES:
        assert name in syms, name
        assert hasattr(lib, name), name


def test_structs_agree_with_a_c99_compile_and_the_ctypes_mirror(rr, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rgbd_recon_hip.h"\n'
                   '_Static_assert(sizeof(tsdf_mesh_frame) == 112, "the frame keeps its layout");\n'
                   '_Static_assert(sizeof(tsdf_mesh_tile_row) == 16, "a table row is 16 bytes");\n'
                   '_Static_assert(TSDF_MESH_INDEX_U32 == 0u && TSDF_MESH_INDEX_TILE16 == 1u, "the two formats");\n'
                   'int main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(tsdf_mesh_compact), offsetof(tsdf_mesh_compact, table), offsetof(tsdf_mesh_compact, triangles),\n'
                   '         offsetof(tsdf_mesh_compact, n_tile_rows), offsetof(tsdf_mesh_compact, tiles), offsetof(tsdf_mesh_compact, level));\n'
                   '  printf("%zu %zu %zu %zu\\n", offsetof(tsdf_mesh_tile_row, tile), offsetof(tsdf_mesh_tile_row, first_vertex),\n'
                   '         offsetof(tsdf_mesh_tile_row, first_triangle), offsetof(tsdf_mesh_tile_row, n_triangles));\n'
                   '  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.dirname(rr.HEADER_PATH), str(src), "-o", exe])
    compact, row = (tuple(int(x) for x in line.split()) for line in subprocess.check_output([exe], text=True).splitlines())
    M = rr.MeshCompact
    assert compact == (C.sizeof(M), M.table.offset, M.triangles.offset, M.n_tile_rows.offset, M.tiles.offset, M.level.offset) == (40, 0, 8, 16, 24, 36)
    D = rr.MESH_TILE_ROW_DTYPE
    assert D.itemsize == 16 and row == tuple(D.fields[n][1] for n in ("tile", "first_vertex", "first_triangle", "n_triangles")) == (0, 4, 8, 12)
    assert C.sizeof(rr.MeshFrame) == 112
    assert (rr.MESH_INDEX_U32, rr.MESH_INDEX_TILE16) == (0, 1)


def test_compact_entries_reject_a_null_context_and_a_null_out(rr):
    lib = rr.load_library()
    u, fmt, out = C.c_uint32, C.c_uint32(), rr.MeshCompact()
    assert lib.tsdf_mesh_stream_config_compact(None, u(0), u(0), u(0), u(1), u(1), u(1), u(1), u(3)) == -1
    assert lib.tsdf_mesh_stream_index_format(None, C.byref(fmt)) == -1
    assert lib.tsdf_mesh_stream_frame_compact(None, C.byref(out)) == -1
    invalid = int(re.search(r"TSDF_ERR_INVALID_ARGUMENT\s*=\s*(-?\d+)", open(rr.HEADER_PATH).read()).group(1))
    assert invalid == -1                                                 # (a NULL out on a live context: test_gpu_mesh_compact.py)
    assert lib.tsdf_mesh_stream_frame_compact(None, None) == invalid and lib.tsdf_mesh_stream_index_format(None, None) == invalid


def test_header_states_the_format(rr):
    text = open(rr.HEADER_PATH).read()
    assert text.index("mesh streaming: the filtered frame") < text.index("mesh streaming: compact triangles") < text.index("frame read-out: the swap")
    doc = text[text.index("mesh streaming: compact triangles"):text.index("int32_t tsdf_mesh_stream_config_compact")]
    for cite in ("512 * 7 = 3584", "offset < 3584", "A tile with triangles has a row", "contains the cell's origin c0", "no fourth overflow bit",
                 "code 7 never occurs", "padding up to a multiple of 16", "rows of 16 bytes", "rows of 6 bytes", "Little endian", "never the capacity",
                 "ascending by tile", "x fastest", "ceil(ceil(res[a] / s) / 8)", "Bits 0..11", "Bits\n *   12..14: dx + 2 dy + 4 dz", "Bit 15: 0",
                 "owner = rows[r].tile + ((code >> 12) & 1) + ((code >> 13) & 1) * tiles[0] + ((code >> 14) & 1) * tiles[0] * tiles[1];",
                 "if (rows[mid].tile <= owner) lo = mid; else hi = mid;", "index = rows[lo].first_vertex + (code & 0xfff);", "byte for byte",
                 "IS that call", "TSDF_ERR_INVALID_ARGUMENT", "align16(max_vertices * vertex_stride) + max_surface_tiles * 16 + max_triangles * 6", "4 GiB",
                 "keeps its 112 bytes", "`triangles` is NULL", "valid until tsdf_mesh_stream_release", "zero rows", "the compact sizes",
                 "tests/mesh_compact_reference.py", "No\n * counterpart"):
        assert cite in doc, cite
    scope = doc[doc.index("Out of scope:"):]
    for cite in ("tsdf_mesh_download and the PLY", "slab parts", "texture taps in the ring", "vertex packing", "entropy coding"):
        assert cite in scope, cite


def test_python_binding_has_the_compact_calls(rr):
    H = rr.ReconIntegrationHip
    for name in ("mesh_stream_index_format", "mesh_stream_frame_compact"):
        assert callable(getattr(H, name)), name
    p = inspect.signature(H.mesh_stream_config).parameters
    assert "index_format" in p and p["index_format"].default == 0
    # the decoder on a hand-made frame: two tiles side by side in a 2 x 1 x 1 grid, the second triangle reaches into the +x tile
    table = np.array([(0, 0, 0, 2), (1, 5, 2, 1)], rr.MESH_TILE_ROW_DTYPE)
    codes = np.array([[0, 1, 4], [2, 0x1000 | 0, 0x1000 | 3], [1, 2, 0]], np.uint16)
    assert rr.unpack_mesh_triangles(table, codes, (2, 1, 1)).tolist() == [[0, 1, 4], [2, 5, 8], [6, 7, 5]]
    assert rr.unpack_mesh_triangles(table[:0], codes[:0], (2, 1, 1)).shape == (0, 3)


def test_adapter_has_the_compact_calls_and_compiles(tmp_path):
    text = open(os.path.join(HOST, "recon_integration_hip.hpp")).read()
    body = text[text.index("class ReconIntegrationHip"):]
    body = body[:body.index("\n};")]
    for m in ("meshStreamIndexFormat", "meshFrameCompact", "decodeMeshTriangles"):
        assert re.search(r"\b%s\s*\(" % m, body), m
    assert "tsdf_mesh_stream_config_compact" in body and re.search(r"static std::vector<std::uint32_t> decodeMeshTriangles", body)
    src = tmp_path / "use_compact_stream.cpp"
    src.write_text('#include <cstdint>\n#include <vector>\n'
                   '#include "recon_integration_hip.hpp"\n'
                   '// stream 6-byte triangles, restore the uint32 indices on the host\n'
                   'std::vector<std::uint32_t> per_frame(kinect::ReconIntegrationHip& recon, std::uint64_t f) {\n'
                   '  if (f == 0) recon.configureMeshStream(false, false, 0u, 0u, TSDF_MESH_INDEX_TILE16, 1u << 20, 1u << 21, 1u << 14, 3u);\n'
                   '  std::vector<std::uint32_t> tri;\n'
                   '  if (recon.meshStreamIndexFormat() != TSDF_MESH_INDEX_TILE16) return tri;\n'
                   '  recon.drawF();\n'
                   '  if (!recon.streamMesh(f)) return tri;\n'
                   '  tsdf_mesh_frame fr;\n'
                   '  if (recon.acquireMeshFrame(fr, false)) {\n'
                   '    const tsdf_mesh_compact c = recon.meshFrameCompact();\n'
                   '    if (!fr.triangles) tri = kinect::ReconIntegrationHip::decodeMeshTriangles(c, fr.n_triangles);\n'
                   '    recon.releaseMeshFrame();\n'
                   '  }\n'
                   '  return tri;\n'
                   '}\n'
                   '// the decoder alone, on a hand-made frame\n'
                   'int main() {\n'
                   '  const tsdf_mesh_tile_row rows[2] = {{0, 0, 0, 2}, {1, 5, 2, 1}};\n'
                   '  const std::uint16_t codes[9] = {0, 1, 4, 2, 0x1000, 0x1003, 1, 2, 0};\n'
                   '  tsdf_mesh_compact c{};\n'
                   '  c.table = rows; c.triangles = codes; c.n_tile_rows = 2; c.tiles[0] = 2; c.tiles[1] = 1; c.tiles[2] = 1;\n'
                   '  const std::vector<std::uint32_t> want = {0, 1, 4, 2, 5, 8, 6, 7, 5};\n'
                   '  return kinect::ReconIntegrationHip::decodeMeshTriangles(c, 3) == want ? 0 : 1;\n'
                   '}\n')
    exe = str(tmp_path / "use_compact_stream")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + HOST, str(src), "-o", exe,
                           "-L" + os.path.join(ROOT, "rgbd-recon_amd"), "-lrgbd_recon_hip", "-Wl,-rpath," + os.path.join(ROOT, "rgbd-recon_amd")])
    assert subprocess.run([exe]).returncode == 0


def test_harness_accepts_the_compact_option(tmp_path):
    exe = str(tmp_path / "frame_harness")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(HOST, "frame_harness.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "rgbd-recon_amd"), "-lrgbd_recon_hip", "-Wl,-rpath," + os.path.join(ROOT, "rgbd-recon_amd")])
    bad = subprocess.run([exe, "--mesh-stream-compacted"], capture_output=True, text=True)
    assert bad.returncode == 1 and "[--mesh-stream-compact]" in bad.stderr
    for extra in ([], ["--mesh-stream-min-triangles", "1"], ["--mesh-level", "1"]):
        p = subprocess.run([exe, "--mesh-stream-compact"] + extra, capture_output=True, text=True)
        assert "usage" not in p.stderr, p.stderr
        if p.returncode == 0:
            assert "5 mesh frames streamed, 5 picked up in order, 0 mismatches" in p.stdout
        else:
            assert p.returncode == 3 and "no HIP device" in p.stderr
