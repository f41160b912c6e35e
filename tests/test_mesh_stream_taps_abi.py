"""CPU: the entries of "mesh streaming: texture taps in the frame" (tsdf_mesh_stream_config_taps / _tap_flags / _frame_taps) are declared and exported,
a NULL context is an error code, the packed tap is 8 bytes and tsdf_mesh_taps 24 with the same offsets in C and in the ctypes and numpy mirrors, the
header states the definition, the Python binding, the C++ adapter, the slab driver, the harness and the timing tool have the calls, and the adapter's
unpacking equals numpy's on every binary16 value."""
import ctypes as C
import inspect
import os
import re
import subprocess
from importlib import import_module

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "rgbd-recon_amd", "host")
CSRC = os.path.join(ROOT, "rgbd-recon_amd", "csrc")
NAMES = ["tsdf_mesh_stream_config_taps", "tsdf_mesh_stream_tap_flags", "tsdf_mesh_stream_frame_taps"]


def test_the_three_entries_are_declared_and_exported(rr):
    syms = rr.declared_symbols()
    lib = rr.load_library()
    for name in NAMES:
        assert name in syms, name
        assert hasattr(lib, name), name
    text = open(rr.HEADER_PATH).read()
    assert re.search(r"#define\s+TSDF_MESH_STREAM_TAPS\s+1u\b", text) and rr.MESH_STREAM_TAPS == 1


def test_entries_reject_a_null_context(rr):
    lib = rr.load_library()
    flags, out = C.c_uint32(), rr.MeshTaps()
    assert lib.tsdf_mesh_stream_config_taps(None, C.c_uint32(1)) == -1
    assert lib.tsdf_mesh_stream_tap_flags(None, C.byref(flags)) == -1
    assert lib.tsdf_mesh_stream_frame_taps(None, C.byref(out)) == -1


def test_structures_are_8_and_24_bytes_in_c_and_in_the_mirrors(rr, tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rgbd_recon_hip.h"\n'
                   '_Static_assert(sizeof(tsdf_packed_tap) == 8 && sizeof(tsdf_mesh_taps) == 24, "8- and 24-byte structures");\n'
                   'int main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(tsdf_packed_tap), offsetof(tsdf_packed_tap, u), offsetof(tsdf_packed_tap, v),\n'
                   '         offsetof(tsdf_packed_tap, quality_h), offsetof(tsdf_packed_tap, dist_h));\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(tsdf_mesh_taps), offsetof(tsdf_mesh_taps, taps), offsetof(tsdf_mesh_taps, n_vertices),\n'
                   '         offsetof(tsdf_mesh_taps, n_streams), offsetof(tsdf_mesh_taps, tap_bytes));\n'
                   '  printf("%u %zu\\n", TSDF_MESH_STREAM_TAPS, sizeof(tsdf_mesh_frame));\n'
                   '  return 0;\n}\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    rows = [[int(v) for v in line.split()] for line in subprocess.check_output([exe], text=True).splitlines()]
    P, M = rr.PackedTap, rr.MeshTaps
    assert rows[0] == [C.sizeof(P), P.u.offset, P.v.offset, P.quality_h.offset, P.dist_h.offset] == [8, 0, 2, 4, 6]
    assert rows[1] == [C.sizeof(M), M.taps.offset, M.n_vertices.offset, M.n_streams.offset, M.tap_bytes.offset] == [24, 0, 8, 16, 20]
    assert rows[2] == [1, C.sizeof(rr.MeshFrame)] == [1, 112]             # tsdf_mesh_frame keeps its layout
    dt = rr.PACKED_TAP_DTYPE
    assert dt.itemsize == 8 and dt.names == ("u", "v", "quality_h", "dist_h") and [dt.fields[n][1] for n in dt.names] == [0, 2, 4, 6]
    assert all(dt.fields[n][0] == np.dtype("<u2") for n in dt.names)


def test_header_states_the_definition(rr):
    text = open(rr.HEADER_PATH).read()
    doc = text[text.index("mesh streaming: texture taps in the frame"):text.index("#define TSDF_MESH_STREAM_TAPS")]
    for cite in ("three uint16 codes q", "bytes 0-5", "the RECEIVER reconstructs", "not at the emit kernel's fp32 u", "u_q = (float) q / 65535.0f", "one fp32 division",
                 "final packed rows", "after the filter's scatter", "needs nothing from the emit", "0.5 / 65535", "depth discontinuity", "dist < limit",
                 "37 x 43 x 35", "5 108 vertices", "0.027 / 255", "22.7 / 255", "the branch (alpha) is the same at every", "no per-vertex closeness",
                 "tsdf_mesh_texture_taps states already", "exactly the four values of tsdf_texture_tap", "NEAREST depth", "current at the tsdf_mesh_stream call",
                 "the not-evaluated record cannot occur", "8 bytes, little endian", "(uint16) rint(min(max(x, 0), 1) * 65535.0f)", "half-way cases to even",
                 "NaN coordinate packs as 0", "does not change a LINEAR, CLAMP_TO_EDGE fetch", "IEEE binary16", "round to nearest even", "overflow to +-inf",
                 "subnormals kept", "0x7E00", "astype(float16)", "[n_vertices][N], vertex-major", "8 * N bytes per vertex", "FILTERED vertices",
                 "join by concatenation", "u = code / 65535.0f", "blend_from_taps", "behind the payload's CAPACITY", "align16(", "max_vertices * N * 8",
                 "a copy of its own", "n_vertices * N * 8", "tsdf_mesh_frame do not change", "4 GiB", "resets it to off", "drops slots", "whatever the vertex flags",
                 "never waits for the host", "overflowed or is empty has no tap bytes", "Z-slab context through a part ring", "exactly the launches and copies it queued before",
                 "valid until the release", "taps is non-NULL and n_vertices 0", "out[2] counts the tap bytes copied", "out[3] the larger slots", "\"mesh_stream_taps\"",
                 "TSDF_ERR_STATE before any config", "any other bit", "the flag stays as it was", "no frame is held or the ring has", "tests/mesh_tap_pack_reference.py"):
        assert cite in doc, cite
    assert doc.index("The point.") < doc.index("tsdf_mesh_stream_config_taps amends") < doc.index("Errors.")   # the definition, the entries, the errors


def test_python_binding_has_the_calls(rr):
    H = rr.ReconIntegrationHip
    for name in ("mesh_stream_config_taps", "mesh_stream_tap_flags", "mesh_stream_frame_taps"):
        assert callable(getattr(H, name)), name
    assert inspect.signature(H.mesh_stream_config).parameters["taps"].default is False
    packed = np.zeros((2, 3), rr.PACKED_TAP_DTYPE)
    packed["u"], packed["v"], packed["quality_h"], packed["dist_h"] = 65535, 13107, 0x3800, 0x0001
    packed[1, 1] = (0, 1, 0x7E00, 0xFC00)
    un = rr.unpack_mesh_taps(packed)
    assert un.dtype == rr.TEXTURE_TAP_DTYPE and un.shape == (2, 3)
    assert un["u"][0, 0] == 1.0 and un["v"][0, 0] == np.float32(13107) / np.float32(65535.0) and un["quality"][0, 0] == 0.5 and un["dist"][0, 0] == 2.0 ** -24
    assert un["u"][1, 1] == 0 and np.isnan(un["quality"][1, 1]) and un["dist"][1, 1] == -np.inf
    # join_mesh_parts concatenates the parts' tap blocks when every part has one
    row = np.zeros(1, rr.MESH_TILE_ROW_DTYPE)
    info = lambda l0, l1, taps: dict(overflow=0, vertex_stride=8, compact=dict(level=0, tiles=(1, 1, 2), table=row), part=dict(layers=(l0, l1), level=0, top=l1 == 2, seam_tiles=0),
                                     **({"taps": taps} if taps is not None else {}))
    v, c = np.zeros((2, 4), np.uint16), np.zeros((1, 3), np.uint16)
    joined = rr.join_mesh_parts([(v, c, info(0, 1, packed)), (v[:0], c[:0], info(1, 2, packed[:0]))])
    assert joined[2]["taps"].tobytes() == packed.tobytes() and joined[2]["taps"].shape == (2, 3)
    assert "taps" not in rr.join_mesh_parts([(v, c, info(0, 1, packed)), (v, c, info(1, 2, None))])[2]


def test_slab_driver_tool_and_harness_carry_the_taps():
    m = import_module("rgbd-recon_amd.multigpu")
    assert "taps" in inspect.getdoc(m.SlabDriver.stream_mesh) and "taps" in inspect.getdoc(m.mesh_parts_on_one_device)
    tool = open(os.path.join(ROOT, "tools", "mesh_stream_timing.py")).read()
    assert '"--taps"' in tool and "mesh_stream_taps" in tool
    harness = open(os.path.join(HOST, "frame_harness.cpp")).read()
    assert "--mesh-stream-taps" in harness and "meshStreamConfigTaps" in harness and "decodeMeshTaps" in harness


def test_adapter_has_the_calls_and_unpacks_as_numpy_does(tmp_path):
    text = open(os.path.join(HOST, "recon_integration_hip.hpp")).read()
    body = text[text.index("class ReconIntegrationHip"):]
    body = body[:body.index("\n};")]
    for m in ("meshStreamConfigTaps", "meshStreamFrameTaps", "decodeMeshTaps"):
        assert re.search(r"\b%s\s*\(" % m, body), m
    assert all(n in body for n in NAMES) and body.index("decodeMeshTriangles(") < body.index("decodeMeshTaps(")
    src = tmp_path / "use_mesh_taps.cpp"
    src.write_text('#include <cstdint>\n#include <cstdio>\n#include <cstring>\n#include <vector>\n'
                   '#include "recon_integration_hip.hpp"\n'
                   'using R = kinect::ReconIntegrationHip;\n'
                   '// what a sender does per frame: the mesh and, beside it, 8 * N bytes of taps per vertex\n'
                   'std::size_t per_frame(R& recon, std::uint64_t f, std::vector<unsigned char>& wire) {\n'
                   '  if (f == 0) { recon.configureMeshStream(false, false, 1u << 20, 1u << 21, 1u << 14, 3u); recon.meshStreamConfigTaps(); }\n'
                   '  if (!recon.meshStreamHasTaps() || !recon.streamMesh(f)) return 0;\n'
                   '  tsdf_mesh_frame fr;\n'
                   '  if (!recon.acquireMeshFrame(fr, false)) return 0;\n'
                   '  const tsdf_mesh_taps t = recon.meshStreamFrameTaps();\n'
                   '  wire.assign((const unsigned char*)t.taps, (const unsigned char*)(t.taps + t.n_vertices * t.n_streams));\n'
                   '  const std::size_t n = R::decodeMeshTaps(t).size();\n'
                   '  recon.releaseMeshFrame();\n'
                   '  return n;\n'
                   '}\n'
                   '// every binary16 value through the unpacking: the bits of the fp32 results\n'
                   'int main() {\n'
                   '  std::vector<tsdf_packed_tap> p(65536);\n'
                   '  for (std::uint32_t k = 0; k < 65536; ++k) p[k] = tsdf_packed_tap{(std::uint16_t)k, (std::uint16_t)(65535 - k), (std::uint16_t)k, (std::uint16_t)(k ^ 0x8000u)};\n'
                   '  const tsdf_mesh_taps t{p.data(), 16384, 4, 8};\n'
                   '  const std::vector<tsdf_texture_tap> out = R::decodeMeshTaps(t);\n'
                   '  if (out.size() != 65536) return 1;\n'
                   '  std::fwrite(out.data(), sizeof(tsdf_texture_tap), out.size(), stdout);\n'
                   '  return 0;\n'
                   '}\n')
    exe = str(tmp_path / "use_mesh_taps")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + HOST, str(src), "-o", exe,
                           "-L" + os.path.join(ROOT, "rgbd-recon_amd"), "-lrgbd_recon_hip", "-Wl,-rpath," + os.path.join(ROOT, "rgbd-recon_amd")])
    raw = subprocess.run([exe], capture_output=True, check=True).stdout
    import rgbd_recon_amd as rr
    got = np.frombuffer(raw, rr.TEXTURE_TAP_DTYPE)
    k = np.arange(65536, dtype=np.uint32)
    packed = np.zeros(65536, rr.PACKED_TAP_DTYPE)
    packed["u"], packed["v"], packed["quality_h"], packed["dist_h"] = k, 65535 - k, k, k ^ 0x8000
    want = rr.unpack_mesh_taps(packed)
    for name in ("u", "v", "quality", "dist"):
        a, b = got[name].view(np.uint32), want[name].view(np.uint32)
        assert ((a == b) | (np.isnan(got[name]) & np.isnan(want[name]))).all(), name


def test_kernel_file_is_built_into_the_library():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "k_mesh_stream_taps.o" in mk and os.path.exists(os.path.join(CSRC, "k_mesh_stream_taps.hip"))
    assert "texture_taps_dev.hpp" in mk and os.path.exists(os.path.join(CSRC, "texture_taps_dev.hpp"))
    kernel = open(os.path.join(CSRC, "k_mesh_stream_taps.hip")).read()
    shared = open(os.path.join(CSRC, "k_texture_taps.hip")).read()
    assert "texture_tap_values(" in kernel and "texture_tap_values(" in shared     # one evaluation, two kernels
    code = kernel[kernel.index("namespace rr"):]
    assert "__shared__" not in code and "__syncthreads" not in code and "atomic" not in code      # no LDS, no barrier, no statistics


def test_harness_accepts_the_taps_option(tmp_path):
    exe = str(tmp_path / "frame_harness")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(HOST, "frame_harness.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "rgbd-recon_amd"), "-lrgbd_recon_hip", "-Wl,-rpath," + os.path.join(ROOT, "rgbd-recon_amd")])
    bad = subprocess.run([exe, "--mesh-stream-tap"], capture_output=True, text=True)
    assert bad.returncode == 1 and "[--mesh-stream-taps]" in bad.stderr
    for extra in ([], ["--mesh-stream-compact"], ["--mesh-stream-part"], ["--mesh-stream-min-triangles", "1"]):
        p = subprocess.run([exe, "--mesh-stream-taps"] + extra, capture_output=True, text=True)
        assert "usage" not in p.stderr, p.stderr
        if p.returncode == 0:
            assert "5 mesh frames streamed, 5 picked up in order, 0 mismatches" in p.stdout
        else:
            assert p.returncode == 3 and "no HIP device" in p.stderr
