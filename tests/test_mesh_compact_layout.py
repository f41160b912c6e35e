"""CPU: the mesh ring's slot and payload arithmetic (rgbd-recon_amd/csrc/result_paths.hpp: MeshFrameLayout, HIP-free) as a stand-alone program with its
own main, built with the host address and undefined-behaviour sanitizers.  The uint32 format must be the arithmetic the ring always had; the tile-local
format the header's: vertices, padding to 16, 16-byte rows, 6-byte triangles -- odd vertex counts at stride 8 for the padding, zero rows, and the 4 GiB
bound to the byte."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbd-recon_amd", "csrc")

MAIN = r'''
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "result_paths.hpp"
using namespace rr;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #x); std::exit(1); } } while (0)

int main() {
  unsigned long rows_walked = 0;
  for (uint32_t stride : {8u, 16u}) {
    const MeshFrameLayout u{kMeshIndexU32, stride}, t{kMeshIndexTile16, stride};
    CHECK(u.triangle_bytes() == 12 && t.triangle_bytes() == 6);
    for (uint64_t nv : {0ull, 1ull, 2ull, 3ull, 7ull, 8ull, 1001ull, 1667352ull, 4294967295ull})
      for (uint64_t nt : {0ull, 1ull, 5ull, 3334940ull})
        for (uint64_t rows : {0ull, 1ull, 27ull, 65536ull}) {
          ++rows_walked;
          // the uint32 format: what abi.cpp computed before the layout had a name; rows play no part
          CHECK(u.table_offset(nv) == nv * stride && u.triangle_offset(nv, rows) == nv * stride);
          CHECK(u.payload_bytes(nv, nt, rows) == (nv ? nv * stride + nt * 12 : 0));
          CHECK(u.payload_capacity(nv, nt, rows) == nv * stride + nt * 12 && u.slot_bytes(nv, nt, rows) == 64 + nv * stride + nt * 12);
          // the tile-local format
          const uint64_t pad = (16 - nv * stride % 16) % 16;
          CHECK(pad == (stride == 8 && (nv & 1) ? 8u : 0u));                              // eight bytes behind an odd count of 8-byte vertices, else none
          CHECK(t.table_offset(nv) == nv * stride + pad && t.table_offset(nv) % 16 == 0);
          CHECK(t.triangle_offset(nv, rows) == t.table_offset(nv) + rows * 16 && t.triangle_offset(nv, rows) % 16 == 0);
          CHECK(t.payload_capacity(nv, nt, rows) == nv * stride + pad + rows * 16 + nt * 6);
          CHECK(t.slot_bytes(nv, nt, rows) == 64 + t.payload_capacity(nv, nt, rows));
          CHECK(t.payload_bytes(nv, nt, rows) == (nv ? t.payload_capacity(nv, nt, rows) : 0));   // a frame's bytes: its counts', nothing for an empty one
          if (nv) CHECK(t.payload_bytes(nv, nt, rows) <= u.payload_bytes(nv, nt, rows) + pad + rows * 16);
        }
  }
  // zero rows and no triangle: the padded vertices alone
  CHECK((MeshFrameLayout{kMeshIndexTile16, 8}.payload_bytes(3, 0, 0)) == 32 && (MeshFrameLayout{kMeshIndexTile16, 16}.payload_bytes(3, 0, 0)) == 48);
  // the issue's c2 frame, level 0: 40.0 MB of triangles become 20.0 MB and a table
  CHECK((MeshFrameLayout{kMeshIndexU32, 8}.payload_bytes(1667352, 3334940, 0)) == 13338816ull + 40019280ull);
  CHECK((MeshFrameLayout{kMeshIndexTile16, 8}.payload_bytes(1667352, 3334940, 20000)) == 13338816ull + 320000ull + 20009640ull);
  // the 4 GiB edge.  uint32 format: on the payload, as ever.  4 GiB = 2^32 = 8 * 2^29 = 12 * 357913941 + 4
  const uint64_t G = 4ull << 30;
  CHECK(kMeshSlotLimit == G);
  CHECK((MeshFrameLayout{kMeshIndexU32, 8}.fits(1ull << 29, 0, 1)) && !(MeshFrameLayout{kMeshIndexU32, 8}.fits((1ull << 29) + 1, 0, 1)));
  CHECK((MeshFrameLayout{kMeshIndexU32, 16}.fits(1ull << 28, 0, 1)) && !(MeshFrameLayout{kMeshIndexU32, 16}.fits(1ull << 28, 1, 1)));
  CHECK((MeshFrameLayout{kMeshIndexU32, 8}.fits(1, 357913940, 4000000000ull)) && !(MeshFrameLayout{kMeshIndexU32, 8}.fits(1, 357913941, 1)));   // (8 + 12 * 357913941 = 2^32 + 4)
  // tile-local format: on the whole slot, header included.  64 + 16 + 16 + 6 t <= 2^32  <=>  t <= 715827866 (6 * 715827866 = 2^32 - 100)
  const MeshFrameLayout t8{kMeshIndexTile16, 8};
  CHECK(t8.slot_bytes(1, 715827866, 1) == G - 4 && t8.fits(1, 715827866, 1) && !t8.fits(1, 715827867, 1));
  CHECK(t8.slot_bytes(2, 0, (G - 64 - 16) / 16) == G && t8.fits(2, 0, (G - 64 - 16) / 16) && !t8.fits(2, 0, (G - 64 - 16) / 16 + 1) && !t8.fits(2, 1, (G - 64 - 16) / 16));
  CHECK(!t8.fits(4294967295ull, 4294967295ull, 4294967295ull));                          // the largest arguments: no wrap
  CHECK(t8.slot_bytes(4294967295ull, 4294967295ull, 4294967295ull) == 64 + 34359738360ull + 8 + 68719476720ull + 25769803770ull);
  std::printf("%lu layouts walked\n", rows_walked);
  std::puts("mesh compact layout ok");
  return 0;
}
'''


def test_layout_arithmetic_under_the_host_sanitizers(tmp_path):
    src = tmp_path / "mesh_compact_layout_main.cpp"
    src.write_text(MAIN)
    exe = str(tmp_path / "mesh_compact_layout_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, str(src), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0 and "mesh compact layout ok" in p.stdout, p.stdout + p.stderr
