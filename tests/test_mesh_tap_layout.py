"""CPU: where the streamed frame's tap block lives (rgbd-recon_amd/csrc/result_paths.hpp: MeshFrameLayout's tap_* functions, HIP-free) as a stand-alone
program with its own main, built with the host address and undefined-behaviour sanitizers: every layout function the ring had keeps its value, the
block sits align16(payload capacity) behind the payload's first byte, holds max_vertices * N * 8 bytes, a frame's bytes are n_vertices * N * 8, and the
4 GiB bound holds for the slot including the block, to the byte and with the largest arguments."""
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
  unsigned long walked = 0;
  CHECK(kMeshTapBytes == 8 && kMeshStreamTaps == 1u && kMeshHeaderBytes == 64 && kMeshSlotLimit == (4ull << 30));
  for (uint32_t format : {kMeshIndexU32, kMeshIndexTile16})
    for (uint32_t stride : {8u, 16u}) {
      const MeshFrameLayout L{format, stride};
      const uint64_t tb = format == kMeshIndexTile16 ? 6 : 12;
      for (uint64_t nv : {0ull, 1ull, 2ull, 3ull, 7ull, 8ull, 1001ull, 1667352ull, 4294967295ull})
        for (uint64_t nt : {0ull, 1ull, 5ull, 3334940ull, 4294967295ull})
          for (uint64_t rows : {0ull, 1ull, 27ull, 65536ull}) {
            ++walked;
            // every function the ring had, restated from the header's words: nothing moved
            const uint64_t pad = format == kMeshIndexTile16 ? (16 - nv * stride % 16) % 16 : 0, table = format == kMeshIndexTile16 ? rows * 16 : 0;
            CHECK(L.triangle_bytes() == tb && L.table_offset(nv) == nv * stride + pad && L.triangle_offset(nv, rows) == nv * stride + pad + table);
            CHECK(L.payload_capacity(nv, nt, rows) == nv * stride + pad + table + nt * tb && L.slot_bytes(nv, nt, rows) == 64 + L.payload_capacity(nv, nt, rows));
            CHECK(L.payload_bytes(nv, nt, rows) == (nv ? L.payload_capacity(nv, nt, rows) : 0));
            CHECK(L.fits(nv, nt, rows) == ((format == kMeshIndexTile16 ? L.slot_bytes(nv, nt, rows) : L.payload_capacity(nv, nt, rows)) <= (4ull << 30)));
            // the block: behind the capacity, at a multiple of 16 (8-byte stores and a 16-byte-aligned copy), never inside the payload
            const uint64_t cap = L.payload_capacity(nv, nt, rows), at = L.tap_offset(nv, nt, rows);
            CHECK(at % 16 == 0 && at >= cap && at - cap < 16 && at == (cap + 15) / 16 * 16);
            for (uint64_t n : {1ull, 3ull, 4ull, 5ull, 16ull}) {
              CHECK(MeshFrameLayout::tap_capacity(nv, n) == nv * n * 8 && MeshFrameLayout::tap_bytes(nv, n) == nv * n * 8);
              CHECK(L.slot_bytes_taps(nv, nt, rows, n) == 64 + at + nv * n * 8 && L.slot_bytes_taps(nv, nt, rows, n) >= L.slot_bytes(nv, nt, rows));
              CHECK(L.fits_taps(nv, nt, rows, n) == (L.fits(nv, nt, rows) && L.slot_bytes_taps(nv, nt, rows, n) <= (4ull << 30)));
              if (!L.fits(nv, nt, rows)) CHECK(!L.fits_taps(nv, nt, rows, n));                // the block never makes room
            }
          }
    }
  // a frame's tap bytes are its counts', never the capacity's: c2's level-0 frame with 4 streams, and an empty one
  CHECK(MeshFrameLayout::tap_bytes(1667352, 4) == 53355264ull && MeshFrameLayout::tap_bytes(0, 4) == 0);
  // the payload capacity of an odd triangle count is no multiple of 16: the block moves up, the payload does not
  const MeshFrameLayout u8{kMeshIndexU32, 8}, u16{kMeshIndexU32, 16}, t8{kMeshIndexTile16, 8};
  CHECK(u8.payload_capacity(3, 1, 9) == 36 && u8.tap_offset(3, 1, 9) == 48 && u8.slot_bytes_taps(3, 1, 9, 2) == 64 + 48 + 48);
  CHECK(t8.payload_capacity(3, 1, 2) == 32 + 32 + 6 && t8.tap_offset(3, 1, 2) == 80);
  // the 4 GiB edge, to the byte.  uint32 format, 1 stream: 64 + 16 v + 8 v <= 2^32 with no triangle  <=>  v <= 178956968 (24 * 178956968 = 2^32 - 64)
  const uint64_t G = 4ull << 30;
  CHECK(u16.slot_bytes_taps(178956968, 0, 1, 1) == G && u16.fits_taps(178956968, 0, 1, 1) && !u16.fits_taps(178956969, 0, 1, 1));
  CHECK(u16.fits(178956969, 0, 1));                                                            // ... which the ring without taps still takes
  // one triangle more: 12 bytes and 4 of padding
  CHECK(u16.slot_bytes_taps(178956967, 1, 1, 1) == G - 24 + 16 && u16.fits_taps(178956967, 1, 1, 1) && !u16.fits_taps(178956968, 1, 1, 1));
  // 16 streams at stride 8: 64 + 8 v + 128 v <= 2^32  <=>  v <= 31580641 (136 * 31580641 = 2^32 - 120; v odd: no padding in the uint32 format, 8 before the block)
  CHECK(u8.slot_bytes_taps(31580641, 0, 1, 16) == G - 120 + 64 + 8 && u8.fits_taps(31580641, 0, 1, 16) && !u8.fits_taps(31580642, 0, 1, 16));
  // tile-local format: the ring's own bound is on the slot already; the block comes on top
  CHECK(t8.fits(1, 715827866, 1) && !t8.fits_taps(1, 715827866, 1, 16) && t8.fits_taps(1, 715827840, 1, 16));
  CHECK(t8.slot_bytes_taps(1, 715827840, 1, 16) == 64 + (16 + 16 + 6 * 715827840ull) + 128);
  // the largest arguments: no wrap anywhere
  const uint64_t M = 4294967295ull;
  CHECK(!u8.fits_taps(M, M, M, 16) && !t8.fits_taps(M, M, M, 16) && !u16.fits_taps(M, M, M, 1));
  CHECK(t8.slot_bytes_taps(M, M, M, 16) == 64 + (34359738360ull + 8 + 68719476720ull + 25769803770ull + 6) + M * 128);
  CHECK(u16.slot_bytes_taps(M, M, M, 16) == 64 + (M * 16 + M * 12 + 12) + M * 128);        // (28 M = 28 * 2^32 - 28: 12 short of a multiple of 16)
  std::printf("%lu layouts walked\n", walked);
  std::puts("mesh tap layout ok");
  return 0;
}
'''


def test_tap_block_arithmetic_under_the_host_sanitizers(tmp_path):
    src = tmp_path / "mesh_tap_layout_main.cpp"
    src.write_text(MAIN)
    exe = str(tmp_path / "mesh_tap_layout_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, str(src), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0 and "mesh tap layout ok" in p.stdout, p.stdout + p.stderr
