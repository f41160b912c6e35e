"""CPU: the texture taps' host bookkeeping (rgbd-recon_amd/csrc/texture_taps.hpp, with result_paths.hpp's CallStaging / CallChunks; HIP-free) as a
stand-alone program with its own main, built with the host address and undefined-behaviour sanitizers: the argument codes, the staging's growth, the cut
of a call into launches, the pair and grid arithmetic in 64 bits and the byte counts."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbd-recon_amd", "csrc")

MAIN = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "texture_taps.hpp"
#include "result_paths.hpp"
using namespace rr;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #x); std::exit(1); } } while (0)
int main() {
  // arguments
  CHECK(texture_taps_arguments(0, 0, false, false, false) == 0);
  CHECK(texture_taps_arguments(0, 4, false, false, false) == 1 && texture_taps_arguments(7, 8, true, true, false) == 1);   // an unknown flag, also with nothing to do
  CHECK(texture_taps_arguments(7, 0, true, true, false) == 0 && texture_taps_arguments(7, kTapsFlagUnitCube, true, true, false) == 0);
  CHECK(texture_taps_arguments(7, 0, false, true, false) == 2 && texture_taps_arguments(7, 0, true, false, false) == 2);
  CHECK(texture_taps_arguments(7, 0, true, true, true) == 3 && texture_taps_arguments(7, kTapsFlagSensor, true, true, false) == 3);
  CHECK(texture_taps_arguments(7, kTapsFlagSensor | kTapsFlagUnitCube, true, true, true) == 0);
  CHECK(texture_taps_arguments(kTapsMaxPoints, 0, true, true, false) == 0 && texture_taps_arguments(kTapsMaxPoints + 1, 0, true, true, false) == 4);
  CHECK(mesh_texture_taps_arguments(0) == 0 && mesh_texture_taps_arguments(kTapsFlagSensor) == 0);
  CHECK(mesh_texture_taps_arguments(kTapsFlagUnitCube) == 5 && mesh_texture_taps_arguments(kTapsFlagUnitCube | kTapsFlagSensor) == 5 && mesh_texture_taps_arguments(4) == 1);
  // staging: grows to a power of two of points, then keeps it
  CallStaging s;
  CHECK(s.grow(1) == 1024 && s.grow_extra(1, false) == 0 && s.grow_extra(1, true) == 1024);
  s.grown(1024);
  CHECK(s.grow(1024) == 0 && s.grow(1025) == 2048 && s.grow(1000000) == (1u << 20) && s.grow(kTapsMaxPoints) == kTapsMaxPoints);
  s.extra_grown(4096);
  CHECK(s.grow_extra(4096, true) == 0 && s.grow_extra(4097, true) == 8192 && s.grow_extra(1u << 20, false) == 0 && s.capacity == 1024);
  s.released();
  CHECK(s.capacity == 0 && s.extra_capacity == 0);
  // launches: they tile [0, n) exactly, none longer than 2^18 points; a launch's pairs fit 32 bits with 16 streams
  CHECK(kTapsChunk == (1u << 18));
  for (unsigned long long n : {1ull, 262143ull, 262144ull, 262145ull, 1000000ull}) {
    std::vector<unsigned char> covered((size_t)n, 0);
    const CallChunks K{n, kTapsChunk};
    unsigned long long next = 0;
    for (unsigned long long k = 0; k < K.launches(); ++k) {
      CHECK(K.first(k) == next && K.count(k) >= 1 && K.count(k) <= kTapsChunk);
      CHECK(tap_pairs(K.count(k), 16) <= 0xffffffffull && tap_grid(K.count(k)) <= (1u << 10) && tap_grid(K.count(k)) * 16 * kTapsThreads >= tap_pairs(K.count(k), 16));
      for (unsigned long long i = 0; i < K.count(k); ++i) covered[(size_t)(K.first(k) + i)] += 1;
      next += K.count(k);
    }
    CHECK(next == n);
    for (unsigned char c : covered) CHECK(c == 1);
  }
  CHECK((CallChunks{0, kTapsChunk}.launches() == 0));
  CHECK((CallChunks{1000000, kTapsChunk}.launches() == 4) && (CallChunks{1000000, kTapsChunk}.count(3) == 1000000 - 3 * 262144));
  // pairs, grid and bytes in 64 bits: 2^40 points x 16 streams
  const uint64_t big = 1ull << 40;
  CHECK(tap_pairs(big, 16) == (1ull << 44) && tap_grid(tap_pairs(big, 16)) == (1ull << 36));
  CHECK(tap_pairs(3, 5) == 15 && tap_grid(15) == 1 && tap_grid(256) == 1 && tap_grid(257) == 2 && tap_grid(0) == 0);
  CHECK(tap_point_bytes(big) == 12 * big && tap_record_bytes(big, 16) == (1ull << 48) && tap_record_bytes(1000, 3) == 48000);
  CHECK((CallChunks{big, kTapsChunk}.launches() == (1ull << 22)) && (CallChunks{big, kTapsChunk}.first((1ull << 22) - 1) == big - kTapsChunk));
  // the statistics' counters: a pair per slot, each in a 128-byte line of its own, consecutive waves on different slots; the host's sum
  CHECK(kTapStatBytes == 8192 && (kTapStatSlots & (kTapStatSlots - 1)) == 0 && kTapStatStride * 8 == 128);
  std::vector<unsigned long long> words(kTapStatSlots * kTapStatStride, 0);
  for (uint32_t wave = 0; wave < 1000; ++wave) {
    const uint32_t w = tap_stat_word(wave);
    CHECK(w + 1 < words.size() && w % kTapStatStride == 0 && (wave == 0 || w != tap_stat_word(wave - 1)));
    words[w] += wave; words[w + 1] += 1;
  }
  CHECK(tap_stat_word(0xffffffffu) == (kTapStatSlots - 1) * kTapStatStride);
  uint64_t sums[2];
  tap_stat_sum(words.data(), sums);
  CHECK(sums[0] == 999ull * 1000 / 2 && sums[1] == 1000);
  std::puts("texture taps staging ok");
  return 0;
}
'''


def test_texture_taps_staging_under_the_host_sanitizers(tmp_path):
    src = tmp_path / "texture_taps_main.cpp"
    src.write_text(MAIN)
    exe = str(tmp_path / "texture_taps_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, str(src), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "texture taps staging ok" in p.stdout, p.stdout + p.stderr
