"""CPU: the ray queries' host bookkeeping (rgbd-recon_amd/csrc/ray_staging.hpp, with result_paths.hpp's CallStaging / CallChunks; HIP-free) as a stand-alone
program with its own main, built with the host address and undefined-behaviour sanitizers: argument checks, the staging's growth, the cut of a cast into
launch pairs, the run length and the sample bound."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbd-recon_amd", "csrc")

MAIN = r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ray_staging.hpp"
#include "result_paths.hpp"
using namespace rr;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #x); std::exit(1); } } while (0)
int main() {
  // arguments
  CHECK(ray_cast_arguments(0, 0, false, false, false) == 0);
  CHECK(ray_cast_arguments(0, 8, false, false, false) == 1);           // an unknown flag is refused even with nothing to cast
  CHECK(ray_cast_arguments(5, 0, true, true, false) == 0);
  CHECK(ray_cast_arguments(5, 0, false, true, false) == 2 && ray_cast_arguments(5, 0, true, false, false) == 2);
  CHECK(ray_cast_arguments(5, kRayFlagNormals, true, true, false) == 3 && ray_cast_arguments(5, kRayFlagUnitCube, true, true, true) == 3);
  CHECK(ray_cast_arguments(5, kRayFlagColours | kRayFlagUnitCube, true, true, true) == 0);
  CHECK(ray_cast_arguments(kRayMaxCount + 1, 0, true, true, false) == 4 && ray_cast_arguments(kRayMaxCount, 0, true, true, false) == 0);
  CHECK(ray_view_rect(0, 0, 64, 36, 64, 36) == 0 && ray_view_rect(63, 35, 1, 1, 64, 36) == 0);
  CHECK(ray_view_rect(0, 0, 0, 1, 64, 36) == 1 && ray_view_rect(-1, 0, 1, 1, 64, 36) == 1 && ray_view_rect(0, 0, 1, -3, 64, 36) == 1);
  CHECK(ray_view_rect(63, 0, 2, 1, 64, 36) == 2 && ray_view_rect(0, 36, 1, 1, 64, 36) == 2 && ray_view_rect(2147483647, 0, 2147483647, 1, 64, 36) == 2);
  // staging: grows to a power of two, then keeps it
  CallStaging s;
  CHECK(s.grow(1) == 1024 && s.grow_extra(1, false) == 0 && s.grow_extra(1, true) == 1024);
  s.grown(1024);
  CHECK(s.grow(1024) == 0 && s.grow(1025) == 2048 && s.grow(kRayMaxCount) == kRayMaxCount);
  s.extra_grown(4096);
  CHECK(s.grow_extra(4096, true) == 0 && s.grow_extra(4097, true) == 8192 && s.capacity == 1024);
  s.released();
  CHECK(s.capacity == 0 && s.extra_capacity == 0);
  // launch pairs: they tile [0, n) exactly, none longer than the list; what a pair indexes stays inside an array of n records
  for (unsigned long long n : {1ull, 63ull, 64ull, 65ull, 262143ull, 262144ull, 262145ull, 1000000ull}) {
    std::vector<unsigned char> covered((size_t)n, 0);
    const CallChunks K{n, 1u << 18};
    unsigned long long next = 0;
    for (unsigned long long k = 0; k < K.launches(); ++k) {
      CHECK(K.first(k) == next && K.count(k) >= 1 && K.count(k) <= (1u << 18));
      for (unsigned long long i = 0; i < K.count(k); ++i) covered[(size_t)(K.first(k) + i)] += 1;
      next += K.count(k);
    }
    CHECK(next == n);
    for (unsigned char c : covered) CHECK(c == 1);
  }
  CHECK((CallChunks{0, 1u << 18}.launches() == 0));
  // the run: (run - 1) steps of limit / 2 * res voxels stay within 6 voxels, between 1 and 32 samples
  const int r512[3] = {512, 512, 512}, r32[3] = {32, 40, 24}, r4096[3] = {4096, 8, 8};
  CHECK(ray_run_length(0.01f, r512) == 3 && ray_run_length(0.04f, r32) == 8 && ray_run_length(0.04f, r4096) == 1 && ray_run_length(1.0e-6f, r32) == 32);
  CHECK(ray_run_length(0.0f, r32) == 1);
  for (float limit : {0.001f, 0.01f, 0.04f, 0.5f}) {
    const int run = ray_run_length(limit, r512);
    CHECK(run >= 1 && run <= 32 && (run == 1 || (float)(run - 1) * limit * 0.5f * 512.0f <= 6.0f));
  }
  // the sample bound: above every ray of the unit cube, finite for any limit
  CHECK(ray_sample_cap(0.04f) == 102.0f && ray_sample_cap(0.04f) > 1.7320508f / 0.02f + 1.0f);
  CHECK(ray_sample_cap(1.0e-12f) == 4.0e9f && ray_sample_cap(0.0f) == 4.0e9f && ray_sample_cap(-1.0f) == 4.0e9f);
  std::puts("ray staging ok");
  return 0;
}
'''


def test_ray_staging_under_the_host_sanitizers(tmp_path):
    src = tmp_path / "ray_staging_main.cpp"
    src.write_text(MAIN)
    exe = str(tmp_path / "ray_staging_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, str(src), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "ray staging ok" in p.stdout, p.stdout + p.stderr
