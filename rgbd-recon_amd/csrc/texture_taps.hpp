// Host bookkeeping of the texture taps (tsdf_texture_taps / tsdf_texture_taps_dev / tsdf_mesh_texture_taps), free of HIP: which arguments a call accepts,
// the pair count and grid size of a launch, the statistics' counters, the byte counts; how the staging grows and how a call is cut into launches is
// result_paths.hpp's (CallStaging, CallChunks).  abi.cpp issues the calls; tests/test_texture_taps_staging.py runs this text under the host sanitizers.
#pragma once
#include <stdint.h>

namespace rr {

constexpr uint32_t kTapsFlagUnitCube = 1u, kTapsFlagSensor = 2u;   // TSDF_TAPS_UNIT_CUBE, TSDF_TAPS_SENSOR
constexpr uint32_t kTapsFlagsAll = kTapsFlagUnitCube | kTapsFlagSensor;
constexpr uint64_t kTapPointBytes = 12;           // float xyz[3]
constexpr uint64_t kTapBytes = 16;                // sizeof(tsdf_texture_tap) == sizeof(tsdf_sensor_tap)
constexpr uint64_t kTapsMaxPoints = 1ull << 40;   // points of one call: with 16 streams every byte count stays below 2^48
constexpr uint32_t kTapsChunk = 1u << 18;         // points of one launch
constexpr uint32_t kTapsThreads = 256;            // lanes of a workgroup: one lane per (point, stream) pair

// 0: the arguments of a call are acceptable; 1: unknown flag; 2: a NULL point / tap array with n > 0; 3: `sensor` given without TSDF_TAPS_SENSOR, or
// missing with it; 4: more points than a call takes
inline int texture_taps_arguments(uint64_t n, uint32_t flags, bool have_points, bool have_taps, bool have_sensor) {
  if (flags & ~kTapsFlagsAll) return 1;
  if (n == 0) return 0;
  if (!have_points || !have_taps) return 2;
  if (((flags & kTapsFlagSensor) != 0) != have_sensor) return 3;
  if (n > kTapsMaxPoints) return 4;
  return 0;
}
// the mesh form: 0, or 1 for an unknown flag, 5 for TSDF_TAPS_UNIT_CUBE (the mesh's positions are world coordinates)
inline int mesh_texture_taps_arguments(uint32_t flags) {
  if (flags & ~kTapsFlagsAll) return 1;
  if (flags & kTapsFlagUnitCube) return 5;
  return 0;
}

// tsdf_texture_tap_stats' two counts are added to by one atomic per wave and count.  A hundred thousand waves adding to ONE address serialise in the
// cache (measured: 1.14 ms instead of 0.23 ms for the 1.67 M vertices of c2's mesh), so the counters are kTapStatSlots pairs, each pair in a 128-byte line
// of its own; a wave adds to the pair of its number, and the host sums the pairs.
constexpr uint32_t kTapStatSlots = 64;            // a power of two
constexpr uint32_t kTapStatStride = 16;           // 64-bit words from one pair to the next: 128 bytes
constexpr uint64_t kTapStatBytes = (uint64_t)kTapStatSlots * kTapStatStride * 8;
// the first word of the pair wave `wave` (its number in the launch) adds to: {pairs with quality > 0, pairs not evaluated}  (constexpr: host and device)
constexpr uint32_t tap_stat_word(uint32_t wave) { return (wave & (kTapStatSlots - 1)) * kTapStatStride; }
inline void tap_stat_sum(const unsigned long long* words, uint64_t out[2]) {
  out[0] = out[1] = 0;
  for (uint32_t k = 0; k < kTapStatSlots; ++k) { out[0] += words[k * kTapStatStride]; out[1] += words[k * kTapStatStride + 1]; }
}

// byte counts of n points / of their records with N streams (n <= kTapsMaxPoints, N <= 16: below 2^48)
inline uint64_t tap_point_bytes(uint64_t n) { return n * kTapPointBytes; }
inline uint64_t tap_record_bytes(uint64_t n, uint32_t streams) { return n * (uint64_t)streams * kTapBytes; }
// (point, stream) pairs of n points -- the lanes that work, the records written -- and the workgroups that cover `lanes` lanes, in 64 bits.  A launch's
// grid is tap_grid(its points) workgroups per stream (blockIdx.y = stream): tap_grid(points) * streams in all
inline uint64_t tap_pairs(uint64_t n, uint32_t streams) { return n * (uint64_t)streams; }
inline uint64_t tap_grid(uint64_t lanes) { return (lanes + kTapsThreads - 1) / kTapsThreads; }

}  // namespace rr
