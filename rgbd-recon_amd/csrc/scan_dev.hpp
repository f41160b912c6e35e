// Prefix sums inside a wave and a workgroup: what the mesh extraction's scans (k_mesh.hip) and the mesh components' (k_mesh_components.hip) are built on.
#ifndef RR_SCAN_DEV_HPP
#define RR_SCAN_DEV_HPP
#include <hip/hip_runtime.h>
#include <cstdint>

namespace rr {

// inclusive prefix sum inside a wave: Hillis-Steele over each row of 16 lanes with DPP row shifts (a lane without a source adds 0), then
// the two row broadcasts
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v) {
#define RR_DPP_ADD(ctrl, rm) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rm, 0xf, false)
  RR_DPP_ADD(0x111, 0xf); RR_DPP_ADD(0x112, 0xf); RR_DPP_ADD(0x114, 0xf); RR_DPP_ADD(0x118, 0xf);   // row_shr 1, 2, 4, 8
  RR_DPP_ADD(0x142, 0xa); RR_DPP_ADD(0x143, 0xc);                                                   // row_bcast 15 -> rows 1, 3; row_bcast 31 -> rows 2, 3
#undef RR_DPP_ADD
  return v;
}
// exclusive prefix sum over the workgroup (every lane calls it); *total = the workgroup's sum.  s_wave: kWaves words of LDS.
template <int kWaves>
__device__ __forceinline__ uint32_t block_exclusive_sum(uint32_t v, uint32_t* s_wave, uint32_t* total) {
  const uint32_t inc = wave_inclusive_sum(v);
  const int wave = threadIdx.x >> 6;
  __syncthreads();                                                     // (s_wave may still be read from the previous call)
  if ((threadIdx.x & 63) == 63) s_wave[wave] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) { const uint32_t s = s_wave[w]; all += s; if (w < wave) before += s; }
  *total = all;
  return before + inc - v;
}

}  // namespace rr
#endif
