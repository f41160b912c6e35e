// Frame read-out (gfx950): the finished framebuffer as the client's window would hold it after glfwSwapBuffers (source/kinect_client.cpp:533;
// GLFW's default framebuffer is RGBA8) -- or that picture as the wire's DXT1 blocks -- written into a ring slot's device buffer, from where a copy
// stream takes it to pinned host memory (abi.cpp: tsdf_present).  The rules are stated in include/rgbd_recon_hip.h ("frame read-out") and restated in
// numpy in tests/present_reference.py; device and numpy agree byte for byte.
// Both kernels read the float4 framebuffer once and are bound by that read (16 B per pixel in, 4 B or 0.5 B out).
#include "tsdf_common.hpp"

namespace rr {

// GL 4.4 section 2.3.5.2 with round-to-nearest-even: the clamp maps NaN to 0 (fmaxf returns its other operand) and +-inf to 0 / 1, the product is
// taken in fp32 (-ffp-contract=off: nothing is fused into it), v_cvt_i32_f32 rounds half-way products to even
__device__ __forceinline__ uint32_t unorm8(float v) { return (uint32_t)__float2int_rn(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f); }
__device__ __forceinline__ uint32_t rgba8(float4 v) { return unorm8(v.x) | (unorm8(v.y) << 8) | (unorm8(v.z) << 16) | (unorm8(v.w) << 24); }

// One lane per pixel, pixels in framebuffer order: a wave loads 1 KiB and stores 256 B, both contiguous (a wave that straddles a row end stores
// two runs).  Flipping moves the destination row only.
__global__ __launch_bounds__(256) void k_present_rgba8(const float4* __restrict__ fb_c, uint32_t* __restrict__ out, int w, int h, int top_down) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= (uint32_t)(w * h)) return;
  const uint32_t j = p / (uint32_t)w, i = p - j * (uint32_t)w;
  const uint32_t dj = top_down ? (uint32_t)h - 1u - j : j;
  out[(size_t)dj * w + i] = rgba8(fb_c[p]);
}

typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b) {     // v_pk_max_u16
  const us2 r = __builtin_elementwise_max(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b));
  return __builtin_bit_cast(uint32_t, r);
}
__device__ __forceinline__ uint32_t pk16(uint32_t lo, uint32_t hi) { return lo | (hi << 16); }
__device__ __forceinline__ void expand565(uint32_t v, int e[3]) {
  const int r = (v >> 11) & 31, g = (v >> 5) & 63, b = v & 31;
  e[0] = (r << 3) | (r >> 2); e[1] = (g << 2) | (g >> 4); e[2] = (b << 3) | (b >> 2);
}

// A wave takes a strip of 16 x 4 output pixels = four blocks side by side: lane l holds the texel of column l & 15 and row l >> 4, so each of the
// strip's four rows is one 256-byte run of the framebuffer, and the 16 texels of a block sit in the lanes that share bits 2-3 of the lane
// number.  What the encoder needs of a whole block -- min / max per channel, the sums of the covariance test, the index word -- is combined
// over those lanes by butterflies across lane bits 0, 1 (the column) and 4, 5 (the row): every lane ends up with its block's values, computes
// the endpoints and the palette redundantly and its own 2-bit index; lane (0, 0) of the block stores the 8 bytes (the strip's four stores are
// one 32-byte run).  Lanes outside the image hold the clamped texel (the replicated last column / row) and take part in every butterfly.
__global__ __launch_bounds__(256) void k_present_dxt1(const float4* __restrict__ fb_c, uint2* __restrict__ out, int w, int h, int top_down) {
  const int nbx = (w + 3) >> 2, nby = (h + 3) >> 2, nsx = (nbx + 3) >> 2;
  const uint32_t strip = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (strip >= (uint32_t)(nsx * nby)) return;                            // (wave-uniform)
  const int l = threadIdx.x & 63, tx = l & 15, ty = l >> 4;
  const int sy = (int)(strip / (uint32_t)nsx), sx = (int)strip - sy * nsx;
  const int ox = min(sx * 16 + tx, w - 1), oy = min(sy * 4 + ty, h - 1); // output coordinates, clamped
  const int fy = top_down ? h - 1 - oy : oy;
  const uint32_t px = rgba8(fb_c[(size_t)fy * w + ox]);
  const uint32_t r = px & 255u, g = (px >> 8) & 255u, b = (px >> 16) & 255u;
  // max of (c, 255 - c) per channel as three packed pairs; sums: (sum r | sum g << 16), (sum r g | sum b << 20) -- 16 * 255^2 < 2^20 --, sum b g
  constexpr int kXor[4] = {1, 2, 16, 32};                                 // lane bits 0, 1 (column in the block) and 4, 5 (row)
  uint32_t m0 = pk16(r, g), m1 = pk16(b, 255u - r), m2 = pk16(255u - g, 255u - b);
  uint32_t s0 = pk16(r, g), s1 = (r * g) | (b << 20), s2 = b * g;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int d = kXor[i];
    m0 = pk_max(m0, (uint32_t)__shfl_xor((int)m0, d)); m1 = pk_max(m1, (uint32_t)__shfl_xor((int)m1, d)); m2 = pk_max(m2, (uint32_t)__shfl_xor((int)m2, d));
    s0 += (uint32_t)__shfl_xor((int)s0, d); s1 += (uint32_t)__shfl_xor((int)s1, d); s2 += (uint32_t)__shfl_xor((int)s2, d);
  }
  int hi[3] = {(int)(m0 & 0xffffu), (int)(m0 >> 16), (int)(m1 & 0xffffu)};
  int lo[3] = {255 - (int)(m1 >> 16), 255 - (int)(m2 & 0xffffu), 255 - (int)(m2 >> 16)};
  const int sum_r = (int)(s0 & 0xffffu), sum_g = (int)(s0 >> 16), sum_b = (int)(s1 >> 20), sum_rg = (int)(s1 & 0xfffffu), sum_bg = (int)s2;
#pragma unroll
  for (int c = 0; c < 3; ++c) { const int inset = (hi[c] - lo[c]) >> 4; lo[c] += inset; hi[c] -= inset; }
  // the diagonal selection: r or b falling where g rises takes its low end in endpoint A
  const bool neg_r = 16 * sum_rg - sum_r * sum_g < 0, neg_b = 16 * sum_bg - sum_b * sum_g < 0;
  const int ar = neg_r ? lo[0] : hi[0], br = neg_r ? hi[0] : lo[0];
  const int ab = neg_b ? lo[2] : hi[2], bb = neg_b ? hi[2] : lo[2];
  const uint32_t a565 = (uint32_t)((ar >> 3) << 11 | (hi[1] >> 2) << 5 | (ab >> 3)), b565 = (uint32_t)((br >> 3) << 11 | (lo[1] >> 2) << 5 | (bb >> 3));
  const uint32_t c0 = max(a565, b565), c1 = min(a565, b565);
  int p0[3], p1[3];
  expand565(c0, p0); expand565(c1, p1);
  const int t[3] = {(int)r, (int)g, (int)b};
  int d0 = 0, d1 = 0, d2 = 0, d3 = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int e0 = t[c] - p0[c], e1 = t[c] - p1[c], e2 = t[c] - (2 * p0[c] + p1[c]) / 3, e3 = t[c] - (p0[c] + 2 * p1[c]) / 3;
    d0 += e0 * e0; d1 += e1 * e1; d2 += e2 * e2; d3 += e3 * e3;
  }
  uint32_t k = 0; int best = d0;                                         // (strict <: ties go to the lowest k)
  if (d1 < best) { best = d1; k = 1; }
  if (d2 < best) { best = d2; k = 2; }
  if (d3 < best) { best = d3; k = 3; }
  uint32_t word = k << (2 * ((ty << 2) | (tx & 3)));                      // texel i = 4 y + x at bits 2i .. 2i + 1
#pragma unroll
  for (int i = 0; i < 4; ++i) word |= (uint32_t)__shfl_xor((int)word, kXor[i]);
  if (c0 == c1) word = 0u;
  const int bx = sx * 4 + (tx >> 2);
  if ((l & 0x33) == 0 && bx < nbx) out[(size_t)sy * nbx + bx] = make_uint2(c0 | (c1 << 16), word);
}

void launch_present(hipStream_t st, const float4* fb_c, void* out, int w, int h, uint32_t format, int top_down) {
  if (format == 0u) {
    hipLaunchKernelGGL(k_present_rgba8, dim3(((uint32_t)(w * h) + 255u) / 256u), dim3(256), 0, st, fb_c, (uint32_t*)out, w, h, top_down);
  } else {
    const uint32_t strips = (uint32_t)((((w + 3) >> 2) + 3) >> 2) * (uint32_t)((h + 3) >> 2);
    hipLaunchKernelGGL(k_present_dxt1, dim3((strips + 3u) / 4u), dim3(256), 0, st, fb_c, (uint2*)out, w, h, top_down);
  }
}

}  // namespace rr
