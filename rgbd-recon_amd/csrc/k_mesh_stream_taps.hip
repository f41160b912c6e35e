// Texture taps in the streamed frame (tsdf_mesh_stream_config_taps; include/rgbd_recon_hip.h, "mesh streaming: texture taps in the frame", has the
// definition): per vertex of the frame and stream the 8-byte packed tap, taken at the position the RECEIVER reconstructs from the vertex's three uint16
// codes, u_q = q / 65535.0f.  The pass reads the slot's final packed rows -- behind the emit, with a filter behind its scatter and final header -- and
// nothing of the emit, so it is the same launch for every form of the ring (uint32 indices, level of detail, filtered, tile-local, slab parts).
//
// A lane is one (vertex, stream) pair, k_texture_taps' mapping: blockIdx.y is the stream, a wave holds 64 consecutive vertices, the stream's LUT pointers
// and resolutions are scalars and the 64 lanes read one LUT at neighbouring places.  Per lane ONE 8-byte load of the vertex's first 8 bytes (stride 8 or
// 16), three divisions, the 8 + 8 LUT taps and the 2 x 2 image footprint through blend_colors()' own device functions (texture_taps_dev.hpp, shared with
// k_texture_taps), the packing in registers, ONE 8-byte store.  No LDS, no barrier, no scratch, no atomics: every pair is evaluated (u_q lies in [0, 1]),
// so there are no statistics to keep.
// The launch is sized by the ring's max_vertices, as the streamed filter's launches are; the frame's n_vertices is read from the slot's device header (a
// scalar load), and a workgroup beyond it returns at once.  An overflowed or emptied frame has n_vertices = 0 and writes nothing.
#include "texture_taps_dev.hpp"
#include "texture_taps.hpp"

namespace rr {

__global__ __launch_bounds__(kTapsThreads) void k_mesh_stream_taps(StreamTable T, FrameImages F, float limit, const MeshStreamHeader* __restrict__ H,
                                                                   const uint8_t* __restrict__ vertices, uint32_t stride, uint2* __restrict__ taps) {
  const unsigned long long nv = H->n_vertices;                           // (<= max_vertices < 2^32: the header launch wrote it, 0 on overflow)
  if ((unsigned long long)blockIdx.x * kTapsThreads >= nv) return;
  const uint32_t vertex = blockIdx.x * kTapsThreads + threadIdx.x, stream = blockIdx.y;   // (gridDim.y = T.n)
  if (vertex >= nv) return;
  const uint2 w = *(const uint2*)(vertices + (size_t)vertex * stride);   // qx | qy << 16, qz | 0 << 16 (vertex < n_vertices: inside the payload's vertices)
  const float3 u = make_float3((float)(w.x & 0xffffu) / 65535.0f, (float)(w.x >> 16) / 65535.0f, (float)(w.y & 0xffffu) / 65535.0f);
  const TapValues t = texture_tap_values(T.s[stream], F, (int)stream, limit, u);
  taps[(size_t)vertex * (uint32_t)T.n + stream] = pack_tap(t.pcol, t.quality, t.dist);   // (vertex < n_vertices <= max_vertices, stream < N: inside the block)
}

void launch_mesh_stream_taps(hipStream_t st, const StreamTable& T, const FrameImages& F, float limit, const MeshStreamHeader* H, const uint8_t* vertices,
                             uint32_t stride, uint32_t max_vertices, void* taps) {
  const dim3 g((uint32_t)tap_grid(max_vertices), (uint32_t)T.n), b(kTapsThreads);   // (at most 2^32 / 256 = 2^24 workgroups per stream)
  hipLaunchKernelGGL(k_mesh_stream_taps, g, b, 0, st, T, F, limit, H, vertices, stride, (uint2*)taps);
}

}  // namespace rr
