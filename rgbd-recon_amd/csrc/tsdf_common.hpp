// Shared host/device declarations of the HIP TSDF core (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rgbd_recon_hip.h"
#include "launch_plan.hpp"

namespace rr {

constexpr int TILE = 8;            // storage tile edge: the TSDF lives in HBM as 8x8x8 tiles of 2 KiB
constexpr int TILE_VOX = 512;

// One calibrated stream: its three LUT volumes (CalibVolumes.cpp:64-80,132-144)
struct StreamLut {
  const float4* inv;   // cv_xyz_inv RGBA32F
  const float2* uv;    // cv_uv      RG32F
  const float4* xyz;   // cv_xyz     RGB32F padded to 16 B texels on upload
  int inv_res[3], uv_res[3], xyz_res[3];
};
struct StreamTable {
  StreamLut s[TSDF_MAX_STREAMS];
  int n;
};

// Per-frame images as resident in HBM: one 16-B texel {depth.r, quality, silhouette, 0} per depth pixel
// (the three arrays are always fetched at the same coordinate, tsdf_integration.vs:32-50) and RGBA8 colour.
struct FrameImages {
  const float4* dqs;      // [N][H][W]
  const float* depth;     // [N][H][W] depth.r alone (brick marking reads nothing else)
  const uchar4* color;    // [N][Hc][Wc]
  int w, h, cw, ch;
  // per 8x8-pixel cell {min depth, max depth, min silhouette, max silhouette} of the packed image, [N][rch][rcw] (k_frame_ranges): lets the
  // dense integrate decide for a whole tile and stream that every voxel takes the same branch of the fusion rule.  nullptr: not built.
  const float4* ranges;
  int rcw, rch;
};

// TSDF volume, tile-major: tile (tx,ty,tz) at ((tz - tz0) * nty + ty) * ntx + tx, voxel (x&7,y&7,z&7) inside
// n / d for n < 2^27 by one 64-bit multiply and a shift (m = floor(2^k / d) + 1, k = 27 + ceil(log2 d): exact, see make_fast_div).
// A tile id is workgroup-uniform in the integrate kernels: this form stays on the scalar unit, an integer division does not.
struct FastDiv { uint32_t m, k; };
struct Volume {
  float* data;
  int res[3];          // logical resolution
  int ntx, nty;        // tiles per axis (x, y); z tiles stored: [tz0, tz1)
  FastDiv div_layer, div_row;   // tile id / (ntx * nty), (tile id within a layer) / ntx
  int tz0, tz1;        // stored tile layers (owned slab + halo)
  int own_tz0, own_tz1;  // owned tile layers: the samples of the raymarch this context is responsible for
  int int_tz0, int_tz1;  // tile layers integrate() computes: the owned ones, plus the halo when it is recomputed locally
  int zlo, zhi;        // stored voxel planes [zlo, zhi]: every Z tap is clamped into them (slab contexts)
  // Sparse tile pool (tsdf_config::sparse_pool_tiles): `data` is a pool of pool_tiles tiles and slot[stored tile index] is the
  // tile's position in it, or kNoSlot (every voxel of the tile reads -limit).  The TSDF is rebuilt from scratch every frame,
  // so a tile's slot is simply its position in this frame's compacted active list: no free list, no fragmentation.
  uint32_t* slot;      // nullptr: dense storage
  uint32_t pool_tiles;
  const uint8_t* cls;  // tile class of every STORED tile, index ((tz - tz0) * nty + ty) * ntx + tx; halo layers stay kTileMixed
  int n_stored_tiles;
  float limit;
};

// Per-tile bookkeeping of the integrated tiles (index = tile id, x fastest, int_tz0 first):
//   active  this frame: some voxel of the tile is in the voxel list of an occupied brick
//   cls     what the tile's 2 KiB in HBM hold: kTileMinus = every voxel is -limit (the clear value), kTileMixed = anything else / unknown
// integrate() clears only inactive tiles with cls != kTileMinus and computes only active ones, so a frame's volume traffic
// follows the occupied bricks instead of the whole volume (the reference clears everything, :249-250).
// (An empty-space pyramid over these classes for the raymarch was built and measured: it loses)
constexpr uint8_t kTileMinus = 0, kTileMixed = 2;
constexpr uint32_t kNoSlot = 0xffffffffu;
struct TileState {
  uint32_t* stamp;     // per integrated tile: the frame number that last put it on the active list (dedupes the scatter of k_classify_lists)
  uint8_t* cls;        // owned tiles only (points into Volume::cls at the first owned layer)
  uint32_t* list;      // compacted active tile ids of THIS frame (unordered)
  uint32_t* count;     // device scalar
  const uint32_t* prev_list;   // the active list of the previous integrate(): the only tiles that can hold anything but the clear value
  const uint32_t* prev_count;
  uint32_t* next_count;        // = prev_count's word: re-armed (zeroed) by the integrate kernel for the next frame
  int n;               // owned tiles
  int uniform;         // every tile lies inside exactly one brick's voxel list: tile active => all its voxels drawn
};

// Occupancy bricks (inc_bricks.glsl:10-20) plus the voxel -> brick tables that restate
// VolumeSampler::containedVoxels (volume_sampler.cpp:50-62): along axis a voxel v lies in bricks
// [first[a][v], first[a][v] + count[a][v]).
struct Bricks {
  uint32_t* counters;       // per brick
  uint8_t* flags;           // counter >= min_voxels (recon_integration.cpp:436)
  uint32_t* num_occupied;   // device scalar: the count of the latest updateOccupiedBricks() (one of two words used alternately, so that
                            // clearOccupiedBricks() leaves the list of the last update intact, as the reference's host vector is)
  uint32_t* occupied;       // compacted ids of the occupied bricks (Occupied SSBO, inc_bricks.glsl:18-20), unordered
  const uint16_t* vox_first[3];
  const uint8_t* vox_count[3];
  const uint16_t* tile_b0[3];   // per storage tile index along an axis: first / last brick whose voxel list reaches into it
  const uint16_t* tile_b1[3];   // (b0 > b1: none)
  const uint8_t* tile_full[3];  // per storage tile index along an axis: 1 = every voxel coordinate of the tile is in at least one brick's list
  const uint16_t* brick_t0[3];  // the inverse: per brick index along an axis, first / last storage tile its voxel list reaches into
  const uint16_t* brick_t1[3];  // (t0 > t1: the brick holds no voxel)
  int res[3];               // brick grid
  int n;
  float size[3];            // world brick size
  float bbox_min[3];
};

// Projection cache (round 3).  texture(cv_xyz_inv[i], voxel centre).xyz -- the (u, v, z) a voxel projects to in stream i,
// tsdf_integration.vs:31 -- depends on the calibration volume and the voxel grid only, never on the frame.  The LDS form of the
// integrate kernel recomputes it every frame (texel box -> LDS -> X pass -> Y pass -> z lerp: ~8 dependent round trips and ~17
// workgroup barriers per tile); with 288 GB of HBM it is cheaper to keep most of it.  What is kept per (tile, stream) is the state
// after the Y pass: the tile's x- and y-filtered LUT planes, dz_max planes of 8 x 8 float3 (the z filter of a voxel then is ONE lerp
// of two of them -- the same operands, the same operation as the LDS form's last step, so the same bits).  dz planes instead of 8
// voxel planes: 2.2 - 3.7 KiB instead of 6 KiB per tile and stream at the BASELINE sizes.  Slots are dealt on first use
// (slot[stored tile]) and filled by the LDS kernel itself while it integrates the tile (write-through); from then on the tile is the
// cached kernel's: per wave one z-plane of 64 voxels -- coalesced 768-byte plane reads, image gathers, fusion rule, 256-byte store.
// No LUT texel, no LDS, no barrier.
constexpr uint32_t kItemFresh = 0x80000000u;   // items[w] >= kItemFresh: not (yet) cached -- the LDS kernel's work; kItemFresh | slot: ... and it fills `slot`
constexpr uint32_t kItemNone = 0xffffffffu;    // no slot (pool exhausted)
struct ProjCache {
  float* data;             // pool: slot s at s * slot_floats; inside: [stream][plane < dz_max][8 x 8 voxels (x fastest)][3]
  uint32_t* slot;          // per STORED tile: its slot, or kNoSlot
  uint32_t* alloc;         // device scalar: slots handed out so far
  uint32_t cap;            // pool capacity in slots
  uint32_t slot_floats;    // N * dz_max * 192
  uint32_t dz_max;         // the most LUT z-planes any tile of the volume touches in any stream (fit_lut_to_volume, abi.cpp)
  uint32_t* items;         // per work item of this frame's launch: slot (cached), kItemFresh | slot (to be filled now), kItemNone
  uint32_t* n_slow;        // device scalar: work items of this frame the LDS kernel must take (0: it returns at once)
  uint32_t* n_slow_next;   // the other of the two alternating words, zeroed by this frame's pair-mask pass for the next frame
  int inv_rz[TSDF_MAX_STREAMS];   // z resolution of each stream's inverse LUT (the cached kernel's only use of the calibration)
};

struct Mat4 { float m[16]; };   // column-major
struct ViewParams {
  Mat4 mv, proj, mv_inv, v2w_inv, img_to_eye, normal, mv_v2w, glnormal_inv;
  float cam_vol[3], cam_world[3];
  int w, h;
  int shade_mode;
  int skip;
  // side-by-side stereo (kinect_client.cpp:637-664): the GL viewport's origin (gl_FragCoord = origin + pixel + 0.5) and the shader's
  // viewport_offset uniform (tsdf_raymarch.fs:70,388-389; setViewportOffset, recon_integration.cpp:527)
  int vp_org[2];
  float vp_off[2];
};

// ViewLod atlas (view_lod.cpp:24-61)
struct Atlas {
  float4* color;
  float* depth;
  int aw, h;          // atlas size (1.5 w, h)
  int num_lods;
  int off[TSDF_MAX_LODS][2];
  int res[TSDF_MAX_LODS][2];
};

// image pre-processing (k_preprocess.hip)
struct PreParams {
  int W, H, N;
  float cv_min[TSDF_MAX_STREAMS], cv_max[TSDF_MAX_STREAMS];   // CalibVolumes::getDepthLimits
  float cam[TSDF_MAX_STREAMS][3];                              // CalibVolumes::getCameraPositions
  float bbox_min[3], bbox_max[3];
  int filter_textures, refine;
  // 8-bit wire depth: compress = isCompressedDepth(); uniforms near / scale / scaled_near (NetKinectArray.cpp:343-349)
  int compress[TSDF_MAX_STREAMS];
  float dc_near[TSDF_MAX_STREAMS], dc_scale[TSDF_MAX_STREAMS], dc_scaled_near[TSDF_MAX_STREAMS];
};
struct PreBuffers {
  const float* raw;       // [N][H][W] metres
  float* depth2;          // morph output
  const float* fdepth;    // what the filter pass samples: depth2 or raw (use_processed_depth)
  float2* depth_rg;       // filter output (normalised depth, range quality)
  float4* lab;            // filter output, Lab colour
  float2* depth_b;        // boundary output
  float4* normal;         // normal output
  float4* dqs;            // packed {depth.r, quality, silhouette, 0}
  float* depth_plane;
  // (round 4) the 16 x 16 blocks that hold a boundary candidate: the filter pass numbers them (blk_flag = 1 + position in cand_list, 0 = none; cand_count zeroed by the
  // morph launch), the boundary pass runs them FIRST (their chain -- Lab tile, then the colour comparisons -- is what its launch waits for).  Null: no list.
  uint32_t* blk_flag; uint32_t* cand_list; uint32_t* cand_count; uint32_t cand_cap;
};
// point back-end (k_points.hip)
struct PointParams {
  Mat4 pmv;                     // P * MV, formed in double, rounded once
  float bbox_min[3], bbox_max[3];
  const float4* normals;        // [N][H][W] kinect_normals (xyz), may be null
};
void launch_draw_points(hipStream_t st, const ViewParams& P, const PointParams& Q, const StreamTable& T, const FrameImages& F, unsigned long long* key,
                        float4* fb_c, float* fb_d);

void launch_draw_trigrid(hipStream_t st, const ViewParams& P, const PointParams& Q, const StreamTable& T, const FrameImages& F, float min_length, uint32_t* zbuf,
                         float4* acc, float4* fb_c, float* fb_d);
void launch_tri_clear(hipStream_t st, uint32_t* zbuf, float4* acc, int n);                                       // (k_trigrid.hip, shared with MVT)
void launch_tri_normalize(hipStream_t st, const uint32_t* zbuf, const float4* acc, int n, float4* fb_c, float* fb_d);
// MVT back-end (k_mvt.hip): raw depth [N][H][W] metres -> per-vertex (filtered depth, lateral quality) vtx [N][W+1][H+1] -> framebuffer
void launch_draw_mvt(hipStream_t st, const ViewParams& P, const PointParams& Q, const StreamTable& T, const FrameImages& F, const float* raw, float min_length,
                     float2* vtx, uint32_t* zbuf, float4* acc, float4* fb_c, float* fb_d);

// overlays of the client's draw3d() (k_overlay.hip): "Draw TSDF" (kinect::ReconCalibs::draw) and "Draw frustums" (Frustum::draw)
struct OverlayView { Mat4 mv, proj; int w, h; };   // the head of every overlay's parameters: the caller's matrices and the view's size
struct CalibVisParams {
  Mat4 v2w;                     // vol_to_world as recon_calibs.cpp:38-45 builds it in fp32
  OverlayView view;
  int gres[3];                  // the point grid: stream 0's inverse LUT resolution (CalibVolumes::getVolumeRes)
  float step[3];                // 1.0f / gres (volume_sampler.cpp:33-35)
  int skip;                     // 1: a workgroup whose taps lie in kTileMinus tiles only is discarded whole (the clear value is <= -0.01)
  unsigned long long* skipped;  // device counter: grid points removed by that test
};
struct FrustumParams {
  OverlayView view;
  float corner[TSDF_MAX_STREAMS][8][3];   // getCornerPoints of each stream's cv_xyz (CalibVolumes.cpp:98-113)
  float cam[TSDF_MAX_STREAMS][3];         // Frustum::getCameraPos
  int n;
};
constexpr float kCalibVisLimit = 0.01f;   // recon_calibs.cpp:20 (static; not the context's setTsdfLimit value)
void launch_draw_calibvis(hipStream_t st, const CalibVisParams& Q, const Volume& V, unsigned long long* key, float4* fb_c, float* fb_d);
void launch_draw_frustums(hipStream_t st, const FrustumParams& Q, unsigned long long* key, float4* fb_c, float* fb_d);
// ... and the two after them: the bounding-box wireframe (gloost::BoundingBox::draw) and the texture view (TextureBlitter::blit)
struct BBoxParams {
  OverlayView view;
  float lo[3], hi[3];           // bbox_min / bbox_max as configured (g_bbox)
};
struct BlitParams {
  const float4* src;            // unit 15: the hole-filling atlas (RGBA32F); unit 16: the depth-limit peels (bits, see k_blit_texture)
  int peels;                    // 1: src is the peel image
  int sw, sh;                   // the source's size
  int vw, vh;                   // the blit viewport (0, 0, vw, vh)
  int fw;                       // framebuffer row length
};
void launch_draw_bbox(hipStream_t st, const BBoxParams& Q, unsigned long long* key, float4* fb_c, float* fb_d);
// the occupied-brick wireframes (ReconIntegration::drawOccupiedBricks): the list and count of B as the latest update left them
struct BrickWireParams { OverlayView view; };
void launch_draw_brickwire(hipStream_t st, const BrickWireParams& Q, const Bricks& B, unsigned long long* key, float4* fb_c, float* fb_d, bool plain);
void launch_blit_texture(hipStream_t st, const BlitParams& Q, float4* fb_c);
// the GUI's "Show textures" windows (tsdf_draw_sensor_texture): what the layer's texel is and how it becomes the sample's vec4
enum SensorTexMode {
  kSensorRgba8 = 0,       // uchar4, LINEAR, rgba / 255
  kSensorRgNearest,       // float2, NEAREST, (r, g, 0, 1)
  kSensorSlotDepth,       // the frame slot's packed texel, NEAREST, (depth.r, 0, 0, 1)
  kSensorSlotQuality,     // the frame slot's packed texel, LINEAR, (q, q, q, 1)
  kSensorSlotSilhouette,  // the frame slot's packed texel, LINEAR, (s, 0, 0, 1)
  kSensorRgb32f,          // float4 (rgb padded to 16 B), LINEAR, (rgb, 1)
  kSensorLumNearest       // float, NEAREST, (L, L, L, 1)
};
struct SensorTexParams {
  const void* src;              // first texel of the LAYER (the plain arrays); the packed-texel modes read F / layer instead
  int mode, layer;
  int sw, sh;                   // the source's size
  int x0, y0, nx, ny;           // the launch's pixel rectangle: a superset of quad, scissor box and view (every lane tests its own pixel)
  int sx0, sy0, sx1, sy1;       // scissor box cut to the view: columns [sx0, sx1), GL window rows [sy0, sy1)
  float pmin[2], pmax[2];       // the image quad in ImGui coordinates
  int fw, fh;                   // the framebuffer
};
void launch_sensor_texture(hipStream_t st, const SensorTexParams& Q, const FrameImages& F, float4* fb_c);
// the 8 corner texels of a forward volume [rz][ry][rx][3] in getCornerPoints order (calib_inverter.cpp)
void frustum_corners(const float* cv_xyz, const uint32_t res[3], float out[8][3]);

// inverse calibration volume builder (k_inverter.hip)
struct InverterGrid {
  uint32_t rx, ry, rz, n;     // forward volume resolution, sample count
  int g[3];                   // uniform grid over the samples
  double gmin[3], cell[3], inv[3];
};
struct InverterQuery {
  uint32_t res[3];            // output resolution
  float start[3], step[3];    // sample_start, sample_step (calibration_inverter.cpp:74-78)
  float plane[6][4];          // kinect::Frustum planes
};
void launch_inverter_build(hipStream_t st, const InverterGrid& G, const float* xyz, uint32_t* count, uint32_t* start, uint32_t* sums, float4* sorted);
void launch_inverter_query(hipStream_t st, const InverterGrid& G, const InverterQuery& Q, const float* xyz, const uint32_t* start, const float4* sorted, float4* out);

// one wire message in HBM: per sensor [colour: cs bytes][depth], rec bytes per sensor (k_ingest.hip)
struct WireLayout {
  const uint8_t* msg;
  uint32_t rec, cs;
  int n, cw, ch, w, h;
  int cfmt, dfmt;         // TSDF_COLOR_* / TSDF_DEPTH_*
};
void launch_wire_unpack(hipStream_t st, const WireLayout& L, uchar4* rgba, float* raw);
// the passes of processTextures() as a set of bits; kPreRelayout: the colour re-layout layers of the morph kernel alone (no depth layer)
enum : unsigned { kPreMorph = 1, kPreFilter = 2, kPreBoundary = 4, kPreNormal = 8, kPreQuality = 16, kPreRelayout = 32, kPreAll = 31 };
// launches the passes of `passes` in the order above.  ranges: the frame slot's 8x8-pixel range cells (written by the last pass), or null;
// rgb -> rgba (n_color_px pixels): the frame's colour re-layout, riding along in the morph launch (or launched alone: kPreRelayout), or null
void launch_preprocess(hipStream_t st, const PreParams& P, const PreBuffers& B, const StreamTable& T, const FrameImages& F, const Bricks& BR, float4* ranges,
                       unsigned passes, const uint8_t* rgb = nullptr, uchar4* rgba = nullptr, size_t n_color_px = 0);
void launch_pre_lab(hipStream_t st, const PreParams& P, const PreBuffers& B, const StreamTable& T, const FrameImages& F);   // PreBuffers::lab, on request

// launchers (one per kernel family, defined in the .hip files)
void launch_pack_color(hipStream_t st, const uint8_t* rgb, uchar4* rgba, size_t n);
void launch_frame_ranges(hipStream_t st, const float4* dqs, int n_streams, int w, int h, float4* ranges);
// pack_frame + frame_ranges (+ pack_color when rgb != nullptr) as one launch; rgb / rgba must be readable / writable up to a multiple of 4 pixels
void launch_pack_frame_fused(hipStream_t st, const float* depth_rg, const float* quality, const float* silhouette, float4* dqs, float* depth, float4* ranges,
                             int n_streams, int w, int h, const uint8_t* rgb, uchar4* rgba, size_t n_color_px,
                             uint32_t* zero = nullptr, uint32_t zero_words = 0);   // zero: a word buffer (multiple of 4 words) the launch clears as well (the coming frame's brick counters)
void launch_fill_u32(hipStream_t st, uint32_t* p, uint32_t v, size_t n);
struct PeelClear;
void launch_mark_bricks(hipStream_t st, const StreamTable& T, const FrameImages& F, const Bricks& B, uint32_t* zero_word = nullptr, const PeelClear* pc = nullptr);   // zero_word: a device word the launch clears as well; pc: peel tiles to reset (one more layer of blocks)
void launch_update_occupied(hipStream_t st, const Bricks& B, uint32_t min_voxels, uint32_t* next_count);
// full_classify: 1 = walk every tile (first frame, after anything that may have left non-clear data outside the previous active
// list); 0 = scatter from the occupied bricks + check the previous list only (work follows the scene, not the volume)
// PeelClear: the peel-tile reset of the coming draw (k_raymarch.hip's k_clear_peel_tiles) rides along in the k_classify_lists launch
// ... and so does the zeroing of the spare brick-counter buffer (`zero`, in 16-byte units of zero_words / 4)
struct PeelClear { uint4* peels; const uint8_t* touched_prev; int w, h, ntx, n_tiles; uint32_t* zero; uint32_t zero_words; };   // null pointers: nothing to do
// one integrate(): the tile classification (culled volumes only), the pair-mask pass (plan.pair_pass only) and the integrate kernel(s), one launcher
// each; `plan` (launch_plan.hpp) says which kernel and which grid.  tile_bounds: per (stored tile, stream) 2 x float4 LUT-box bounds (launch_tile_bounds);
// pair_masks: per work item the frame's pair classes; work_recs: per work item the 16-byte record of k_integrate_tiles_rec, then (after all records)
// the tiles' per-voxel bits; proj: the projection cache -- each read only where the plan uses it
void launch_classify_tiles(hipStream_t st, const Volume& V, const Bricks& B, const TileState& S, bool full_classify, uint32_t frame_stamp, const PeelClear& pc);
void launch_pair_masks(hipStream_t st, const StreamTable& T, const FrameImages& F, const Volume& V, const Bricks& B, const TileState& S, const IntegratePlan& plan,
                       const float4* tile_bounds, uint32_t* pair_masks, const ProjCache* proj, uint4* work_recs);
void launch_integrate_tiles(hipStream_t st, const StreamTable& T, const FrameImages& F, const Volume& V, const Bricks& B, const TileState& S, const IntegratePlan& plan,
                            const uint32_t* pair_masks, const ProjCache* proj, const uint4* work_recs);
// [work items, cached items, (tile, stream) pairs of cached items evaluated per voxel, items taken by the LDS kernel] of the last launch -> out[4] (device)
void launch_item_stats(hipStream_t st, const StreamTable& T, const TileState& S, int use_bricks, const uint32_t* pair_masks, const ProjCache& PC, uint32_t* out);
void launch_tile_bounds(hipStream_t st, const StreamTable& T, const Volume& V, float4* bounds);
int integrate_box_cap();
int integrate_row_cap();
void launch_mark_all_mixed(hipStream_t st, const TileState& S);
void launch_volume_to_linear(hipStream_t st, const Volume& V, float* linear);
void launch_volume_from_linear(hipStream_t st, const Volume& V, const float* linear);
void launch_clear_peels(hipStream_t st, float4* peels, int n);   // every peel to the clear value (1,0,1,0)
void launch_depth_limits(hipStream_t st, const ViewParams& P, const Bricks& B, float4* peels, uint8_t* touched_cur = nullptr, const uint8_t* touched_prev = nullptr,
                         int already_cleared = 0);
struct LongRay { uint32_t pix, n, max_n; float prev; float x, y, z, pad; };   // state of a ray handed to k_march_long
struct RayTarget {
  float4* color; float* depth; int stride; float* nsamples; const float4* peels; float clear[4];
  // 8x8-pixel tile history (k_raymarch.hip); null = none.  touched_prev: the previous draw's tiles (its sample counts), touched_prev_target:
  // the tiles of the draw that last wrote THIS target (the previous one, or the one before when two pyramids alternate), touched_recycle:
  // the oldest mask, zeroed for the next draw; rewrite_target / rewrite_all: no valid history for the target / for the sample counts
  const uint8_t* touched_cur; const uint8_t* touched_prev; const uint8_t* touched_prev_target; uint8_t* touched_recycle; int rewrite_all, rewrite_target;
  uint8_t* fill_mask;   // (nullable) per tile: touched by this draw or one of the two before -- what the hole filling of this draw has to look at
};
// one draw's march and shading, as `plan` (launch_plan.hpp) names them
void launch_march(hipStream_t st, const ViewParams& P, const Volume& V, const RayTarget& R, const MarchPlan& plan, void* hit_list, uint32_t* hit_counters, int parity,
                  void* long_list);
void launch_shade(hipStream_t st, const ViewParams& P, const StreamTable& T, const FrameImages& F, const Volume& V, const RayTarget& R, const MarchPlan& plan,
                  const void* hit_list, uint32_t* hit_counters, int parity, const void* long_list);
// hit_list: 16 B per view pixel; long_list: 32 B per view pixel (rays handed to the wave-per-ray pass after `cap` samples);
// hit_counters: 4 words [hit, hit', long, long'], the primed ones re-armed for the next frame by k_shade
void launch_inpaint_level(hipStream_t st, const Atlas& A, int lod);
// tile_mask (nullable): one byte per 8x8-pixel level-0 tile -- only tiles it flags (and what depends on them) are computed; lvl_mask: scratch
void launch_inpaint_pyramid(hipStream_t st, const Atlas& A, const uint8_t* tile_mask = nullptr, uint8_t* const lvl_mask[2] = nullptr);
// mask: Reconstruction::m_color_mask_mode (0 all channels, 1 red only, 2 green + blue only: glColorMask, recon_integration.cpp:321-333);
// keep_color: the colour buffer was NOT cleared before this draw (the anaglyph's second eye, kinect_client.cpp:627)
void launch_colorfill(hipStream_t st, const Atlas& A, int w, int h, float4* fb_color, float* fb_depth, int mask = 0, int keep_color = 0, const uint8_t* tile_mask = nullptr);
// fill_holes off with a colour mask / an uncleared colour buffer: the march renders into the atlas' level-0 region and this merges it
void launch_resolve_masked(hipStream_t st, const Atlas& A, int w, int h, float4* fb_color, float* fb_depth, int mask, int keep_color);
// frame read-out (k_present.hip): the framebuffer colour as RGBA8 (format 0: w * h * 4 bytes) or DXT1 blocks (1: ceil(w/4) * ceil(h/4) * 8 bytes) into out
void launch_present(hipStream_t st, const float4* fb_c, void* out, int w, int h, uint32_t format, int top_down);
// mesh extraction (k_mesh.hip): per-tile scratch of one extract, sized by the launchers' caller.  These launchers: whole-volume contexts only, tile id = stored tile index.
struct MeshGeometry { float bbox_min[3], bbox_max[3]; };
// The lattice of a level of detail (tsdf_mesh_extract_lod): lattice point (i, j, k) of level L is voxel (i, j, k) << L, cr = ceil(res / (1 << L)) points
// per axis, tiles of 8^3 lattice points.  Level 0 is the voxel grid and its storage tiles.  A lattice tile's id is (tz * nty + ty) * ntx + tx.
constexpr int kMeshMaxLevel = 2;
struct MeshLattice {
  int level;
  int cr[3];            // lattice points per axis
  int ntx, nty, ntz;    // lattice tiles per axis
};
__host__ __device__ inline MeshLattice mesh_lattice(const int res[3], int level) {
  MeshLattice L;
  L.level = level;
  for (int a = 0; a < 3; ++a) L.cr[a] = (res[a] + (1 << level) - 1) >> level;
  L.ntx = (L.cr[0] + 7) >> 3; L.nty = (L.cr[1] + 7) >> 3; L.ntz = (L.cr[2] + 7) >> 3;
  return L;
}
struct MeshScratch {
  uint2* tile_cnt;                  // per tile {vertices, triangles}
  uint8_t* tile_skip;               // per tile: 1 = skipped by its class (no voxel read)
  uint32_t* tile_vbase;             // exclusive scan of the vertex counts
  unsigned long long* tile_tbase;   // ... of the triangle counts
  uint32_t* tile_rec;               // compact slot of a tile with surface in the record pool, or kNoSlot
  void* sums;                       // mesh_scan_blocks(n_tiles) + 1 entries of 4 x uint64: per-block prefixes, then the totals {vertices, triangles, tiles with surface, tiles skipped}
  int n_tiles;                      // lattice tiles of `level`: ntx * nty * ntz of mesh_lattice(res, level)
  int level;                        // 0 .. kMeshMaxLevel: which instantiation the launchers take
};
int mesh_scan_blocks(int n_tiles);
void launch_mesh_count(hipStream_t st, const Volume& V, const MeshScratch& S);
void launch_mesh_scan(hipStream_t st, const MeshScratch& S);   // three launches: block sums, scan of the block sums, add
// records: 512 words per tile with surface; nrm / col may be null (attribute not wanted; T and F are read for colours only)
void launch_mesh_emit(hipStream_t st, const Volume& V, const StreamTable& T, const FrameImages& F, const MeshGeometry& G, const MeshScratch& S, uint32_t* records,
                      float* pos, float* nrm, float* col, uint32_t* tri);
// a Z-slab's part of the mesh (k_mesh_slab.hip): the scratch then covers n_own + n_seam slab-local tiles -- the owned lattice tile layers from layer0 on,
// then the ntx * nty tiles of the first layer above them (n_seam = 0 when the slab reaches the volume's top) -- and launch_mesh_scan runs over all of them
struct MeshSlab { int layer0, n_own, n_seam; };
void launch_mesh_slab_count(hipStream_t st, const Volume& V, const MeshScratch& S, const MeshSlab& B);
// records: 512 words per tile with surface, seam tiles included; pos / nrm / col: the owned tiles' vertices (nrm / col may be null)
void launch_mesh_slab_vertices(hipStream_t st, const Volume& V, const StreamTable& T, const FrameImages& F, const MeshGeometry& G, const MeshScratch& S, const MeshSlab& B,
                               uint32_t* records, float* pos, float* nrm, float* col);
// the owned tiles' triangles with indices base + (slab-local index); a seam tile's vertices start at base + slab_vertices + above[tile] (above: n_seam
// words in device memory, not read when n_seam == 0).  The caller has checked that every index fits 32 bits.
void launch_mesh_slab_triangles(hipStream_t st, const Volume& V, const MeshScratch& S, const MeshSlab& B, const uint32_t* records, uint32_t base, uint32_t slab_vertices,
                                const uint32_t* above, uint32_t* tri);
// mesh streaming (tsdf_mesh_stream): a frame's header as k_mesh_stream_header leaves it in the slot's device buffer, and as the copy stream brings it to
// the host -- 64 bytes in front of the payload.  The emit kernels read the needs and the capacities from it and return at once when one is exceeded.
struct MeshStreamHeader {
  unsigned long long needed_vertices, needed_triangles, needed_tiles, n_vertices, n_triangles, tiles_skipped;
  uint32_t max_vertices, max_triangles, max_tiles, overflow;
};
static_assert(sizeof(MeshStreamHeader) == 64, "the payload follows the header at a 64-byte offset");
void launch_mesh_stream_header(hipStream_t st, const MeshScratch& S, MeshStreamHeader* H, uint32_t max_vertices, uint32_t max_triangles, uint32_t max_tiles);
// flags: TSDF_MESH_NORMALS | TSDF_MESH_COLOURS; payload: packed vertices (8 bytes each, 16 with a flag), then the triangles
void launch_mesh_stream_emit(hipStream_t st, const Volume& V, const StreamTable& T, const FrameImages& F, const MeshGeometry& G, const MeshScratch& S, uint32_t flags,
                             const MeshStreamHeader* H, uint32_t* records, void* payload);
// The tile-local triangle format (TSDF_MESH_INDEX_TILE16; the header's "mesh streaming: compact triangles"): a table row per lattice tile with a vertex,
// three 16-bit corner codes per triangle; three launches (packed vertices, table, triangles).  raw_table == nullptr: the payload is vertices, padding to
// 16, needed_tiles rows, the 6-byte triangles.
// raw_table != nullptr (the filter's raw frame): the payload is the uint32 frame launch_mesh_stream_emit writes, and the rows go to raw_table.
struct MeshTileRow { uint32_t tile, first_vertex, first_triangle, n_triangles; };
static_assert(sizeof(MeshTileRow) == 16, "tsdf_mesh_tile_row");
void launch_mesh_stream_emit_compact(hipStream_t st, const Volume& V, const StreamTable& T, const FrameImages& F, const MeshGeometry& G, const MeshScratch& S, uint32_t flags,
                                     const MeshStreamHeader* H, uint32_t* records, void* payload, MeshTileRow* raw_table);
// ... its table launch alone: the rows of S's first n tiles, the first of them first_tile in the level's grid (k_mesh.hip; launch_mesh_part_emit uses it too)
void launch_mesh_stream_table(hipStream_t st, const MeshScratch& S, const MeshStreamHeader* H, int n, uint32_t first_tile, void* payload, uint32_t stride, MeshTileRow* raw_table);
// A Z-slab's part of the tile-local frame (k_mesh_slab.hip; the header's "mesh streaming: slab parts"): behind launch_mesh_slab_count and launch_mesh_scan
// over B.n_own + B.n_seam tiles.  The header counts the OWNED tiles' vertices and surface tiles; what the seam tiles added to the scan's totals goes into the
// 64-byte record in front of it (one copy takes both, as with the filter's record).  records: 512 words for each of max_tiles + B.n_seam tiles.
struct MeshStreamPartRecord { unsigned long long seam_tiles, seam_vertices, reserved[6]; };
static_assert(sizeof(MeshStreamPartRecord) == 64, "the header stays 64 bytes in front of the payload");
void launch_mesh_part_header(hipStream_t st, const MeshScratch& S, const MeshSlab& B, MeshStreamPartRecord* record, MeshStreamHeader* H, uint32_t max_vertices,
                             uint32_t max_triangles, uint32_t max_tiles);
void launch_mesh_part_emit(hipStream_t st, const Volume& V, const StreamTable& T, const FrameImages& F, const MeshGeometry& G, const MeshScratch& S, const MeshSlab& B,
                           uint32_t flags, const MeshStreamHeader* H, uint32_t* records, void* payload);
// the streamed filter (k_mesh_stream_filter.hip; tsdf_mesh_stream_config_filter with min_triangles >= 1): the emit writes the unfiltered frame into `raw`
// (a header, the capacity-sized payload behind it: device only, one per configuration), the filter's launches move what stays into a slot's payload and
// write the slot's header and record.  Every launch is sized by the capacities and reads the frame's counts from the raw header.
struct MeshStreamFilter {
  MeshStreamHeader* raw;
  uint32_t* parent;                 // max_vertices words: the forest, behind the flatten the kept vertices' new indices
  uint32_t* label;                  // max_vertices words: the smallest vertex index of the vertex's component
  uint32_t* count;                  // max_vertices words: at a root, its component's triangles
  uint8_t* keep;                    // max_vertices bytes rounded up to 4
  unsigned long long* vertex_sums;  // mesh_stream_filter_scan_words(max_vertices): block prefixes of the kept vertices, then their total
  unsigned long long* triangle_sums;   // ... (max_triangles)
  uint32_t* words;                  // {components, components kept, table rows kept (tile-local format)}
  uint32_t max_vertices, max_triangles, min_triangles, stride;
  // the tile-local format only (null / 0 otherwise): the raw frame's tile table (max_tiles rows, device only), per four triangles the kept triangles
  // before them inside their scan block, and the level's lattice tiles per axis
  MeshTileRow* raw_table;
  uint16_t* tri_local;              // (max_triangles + 3) / 4 words
  int ntx, nty;
};
// what travels to the host in front of a filtered slot's header: out[4] of tsdf_mesh_stream_frame_filter
// (table_rows: the filtered frame's tile-table rows in the tile-local format, 0 otherwise)
struct MeshStreamFilterRecord { unsigned long long components, kept, vertices_removed, triangles_removed, table_rows, reserved[3]; };
static_assert(sizeof(MeshStreamFilterRecord) == 64, "record and header travel as one 128-byte copy; the payload stays 64 bytes behind the header");
size_t mesh_stream_filter_scan_words(uint32_t capacity);
void launch_mesh_stream_filter(hipStream_t st, const MeshStreamFilter& F, void* payload);   // everything up to the scatter
void launch_mesh_stream_filter_header(hipStream_t st, const MeshStreamFilter& F, MeshStreamHeader* H, MeshStreamFilterRecord* record);
// mesh components (k_mesh_components.hip): the mesh arrays alone are read, so neither the volume nor a level appears.  Every scan works on `sums`:
// mesh_cc_scan_blocks(n) + 1 64-bit words for n elements, the last of them the total once the launcher's work is done.
struct MeshArrays { float* pos; float* nrm; float* col; uint32_t* tri; };   // nrm / col: null where the extract produced none
int mesh_cc_scan_blocks(size_t n);
// union-find over parent[nv] (scratch), label[v] = the smallest vertex index of v's component, sums (of nv) = the roots' scan: sums[blocks] = components
void launch_mesh_cc_label(hipStream_t st, const uint32_t* tri, uint32_t nv, size_t nt, uint32_t* parent, uint32_t* label, unsigned long long* sums);
// vertex_component: the labels on entry, the component indices on return; rank: nv words of scratch (parent may serve again); table: n_components
// entries, written whole; largest: one word, zero on entry, the largest n_triangles on return
void launch_mesh_cc_number(hipStream_t st, const uint32_t* tri, uint32_t nv, size_t nt, const unsigned long long* sums, uint32_t n_components, uint32_t* rank,
                           uint32_t* vertex_component, uint32_t* triangle_component, tsdf_mesh_component* table, uint32_t* largest);
void launch_mesh_cc_keep_from_table(hipStream_t st, const tsdf_mesh_component* table, uint32_t n_components, uint32_t min_triangles, uint8_t* keep);
// the kept counts: vertex_sums[blocks(nv)] and triangle_sums[blocks(nt)] ...
void launch_mesh_cc_keep_count(hipStream_t st, const uint8_t* keep, const uint32_t* vertex_component, const uint32_t* triangle_component, uint32_t nv, size_t nt,
                               unsigned long long* vertex_sums, unsigned long long* triangle_sums);
// ... and the scatter into arrays of exactly those sizes; new_index: nv words of scratch
void launch_mesh_cc_keep_scatter(hipStream_t st, const uint8_t* keep, const uint32_t* vertex_component, const uint32_t* triangle_component, uint32_t nv, size_t nt,
                                 const unsigned long long* vertex_sums, const unsigned long long* triangle_sums, const MeshArrays& src, const MeshArrays& dst,
                                 uint32_t* new_index);
// mesh component measures (k_mesh_component_measures.hip, mesh_measure.hpp): rows: n_components entries, ZERO on entry (the caller's memset on the same
// stream), final on return; packed: nv 64-bit words, written whole.  The caller launches with n_components > 0 (so nv > 0).
struct MeshMeasureGeometry { float bbox_min[3]; double scale; };
void launch_mesh_measures(hipStream_t st, const MeshMeasureGeometry& G, const float* pos, const uint32_t* tri, uint32_t nv, size_t nt, const uint32_t* vertex_component,
                          const uint32_t* triangle_component, uint32_t n_components, unsigned long long* packed, tsdf_mesh_component_measure* rows);
// keep[c] = the rule holds for component c (rows final)
void launch_mesh_measure_keep(hipStream_t st, const tsdf_mesh_component_measure* rows, const tsdf_mesh_component* table, uint32_t n_components,
                              const tsdf_mesh_measure_rule& rule, uint8_t* keep);
// mesh components of a Z-slab's linked part (k_mesh_slab_components.hip).  tri: the part's nt triangles with global indices from `base` on; nv own
// vertices, n >= nv the index space with the span into the slab above.  parent (scratch), label: n words; rank: nv words; down_mark, seam_root: nv bytes,
// zero on entry; each of the four sums: mesh_sc_scan_blocks(of its elements) + 1 64-bit words, the last of them the total.  The caller launches with nv > 0.
struct MeshSlabLabelling {
  const uint32_t* tri; size_t nt; uint32_t nv, n, base;
  uint32_t* parent; uint32_t* label; uint32_t* rank; uint8_t* down_mark; uint8_t* seam_root;
  unsigned long long* root_sums; unsigned long long* up_sums; unsigned long long* down_sums; unsigned long long* seam_sums;
};
int mesh_sc_scan_blocks(size_t n);
// step 1, up to what sizes the lists: root_sums' total = local components, up_sums' = up records, down_sums' = down records.  first_layer_tiles: the
// lattice tiles of the part's first owned layer (S and records: the part's scratch), 0 for a slab at the volume's bottom (no down records)
void launch_mesh_sc_label(hipStream_t st, const MeshSlabLabelling& W, const MeshScratch& S, const uint32_t* records, int first_layer_tiles);
// ... and the rest: local (one row per local component), down, up sized by those totals, roots by down + up; seam_sums' total = root records
void launch_mesh_sc_lists(hipStream_t st, const MeshSlabLabelling& W, tsdf_mesh_component* local, tsdf_mesh_seam_vertex* down, tsdf_mesh_seam_vertex* up,
                          tsdf_mesh_seam_root* roots);
// step 3.  links: n_links records in device memory, checked by the host (mesh_cc_seams.hpp: component_links_check); link_of: nv words of 0xffffffff on
// entry; number: nv words of scratch; sums: blocks(nv) + 1 words, its total = the components the part owns; table: a row per local component at most
void launch_mesh_sc_link(hipStream_t st, const MeshSlabLabelling& W, const tsdf_mesh_component* local, const tsdf_mesh_component_link* links, uint32_t n_links,
                         uint32_t component_base, uint32_t* link_of, uint32_t* number, unsigned long long* sums, uint32_t* vertex_component,
                         uint32_t* triangle_component, tsdf_mesh_component* table);
// ray queries (k_rays.hip): one launch pair serves at most kRayChunk rays -- the capacity of the context's hit list
constexpr uint32_t kRayChunk = 1u << 18;
struct RayCast {
  float bbox_min[3], ext[3];        // vol_to_world: world = bbox_min + u * ext, ext = bbox_max - bbox_min in fp32
  uint32_t flags;                   // TSDF_RAYS_UNIT_CUBE | TSDF_RAY_NORMALS | TSDF_RAY_COLOURS
  uint32_t n;                       // rays of this launch (<= kRayChunk)
  int run;                          // samples per look at the tile classes (ray_run_length)
  float n_cap;                      // the bound on a ray's sample count (ray_sample_cap)
};
struct RayHitRec { float x, y, z; uint32_t ray; };   // a hit's unit-cube position and its ray's number in the launch
// stats: three device words {hits, samples accounted for, samples fetched}, added to; list_count: zero at the launch
void launch_rays_march(hipStream_t st, const Volume& V, const RayCast& Q, const tsdf_ray* rays, tsdf_ray_hit* hits, tsdf_ray_surface* surf, RayHitRec* list,
                       uint32_t* list_count, unsigned long long* stats);
void launch_rays_surface(hipStream_t st, const Volume& V, const StreamTable& T, const FrameImages& F, const RayCast& Q, const RayHitRec* list,
                         const uint32_t* list_count, tsdf_ray_surface* surf);
// the part cast of a Z-slab context (the samples it owns; stats[1] counts those) and the merge of `parts` parts that lie stride_records apart
void launch_rays_march_part(hipStream_t st, const Volume& V, const RayCast& Q, const tsdf_ray* rays, tsdf_ray_hit* hits, tsdf_ray_surface* surf, RayHitRec* list,
                            uint32_t* list_count, unsigned long long* stats);
void launch_rays_merge(hipStream_t st, const tsdf_ray_hit* hit_parts, const tsdf_ray_surface* surf_parts, uint32_t parts, uint32_t n, uint64_t stride_records,
                       tsdf_ray_hit* hits, tsdf_ray_surface* surf);
void launch_view_rays(hipStream_t st, const ViewParams& P, int x0, int y0, int w, int h, tsdf_ray* rays);
// texture taps (k_texture_taps.hip): one launch serves at most kTapsChunk points (texture_taps.hpp), one lane per (point, stream) pair, blockIdx.y = stream
struct TapsLaunch {
  float bbox_min[3], ext[3];        // the ray section's mapping: u = (p - bbox_min) / ext, ext = bbox_max - bbox_min in fp32
  uint32_t flags;                   // TSDF_TAPS_UNIT_CUBE | TSDF_TAPS_SENSOR
  uint32_t n_points;                // points of this launch (<= kTapsChunk)
};
// xyz: the launch's points, 3 floats each; taps / sensor: [point][stream] records (sensor: nullptr without the flag); stats: the kTapStatSlots pairs
// of device words {pairs with quality > 0, pairs not evaluated} (texture_taps.hpp), added to
void launch_texture_taps(hipStream_t st, const StreamTable& T, const FrameImages& F, float limit, const TapsLaunch& Q, const float* xyz, tsdf_texture_tap* taps,
                         tsdf_sensor_tap* sensor, unsigned long long* stats);
// the packed taps of a streamed frame (k_mesh_stream_taps.hip): sized by max_vertices, n_vertices read from the slot's device header H
void launch_mesh_stream_taps(hipStream_t st, const StreamTable& T, const FrameImages& F, float limit, const MeshStreamHeader* H, const uint8_t* vertices,
                             uint32_t stride, uint32_t max_vertices, void* taps);
void launch_clear_image(hipStream_t st, float4* color, float* depth, size_t n, float4 c, float d);
void launch_export_partial(hipStream_t st, const RayTarget& R, int w, int h, void* dst);
void launch_composite(hipStream_t st, const void* gathered, int n, const RayTarget& R, int w, int h);
void launch_export_hits(hipStream_t st, const RayTarget& R, int w, const void* hit_list, const uint32_t* hit_count, const void* long_list, const uint32_t* long_count,
                        void* dst, uint32_t capacity);   // long_list: the second-pass rays of a two-pass march (null: none)
void launch_composite_hits(hipStream_t st, const void* gathered, size_t stride_bytes, int n, const RayTarget& R, int w, int h, unsigned long long* key, int own_counts);

}  // namespace rr
