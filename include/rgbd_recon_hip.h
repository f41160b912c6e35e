/* rgbd_recon_hip.h -- C ABI of the MI355X-native TSDF fusion core (librgbd_recon_hip.so).
 *
 * Drop-in boundary for the per-frame hot path of rgbd-recon: everything
 * kinect::ReconIntegration (framework/reconstruction/recon_integration.hpp:35-103) does on the GL
 * thread -- integrate(), drawF() = drawDepthLimits() + draw() + fillColors(), the brick-occupancy
 * bookkeeping and the setters -- behind plain C entry points.  No C++ or torch types cross this line.
 *
 * Conventions
 *   - every call returns 0 on success, a negative tsdf_status otherwise; tsdf_last_error() gives text.
 *     Nothing throws or aborts across the boundary (reference: exceptions/exit/assert).
 *   - a context is single-threaded; all device work is queued on ONE HIP stream (own, or adopted with
 *     tsdf_set_stream) and is asynchronous until tsdf_sync() or a download.
 *   - host pointers unless the name says `_dev`; matrices are 16 floats column-major exactly as
 *     glGetFloatv(GL_MODELVIEW_MATRIX / GL_PROJECTION_MATRIX) returns them (recon_integration.cpp:183,197).
 *   - volumes are x-fastest, z-outermost (calibration_volume.hpp:57-59, volume_sampler.cpp:39-45);
 *     images are row-major, bottom row first (GL window coordinates), layers outermost.
 *   - GL implicit state of the reference becomes explicit arguments (SURVEY.md §8b "implicit inputs").
 */
#ifndef RGBD_RECON_HIP_H
#define RGBD_RECON_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSDF_MAX_STREAMS 16   /* reference hard-codes 5 (tsdf_integration.vs:13); configs c3/c4 need 8 */
#define TSDF_MAX_LODS 20      /* tsdf_inpaint.fs:11-12 uniform uvec2[20] */

typedef struct tsdf_ctx tsdf_ctx;

typedef enum tsdf_status {
  TSDF_OK = 0,
  TSDF_ERR_INVALID_ARGUMENT = -1,
  TSDF_ERR_HIP = -2,           /* a hip* call failed; message in tsdf_last_error */
  TSDF_ERR_NO_DEVICE = -3,
  TSDF_ERR_STATE = -4,         /* call order violated (e.g. integrate before calibration upload) */
  TSDF_ERR_OUT_OF_MEMORY = -5
} tsdf_status;

/* Replaces the constructor arguments ReconIntegration(cfs, cv, bbox, limit, size)
 * (recon_integration.cpp:30-60) plus what it pulls out of CalibrationFiles (stream count, image sizes,
 * reconstruction.cpp:14-22) and the window size it is resize()d to (:482-500). */
typedef struct tsdf_config {
  uint32_t struct_size;     /* = sizeof(tsdf_config) */
  float bbox_min[3], bbox_max[3];
  float voxel_size;         /* used when res[0] == 0: res = ceil(bbox / voxel_size)   (:340-344) */
  uint32_t res[3];          /* explicit TSDF resolution (benchmark configs), overrides voxel_size */
  float brick_size[3];      /* world units; the reference has one scalar (:53, :462-472); snapped to whole voxels */
  float limit;              /* TSDF truncation, also the raymarch step basis (tsdf_raymarch.fs:34) */
  uint32_t num_streams;
  uint32_t depth_w, depth_h;   /* depth/quality/silhouette arrays (NetKinectArray.cpp:159-178) */
  uint32_t color_w, color_h;   /* colour array (NetKinectArray.cpp:147-157) */
  uint32_t view_w, view_h;     /* viewport (resize(), :482-500) */
  int32_t device;              /* HIP device ordinal */
  /* multi-GPU Z-slab partition: this context owns voxel planes [slab_z0, slab_z1);
   * 0,0 = the whole volume.  Both must be multiples of 8 (storage tile) unless 0 / res_z. */
  uint32_t slab_z0, slab_z1;
  /* 1: this context also integrates the halo tile layers next to its slab itself (voxels are independent in K1), so no
   * halo exchange is needed before the raymarch; 0: the halo is filled by tsdf_halo_unpack_dev from the neighbours. */
  uint32_t slab_recompute_halo;
  /* > 0: sparse tile pool (BASELINE.json configs[4] "sparse-brick allocation"): the TSDF is stored as a pool of this many
   * 8^3-voxel tiles (2 KiB each) plus a tile -> slot table instead of a dense res_x*res_y*res_z array; only tiles that an
   * occupied brick reaches hold storage, every other voxel reads as -limit.  Volumes far beyond dense memory become
   * possible (4096^3 = 256 GiB dense).  Needs brick culling (setUseBricks(true)); with a slab, slab_recompute_halo = 1.
   * A frame that needs more tiles than the pool holds drops the excess (they read -limit): tsdf_sparse_pool_stats. 0: dense. */
  uint32_t sparse_pool_tiles;
  /* Projection cache, OPT-IN (dense storage, culled or dense integrate): texture(cv_xyz_inv[i], voxel centre).xyz of
   * tsdf_integration.vs:31 depends on the calibration and the voxel grid only, so the integrate kernel can keep the x/y-filtered
   * LUT planes of every 8^3-voxel tile in HBM once the tile has been integrated (N x dz x 768 B per tile, dealt on first use) and
   * from then on read them back instead of re-filtering the LUT.  Budget in MiB; 0 = off (default: on MI355X the cached kernel
   * is bound by the same image gathers as the LUT kernel and measured slower).  Tiles beyond the budget keep
   * the LUT path.  Results are bit-identical either way. */
  uint32_t proj_cache_mib;
  /* The lanes of a context (rounds 3 / 4; the reference has ONE GL command stream, recon_integration.hpp:43-49 configures its operator through
   * setters: these fields are their counterpart for what has no setter there).  0 = the default: four HIP streams per context -- the lane ahead
   * (frame re-layout / processTextures, brick passes), the integrate lane, the context's stream (depth limits, march, shade), the fill lane
   * (hole filling, issued by a helper thread) -- with everything the lanes hand over allocated twice.  MEMORY: the integrate lane keeps a SECOND
   * VOLUME SET (volume + tile tables: 4 bytes x voxels again -- 0.5 GiB at 512^3, 4 GiB at 1024^3), allocated at the first tsdf_integrate();
   * TSDF_LANES_NO_INTEGRATE_LANE does without it (integrate() on the context's stream, ~30 % fewer frames/s at 512^3 x 4 streams).  Results are
   * bit-identical in every combination.  tsdf_set_stage_overlap() switches TSDF_LANES_ONE_STREAM at run time.  (The RR_* environment variables
   * the A/B tools use -- RR_OVERLAP_FILL, RR_DEEP, RR_FILL_THREAD, RR_LANES, RR_LANE_PRIORITY -- override these fields when set.) */
  uint32_t lane_flags;
  /* stream priority of {lane ahead, fill lane, integrate lane, context's stream}: -1 high, 0 normal (default), 1 low */
  int32_t lane_priority[4];
} tsdf_config;
#define TSDF_LANES_ONE_STREAM        1u   /* every kernel of a frame on the context's stream, one copy of everything (rounds 1 / 2) */
#define TSDF_LANES_NO_INTEGRATE_LANE 2u   /* integrate() on the context's stream, ONE volume set */
#define TSDF_LANES_NO_FILL_THREAD    4u   /* the fill lane's calls are issued by the calling thread */
#define TSDF_LANES_SHARED_FILL_LANE  8u   /* the lane ahead and the fill lane share one stream */

/* ---- lifetime / errors ------------------------------------------------------------------------- */
int32_t tsdf_create(const tsdf_config* cfg, tsdf_ctx** out);
int32_t tsdf_destroy(tsdf_ctx* ctx);
const char* tsdf_last_error(const tsdf_ctx* ctx);   /* ctx may be NULL: error of the last failed tsdf_create */
/* sparse contexts: tiles the last integrate() needed / pool capacity (synchronises the stream) */
int32_t tsdf_sparse_pool_stats(tsdf_ctx* ctx, uint32_t* tiles_needed, uint32_t* pool_tiles);
/* what the last integrate() launch was made of (synchronises the stream; measurement only): out[0] work items (8^3-voxel tiles),
 * out[1] of them served from the projection cache, out[2] (tile, stream) pairs of those evaluated per voxel (6 KiB of cached
 * coordinates read each), out[3] tiles taken by the LUT kernel, out[4] cache slots in use, out[5] cache capacity in slots.
 * All zero when the context does not use the cache. */
int32_t tsdf_integrate_stats(tsdf_ctx* ctx, uint32_t out[6]);
/* hole filling (fillColors): out[0] passes so far, out[1] of them restricted to the screen tiles the last three draws touched (the
 * default whenever three culled draws in a row left nothing else in the pyramid and the framebuffer; RR_FILL_TILES=0 in the
 * environment at tsdf_create switches it off).  Host counters, no synchronisation. */
int32_t tsdf_fill_stats(tsdf_ctx* ctx, uint64_t out[2]);
int32_t tsdf_set_stream(tsdf_ctx* ctx, void* hip_stream);   /* adopt a caller-owned hipStream_t (NULL: back to own) */
/* adopt the process's NULL ("legacy default") stream, whose handle is 0 and therefore cannot be passed to tsdf_set_stream:
 * torch.cuda.default_stream().cuda_stream is 0, so this is how a context is ordered with work issued on torch's default
 * stream (the reference has one implicit GL command stream; this is its HIP counterpart) */
int32_t tsdf_adopt_null_stream(tsdf_ctx* ctx);
int32_t tsdf_sync(tsdf_ctx* ctx);

/* ---- inputs ------------------------------------------------------------------------------------ */
/* CalibVolumes textures (CalibVolumes.cpp:64-80,132-144): per stream the inverse LUT cv_xyz_inv (RGBA32F,
 * unit 30+i), the colour LUT cv_uv (RG32F, unit 10+2i) and the forward LUT cv_xyz (RGB32F, unit 9+2i).
 * uv / xyz may be NULL when raymarch colouring / brick marking are not used. */
int32_t tsdf_set_calibration(tsdf_ctx* ctx, uint32_t stream,
                             const float* xyz_inv_rgba, const uint32_t res_inv[3],
                             const float* uv_rg, const uint32_t res_uv[3],
                             const float* xyz_rgb, const uint32_t res_xyz[3]);
/* NetKinectArray's processed arrays on texture units 1,2,3,5 (NetKinectArray.cpp:428-449):
 * depth RG32F [N][H][W][2] (r = normalised depth), quality R32F, silhouette R32F, colour RGB8 [N][Hc][Wc][3].
 * colour may be NULL (keeps the previous one).  Normals (unit 4) are not read by the path
 * (GRAD_NORMALS, tsdf_raymarch.fs:46). */
int32_t tsdf_upload_frame(tsdf_ctx* ctx, const float* depth_rg, const float* quality,
                          const float* silhouette, const uint8_t* colour_rgb);

/* The same frame from DEVICE memory (arrays produced on the GPU, or staged there by the caller): no copy, one re-layout launch into a
 * frame slot -- what a new frame costs the path itself; integrate() is handed a new frame every time in the reference
 * (kinect_client.cpp:586-599, NetKinectArray.cpp:225-236).  Pointers aligned to their element size; colour may be NULL.
 *   flags 0                      the arrays are written by work queued on the context's stream: the re-layout is ordered behind it
 *   TSDF_FRAME_ARRAYS_COMPLETE   the arrays are complete when the call is made: the re-layout starts at once, on the context's lane
 *                                ahead (see tsdf_set_stage_overlap), beside the previous frame's kernels
 * The arrays must stay untouched until work queued on the context's stream after the next tsdf_integrate() / draw call runs. */
#define TSDF_FRAME_ARRAYS_COMPLETE 1u
int32_t tsdf_upload_frame_dev(tsdf_ctx* ctx, const float* depth_rg_dev, const float* quality_dev,
                              const float* silhouette_dev, const uint8_t* colour_rgb_dev, uint32_t flags);

/* Asynchronous upload: NetKinectArray keeps the incoming frame in a double-buffered, mapped PBO (framework/double_pixel_buffer.cpp:18-81:
 * the reader thread memcpy's into the back buffer, NetKinectArray.cpp:516-520; update() swaps and starts the PBO -> texture
 * DMA, :225-236).  Here: two device frame slots, a pinned host staging ring and a copy stream.
 *   tsdf_frame_staging       pinned host pointers of the next upload's staging buffer (the mapped back PBO): a producer that
 *                            writes the images there pays no extra host copy.  Blocks while that buffer's previous upload is in flight.
 *   tsdf_upload_frame_async  send the frame to the slot that is NOT current, on the copy stream; returns at once.  NULL (or the
 *                            staging pointer) = "already in the staging buffer"; other pointers are memcpy'd there first.
 *                            with_colour = 0 leaves the slot's colour image as it is.
 *   tsdf_select_frame_slot   make a slot current (update()'s swap): the context's stream waits -- on the GPU -- for the slot's
 *                            upload; everything queued afterwards reads the new frame.  Also switches between two resident
 *                            frames without any upload (tsdf_upload_frame fills the current slot). */
int32_t tsdf_frame_staging(tsdf_ctx* ctx, float** depth_rg, float** quality, float** silhouette, uint8_t** colour_rgb);
int32_t tsdf_upload_frame_async(tsdf_ctx* ctx, const float* depth_rg, const float* quality, const float* silhouette,
                                const uint8_t* colour_rgb, int32_t with_colour);
int32_t tsdf_select_frame_slot(tsdf_ctx* ctx, uint32_t slot);
int32_t tsdf_current_frame_slot(const tsdf_ctx* ctx, uint32_t* slot);

/* ---- calibration volume files (format only): kinect::CalibrationVolume<T>::read / write,
 * framework/calibration/calibration_volume.hpp:30-38,62-78 -- u32 res[3]; f32 depth_min, depth_max; T[res.x*res.y*res.z].
 * texel_floats: 3 for *.cv_xyz (CalibrationVolume<xyz>), 2 for *.cv_uv, 4 for *.cv_xyz_inv (CalibVolumes.cpp:64-80,115-130).
 * Host only, no context; errors: negative status + tsdf_calib_last_error(). */
int32_t tsdf_calib_volume_info(const char* path, uint32_t texel_floats, uint32_t res[3], float depth_limits[2]);
int32_t tsdf_calib_volume_read(const char* path, uint32_t texel_floats, float* data, uint64_t capacity_floats);
int32_t tsdf_calib_volume_write(const char* path, uint32_t texel_floats, const uint32_t res[3], const float depth_limits[2], const float* data);
const char* tsdf_calib_last_error(void);

/* ---- the point back-end behind the same interface: kinect::ReconPoints::draw(),
 * framework/reconstruction/recon_points.cpp:71-111 + glsl/points.{vs,gs,fs}: one depth-tested point sprite per depth pixel
 * and sensor (size 10 / eye distance, 4 in shade mode 3), flat-shaded with the sensor's colour image and normal.
 * Reads what the TSDF path reads (frame, cv_xyz, cv_uv) plus the NetKinectArray normal array: tsdf_process_textures
 * produces it, or upload it with tsdf_upload_normals ([N][H][W][3]).  Result: tsdf_download_framebuffer. */
int32_t tsdf_upload_normals(tsdf_ctx* ctx, const float* normals_rgb);
int32_t tsdf_draw_points(tsdf_ctx* ctx, const float modelview[16], const float projection[16]);
/* kinect::ReconTrigrid::draw(), framework/reconstruction/recon_trigrid.cpp:85-148 + glsl/trigrid_accum.{vs,gs,fs},
 * trigrid_normalize.fs: two triangles per depth-pixel cell and sensor; z pre-pass, quality-weighted blend of all fragments
 * within 0.075 m of the front surface, normalise.  min_length: Reconstruction::m_min_length = CalibrationFiles::minLength()
 * (default 0.0125, KinectCalibrationFile.cpp:96).  Result: tsdf_download_framebuffer. */
int32_t tsdf_set_min_length(tsdf_ctx* ctx, float min_length);
int32_t tsdf_draw_trigrid(tsdf_ctx* ctx, const float modelview[16], const float projection[16]);
/* kinect::ReconMVT::draw(), framework/reconstruction/recon_mvt.cpp:84-150 + glsl/mvt_accum.{vs,gs,fs}, trigrid_normalize.fs: the
 * client's "Trigrid orig" mode (source/kinect_client.cpp:249-253).  Trigrid's passes, but every grid vertex reads the RAW depth of the
 * last raw upload (tsdf_upload_raw_frame / _dev / tsdf_upload_wire_frame; metres, NetKinectArray.cpp:173,191 -- the 8-bit compressed raw
 * array of :170 is not reproduced) through a 13 x 13 bilateral filter (mvt_accum.vs:43-115, depth limits the constants 0.5 / 4.5 m of
 * recon_mvt.cpp:35-36), validSurface rejects depths < 0.5 m and edges >= min_length * avg_depth + 0.005 (mvt_accum.gs:29-41), fragment
 * quality = lateral_quality / depth (mvt_accum.fs:53).  tsdf_process_textures is not needed and tsdf_set_preprocess does not matter.
 * View size, viewport offset, colour mask, min_length (tsdf_set_min_length) and timers ("mvt") as for tsdf_draw_trigrid.
 * Result: tsdf_download_framebuffer.  TSDF_ERR_STATE without a raw frame. */
int32_t tsdf_draw_mvt(tsdf_ctx* ctx, const float modelview[16], const float projection[16]);
/* The last tsdf_draw_mvt's vertex stage (inspection, like tsdf_download_preprocessed): out [N][W+1][H+1][2] = (filtered depth in metres,
 * lateral quality) of grid vertex (gx, gy), gx in [0, H], gy in [0, W] at u = (gx + 0.5) / W, v = (gy + 0.5) / H (the swapped loop bounds
 * of recon_mvt.cpp:53-54).  TSDF_ERR_STATE before the first MVT draw. */
int32_t tsdf_download_mvt_vertices(tsdf_ctx* ctx, float* out);

/* ---- the overlays the client draws after drawF() in mono mode (source/kinect_client.cpp:672-683), each into the framebuffer as the
 * previous draw left it (tsdf_download_framebuffer reads the result; tsdf_upload_framebuffer puts a known one under an overlay), depth
 * func GL_LESS (:983-984), colour and depth written, no blending.  Pixels no fragment passes keep their colour and depth.
 * TSDF_ERR_INVALID_ARGUMENT for a null or singular modelview / projection; TSDF_ERR_STATE with a colour-mask mode != 0 or a viewport
 * origin / offset != 0 (the stereo modes draw no overlay).
 *
 * tsdf_draw_calibvis: "Draw TSDF" (g_draw_calibvis, :420, key V :791) = kinect::ReconCalibs::draw(), recon_calibs.cpp:54-61 with
 *   glsl/calib_vis.{vs,fs}.  One point per cell of a grid of stream 0's inverse LUT resolution (CalibVolumes::getVolumeRes,
 *   CalibVolumes.cpp:90-92, whatever the active sensor), point (x, y, z) at p = ((x + 0.5f) * (1.0f / res.x), ...) in fp32, drawn x fastest,
 *   then y, then z (volume_sampler.cpp:33-45).  d = the TSDF of the latest integrate() at p (trilinear, CLAMP_TO_EDGE; calib_vis.vs:37);
 *   gl_Position = P * (MV * (vol_to_world * (p, 1))), the products in that order (:29-38), vol_to_world = translate(bbox_min) *
 *   scale(bbox_max - bbox_min) in fp32 (recon_calibs.cpp:38-45).  Colour (calib_vis.fs:17-30) with the static limit 0.01
 *   (recon_calibs.cpp:20; not tsdf_set_tsdf_limit's value): inv = |d| / 0.01 (an IEEE division); d > 0 -> (1 - inv, 0, 0, 1), else
 *   (0, 1 - inv, 0, 1); then d >= 0.01 -> (0, 0, 1, 1); d <= -0.01 -> discarded before the depth test.  Timer "calibvis".
 *   TSDF_ERR_STATE without stream 0's cv_xyz_inv and on a Z-slab context (the overlay needs the whole volume).
 * tsdf_set_active_kinect: ReconCalibs::setActiveKinect.  Validates the stream (TSDF_ERR_INVALID_ARGUMENT out of range) and changes no
 *   output: the layer only selects the cv_xyz_inv / cv_xyz lookups of calib_vis.vs:26-27 / .fs:25, which feed nothing the output uses.
 * tsdf_draw_frustums: "Draw frustums" (g_draw_frustums, key F :742) = CalibVolumes::drawFrustums() (CalibVolumes.cpp:214-218) ->
 *   Frustum::draw() (frustum.cpp:45-95), stream after stream: 12 GL_LINES between the 8 corner samples of the stream's forward LUT
 *   (getCornerPoints, CalibVolumes.cpp:98-113,122; captured by tsdf_set_calibration) in the order 0-4 1-5 2-6 3-7 0-1 1-2 2-3 3-0 4-5 5-6
 *   6-7 7-4, colour (0, 1, 0, 1), width 1, aliased; then one point of size 3 at Frustum::getCameraPos() (the value of
 *   tsdf_frustum_from_volume), colour (1, 0, 0, 1).  Positions are world coordinates through P * (MV * p).  Timer "frustums".
 *   TSDF_ERR_STATE when a stream has no cv_xyz.
 * tsdf_calibvis_stats: out[0] = grid points of the last tsdf_draw_calibvis, out[1] = of them removed whole by its empty-space test (blocks
 *   whose trilinear taps lie in tiles that hold only the clear value -limit, when -limit <= -0.01: every such sample is discarded).
 * tsdf_draw_bbox: the bounding-box wireframe (g_draw_grid, on by default :70, .conf key draw_grid :299; :685-702) = gloost::BoundingBox::
 *   draw() (external/gloost/BoundingBox.cpp:298-318) -> gloost::drawWiredBox (gloostRenderGoodies.h:251-304): six GL_LINE_LOOPs of four
 *   corners of the box bbox_min..bbox_max as configured, in world coordinates through P * (MV * p): front (z = max), right (x = max), back
 *   (z = min), left (x = min), top (y = max), bottom (y = min), corners in drawWiredBox's order, each loop closed by its v3 -> v0 segment
 *   (24 segments; every box edge is drawn twice, once in each direction, and the first one drawn wins depth ties).  glLineWidth(2), aliased.
 *   Colour (1, 1, 1, 0.75) with GL_COLOR_MATERIAL on and lighting off, written unmodulated, no blending.  Timer "bbox".  Runs after any
 *   back-end (tsdf_draw_f, tsdf_draw_points, tsdf_draw_trigrid, tsdf_draw_mvt) and after the two overlays above (the client's order).
 * tsdf_draw_bricks: "Draw occupied bricks" (g_draw_bricks, :83,275,409-410, key :764-765) = ReconIntegration::drawOccupiedBricks()
 *   (recon_integration.cpp:447-454): the program linked from glsl/bricks.vs + glsl/solid.fs (:130-133), uniform Color = (1, 0, 0),
 *   UnitCube::drawWireInstanced (unit_cube.cpp:20-29,74-83) with one instance per entry of m_bricks_occupied.  Per instance 12 GL_LINES
 *   between the unit cube's vertices v0..v7 = (1,1,1) (0,1,1) (1,1,0) (0,1,0) (1,0,1) (0,0,1) (0,0,0) (1,0,0), start -> end in this order:
 *   v0-v1 v0-v2 v0-v4 v5-v1 v5-v4 v5-v6 v3-v1 v3-v6 v3-v2 v7-v2 v7-v4 v7-v6.  A vertex p of brick id lies at world
 *   float(index) * brick_size + bbox_min + p * brick_size per axis, in that operand order, index = index_3d(id) (bricks.vs:16-20,
 *   inc_bricks.glsl:22-38), and goes through P * (MV * (world, 1)).  Every brick is drawn at the full brick size, the clipped last brick of
 *   an axis too, so the wireframe can stick out of the bounding box.  Colour (1, 0, 0, 1) (solid.fs), width 1, aliased (the only
 *   glLineWidth of the client is the bounding box's, inside glPushAttrib / glPopAttrib, external/gloost/BoundingBox.cpp:301-316).  The
 *   instances are the bricks of the latest tsdf_update_occupied (:430-445: ascending brick id, threshold tsdf_set_min_voxels_per_brick),
 *   whatever tsdf_set_use_bricks / tsdf_set_space_skip say; while there is no list (a new context, a new brick grid after
 *   tsdf_set_voxel_size / tsdf_set_brick_size) nothing is drawn and the call returns TSDF_OK.  (As for every reader of the list: a
 *   tsdf_mark_bricks issued since the latest update, with no draw, integrate or ratio read-back in between, may already have reset the
 *   count for the coming update.)  Needs no volume: sparse-pool and Z-slab contexts draw the same lines (every rank marks the whole brick
 *   grid).  This is the client's call while another back-end is showing (kinect_client.cpp:681-683), after "Draw TSDF" and "Draw
 *   frustums" and before the bounding box.  Timer "brickwire" (the reference has none; "brickdraw" is the depth limits').
 *   TSDF_ERR_STATE for a brick grid with 12 * bricks >= 2^32 - 1.
 *   Assumed, not checkable without a GL implementation: that bricks.vs + solid.fs links although bricks.vs writes a non-flat uint output
 *   that solid.fs never reads.  The depth-limit program (bricks.vs + bricks.gs + bricks.fs) uses the same vertex shader, and this project
 *   treats it as working throughout.
 * tsdf_set_draw_bricks: ReconIntegration::setDrawBricks, off by default (recon_integration.cpp:57).  While it is on, tsdf_draw_f -- and
 *   through it tsdf_frame_dev / tsdf_frame_raw_dev -- ends with tsdf_draw_bricks under the draw's own matrices, after the hole filling and
 *   before timer "3recon" ends (:160-173).  With it on and a stereo state set (colour-mask mode != 0, viewport origin / offset != 0)
 *   tsdf_draw_f returns TSDF_ERR_STATE before it queues anything: the stereo form of this debug view is not provided.  The overlay
 *   joins the hole-filling lane and the lane ahead, so with stage overlap the lanes run one after the other for that frame: accepted
 *   for a debug view.  With the flag off every path is what it is without this entry.
 * tsdf_draw_textures: the texture view (g_draw_textures, key T :773, selector key Y :768; :704-707) = TextureBlitter::blit(15 + which,
 *   resolution_full / 2) (texture_blitter.cpp, glsl/texture_passthrough.{vs,fs} mode 0), drawn last.  which = 0: unit 15, the atlas the
 *   latest hole filling completed (the one fillColors() binds at recon_integration.cpp:315: the 1.5w x h RGBA32F ViewLod whose level 0 is
 *   that draw's raymarch, levels 1.. its pyramid and every other texel the clear value (0, 1, 0, 0) of ViewLod::enable -- GL's T atlas of
 *   the two-atlas sequence, which no transfer pass clears).  which = 1: unit 16, the w x h RGBA32F depth-limit image drawDepthLimits() left
 *   (:171; clear (1, 0, 1, 0) :144, then per pixel MIN-blended (z, -z, back-facing ? z : 1, 1) of bricks.fs).  A drawF() without colour
 *   filling or without space skipping leaves the respective texture as it was.  The blit covers the viewport (0, 0, vw, vh), (vw, vh) =
 *   uvec2(fvec2(uvec2(1.5f * w, h)) / 2) (960 x 360 at 1280 x 720) whatever the source's size; framebuffer row y is GL window row y, as
 *   tsdf_download_framebuffer returns it.  Output (rgb, 1); the depth test is off and depth is not written; pixels outside the viewport are
 *   untouched.  Timer "textures".  TSDF_ERR_INVALID_ARGUMENT for which > 1; TSDF_ERR_STATE when the chosen texture has not been produced
 *   since create / tsdf_resize (no draw with colour filling, no drawF with space skipping -- GL would show an undefined texture), after a
 *   march into the pyramid that no hole filling has completed yet, and for unit 16 after an integrate() that already reset the image for
 *   the coming draw.
 *   Assumed, not defined by GL state alone: the client's glEnable(GL_TEXTURE_2D) on unit 0 (kinect_client.cpp:982) would modulate the
 *   wireframe's colour by a complete 2-D texture bound on unit 0 under fixed-function texturing; this definition assumes none is, so the wire
 *   colour is the current colour.  After tsdf_draw_trigrid / tsdf_draw_mvt GL's units 15 / 16 hold those back-ends' pass textures
 *   (recon_trigrid.cpp:142-143); tsdf_draw_textures shows ReconIntegration's textures, which is what the client's texture view is for.
 *
 * What GL leaves open, defined here and restated by tests/overlay_reference.py (the kernels match it bit for bit; fp32 throughout, matrix
 * products as sum_k m[k][row] * v[k] left to right, no contraction):
 *   Points.  Whole-point clip: dropped unless clip.w > 0 and |x|, |y|, |z| <= clip.w; window x = (clip.x / clip.w * 0.5 + 0.5) * W (y alike),
 *     z = clip.z / clip.w * 0.5 + 0.5, dropped unless z < 1.  A point of size s covers the pixels px in [ceil((x - s/2) - 0.5),
 *     ceil((x + s/2) - 0.5) - 1] (rows alike) inside the view: s = 1 for the TSDF overlay (calib_vis.vs never writes gl_PointSize), 3 for the
 *     camera point.
 *   Lines (GL 4.4 section 14.5.1, diamond exit, width 1).  The segment is clipped in clip space against the near plane (z + w >= 0), then
 *     the far plane (w - z >= 0): an end point e outside moves towards the other one o, to e + (o - e) * t with t = d_e / (d_e - d_o)
 *     (d: the plane distances above); a line wholly outside either plane is dropped, as is one with an end point at w <= 0 after clipping.  With the window coordinates of start a and end b: if
 *     |b.x - a.x| >= |b.y - a.y| (x-major) every pixel column i whose centre c = i + 0.5 lies in [a.x, b.x) along the direction of travel
 *     (a.x <= c < b.x, or b.x < c <= a.x) makes one fragment in row r = floor(a.y + (b.y - a.y) * t), t = (c - a.x) / (b.x - a.x).  Its depth
 *     is GL's (eq. 14.5, 14.6): that of the fragment's centre p = (c, r + 0.5) projected onto the segment, a.z + (b.z - a.z) * tz with
 *     tz = ((p.x - a.x) * dx + (p.y - a.y) * dy) / (dx * dx + dy * dy), d = b - a, clamped to [0, 1] -- not the depth of the line where it
 *     crosses the column, which is off by up to half a pixel's depth step.  y-major lines the same with rows.  Fragments outside the view
 *     are dropped.
 *   Wide lines (GL 4.4 section 14.5.2.2, aliased; the bounding box's width 2).  After the near / far clip the width is rounded to w = 2 and
 *     the window segment moves by -(w - 1) / 2 = -0.5 in its minor direction (a.y and b.y of an x-major line, where |dx| >= |dy|; a.x and b.x
 *     of a y-major one; the major direction is that of the unmoved segment, which the shift does not change).  The moved segment is walked
 *     by the width-1 rule above, and each of its fragments becomes a column (x-major) or row (y-major) of w fragments whose lowest
 *     (leftmost) one is that fragment, all at its depth, each dropped on its own outside the view.
 *   Texture view.  Pixel (x, y) of the viewport takes the texture coordinate (u, v) = ((x + 0.5f) / vw, (y + 0.5f) / vh) (IEEE divisions;
 *     the full-screen triangle of screen_quad.cpp:11-15).  Sampling is fp32 bilinear on the source's own size (sw, sh), sampling.hpp's
 *     axis_linear: f = u * sw - 0.5, taps clamp(floor(f)) and clamp(floor(f) + 1) to [0, sw - 1] (CLAMP_TO_EDGE; for u in [0, 1] the
 *     atlas's MIRRORED_REPEAT picks the same taps), weight a = f - floor(f); rows alike.  Per channel lerp(lerp(t00, t10, ax), lerp(t01, t11,
 *     ax), ay) with lerp(p, q, t) = p + (q - p) * t, t10 the tap right of t00 and t01 the one above it.  Unit 16's green channel is
 *     min(0, -z) = 0 - max z, +0 where no brick fragment landed.
 *   Depth test.  A fragment passes only if z < the framebuffer's depth before the overlay (strict); among passing fragments of one pixel the
 *     smallest (z bits, primitive index) wins -- GL_LESS with primitives drawn in order.  Primitive index: the grid's linear index
 *     (x + res.x * (y + res.y * z)) for the TSDF overlay, stream * 13 + k for the frustums (k < 12 the lines in the order above, 12 the point),
 *     4 * loop + k for the bounding box (loop in the order above, k the segment from its corner k to corner (k + 1) % 4), 12 * brick id + k
 *     for the occupied bricks (k the segment in the order above; GL draws instance after instance and the reference's list ascends in brick
 *     id, so this is its draw order whatever the order of the device list). */
int32_t tsdf_draw_calibvis(tsdf_ctx* ctx, const float modelview[16], const float projection[16]);
int32_t tsdf_set_active_kinect(tsdf_ctx* ctx, uint32_t stream);
int32_t tsdf_draw_frustums(tsdf_ctx* ctx, const float modelview[16], const float projection[16]);
int32_t tsdf_calibvis_stats(tsdf_ctx* ctx, uint64_t out[2]);
int32_t tsdf_draw_bbox(tsdf_ctx* ctx, const float modelview[16], const float projection[16]);
int32_t tsdf_draw_bricks(tsdf_ctx* ctx, const float modelview[16], const float projection[16]);
int32_t tsdf_set_draw_bricks(tsdf_ctx* ctx, int32_t active);
int32_t tsdf_draw_textures(tsdf_ctx* ctx, uint32_t which);

/* ---- the GUI's "Show textures" windows (settings panel, source/kinect_client.cpp:336-338,483-515): each window is an ImGui::Image of ONE
 * LAYER of one of NetKinectArray's seven texture arrays -- the view people open first when a reconstruction looks wrong.
 * tsdf_draw_sensor_texture draws that image quad into the framebuffer as the previous draw left it (tsdf_upload_framebuffer puts a known one
 * underneath, tsdf_download_framebuffer reads the result).  Out of scope, the host GUI's business: ImGui's window chrome, its list boxes and
 * the one-pixel border rectangle around the image (imgui.cpp:5621-5625, anti-aliased through the font atlas).  `rect` is the image quad itself
 * (bb.Min + 1 .. bb.Max - 1 when the border colour is set, as at kinect_client.cpp:509).
 *   type   0 Color, 1 Depth, 2 Quality, 3 Normals, 4 Silhouette, 5 Orig Depth, 6 LAB colors (the list box of kinect_client.cpp:496)
 *   stream the sensor = the array layer (TexInfo::layer = -stream - 1, :499; the back-end passes -(layer + 1), imgui_impl_glfw_glb.cpp:116)
 *   rect   p_min.x, p_min.y, p_max.x, p_max.y in ImGui coordinates: origin at the top left of the w x h view, y down
 *   clip   ImDrawCmd::ClipRect (x, y, z, w), or NULL = the whole view
 * tsdf_sensor_view_size: the size the client gives the image, ImVec2(width, width / aspect) with aspect = float(res.y) / res.x of the DEPTH
 *   resolution (:502-509: the image is shown turned by a quarter turn, so a 640 x 480 sensor makes a 480-wide image 640 high).  Host only.
 *
 * Sources.  The arrays are picked through texture units getStartTextureUnit() + type (NetKinectArray.cpp:428-462, bound at :451-462); every
 * array is a globjects texture with its default LINEAR + CLAMP_TO_EDGE (TextureArray.cpp:27) unless NEAREST is set (NetKinectArray.cpp:
 * 147-188).  A texel becomes the sample's vec4 as GL expands its format:
 *   0  m_colorArray: RGB8 -> (rgb / 255, 1); the COMPRESSED_RGBA DXT1 / DXT5 formats -> rgba / 255 of the decoded RGBA8 this library holds
 *      (tsdf_download_raw_frame's colour).  LINEAR, COLOUR resolution.  Bytes are converted (c / 255, an IEEE division) before the filter, and
 *      all four channels are filtered, DXT alpha too.
 *   1  the texture unit "depth" holds after processTextures(), m_textures_depth_b (:364,377): RG32F -> (r, g, 0, 1), NEAREST.
 *   2  m_textures_quality: LUMINANCE32F -> (L, L, L, 1), LINEAR.
 *   3  m_textures_normal: RGB32F -> (rgb, 1), LINEAR.
 *   4  m_textures_silhouette: R32F -> (r, 0, 0, 1), LINEAR.
 *   5  unit "morph_depth", m_textures_depth2.front (:283): the eroded-then-dilated raw depth, whatever useProcessedDepths says;
 *      LUMINANCE32F -> (L, L, L, 1), NEAREST.
 *   6  unit "color_lab", m_textures_color: the Lab image of pre_depth.fs, RGB32F -> (rgb, 1), LINEAR.
 *   Types 1 - 6 have the depth resolution.  LINEAR is sampling.hpp's axis_linear on the source's own size (the "Texture view" paragraph
 *   above: f = u * n - 0.5, taps clamp(floor(f)) and clamp(floor(f) + 1), weight f - floor(f)), lerp along x, then along y, per channel.
 *   NEAREST is texel clamp(floor(u * n), 0, n - 1) per axis.
 * Coverage and Frag_UV (GL leaves rasterisation and interpolation latitude; defined here).  Framebuffer pixel (i, j) is GL window row j, as
 *   tsdf_download_framebuffer returns it; its centre in ImGui coordinates is cx = i + 0.5f, cy = float(h) - (j + 0.5f) -- the orthographic
 *   projection of imgui_impl_glfw_glb.cpp:79-85 undone.  The pixel is covered iff p_min.x <= cx < p_max.x and p_min.y <= cy < p_max.y, and
 *   it lies inside the view and inside the scissor box of :123: columns [sx, sx + sw), rows [sy, sy + sh) with sx = (int)clip.x,
 *   sy = (int)(float(h) - clip.w), sw = (int)(clip.z - clip.x), sh = (int)(clip.w - clip.y) (fp32 differences; (int) truncates, values beyond
 *   +-2^30 saturate there; a negative sw or sh -- which GL rejects -- covers nothing).  Frag_UV = ((cx - p_min.x) / (p_max.x - p_min.x),
 *   (cy - p_min.y) / (p_max.y - p_min.y)), IEEE divisions: uv0 = (0, 0) and uv1 = (1, 1) as at kinect_client.cpp:509.
 * The turn (fragment shader, imgui_impl_glfw_glb.cpp:275-281).  uv -= .5; uv = mat2(cos r, -sin r, sin r, cos r) * uv (column major), that is
 *   (c * u + s * v, (-s) * u + c * v), products first, then the sum, no contraction; uv += .5; r = radians(90.0).  c and s are the fp32 values
 *   cosf(1.5707964f) = -4.37113883e-08f (bits 0xb33bbd2e, NOT 0) and sinf(1.5707964f) = 1.  The sample is texture(array, (uv, stream)).
 *   Assumed, not checkable without a GL implementation: a GLSL compiler may fold these constants at another precision (c = 0 exactly would
 *   move uv by at most 2.2e-8, which can change a NEAREST pick or a LINEAR weight only at a texel border).
 * Blend and writes (:68-74).  Depth test off, depth not written.  Frag_Color is white (ImColor(255,255,255,255), :509), so Out_Color is the
 *   sample s.  GL_FUNC_ADD with (SRC_ALPHA, ONE_MINUS_SRC_ALPHA) on all four channels of the destination d, fp32: k = 1 - s.a, out =
 *   (s * s.a) + (d * k) per channel, alpha included.  A sample with s.a == 1 REPLACES the pixel exactly (every type but DXT colour): a NaN or
 *   inf a previous draw left underneath does not get through d * 0.  Values are not clamped: the client's RGBA8 window would clamp, this
 *   project's float framebuffer does not (the convention of tsdf_draw_textures).  Pixels outside the quad, the scissor box or the view are
 *   untouched.  Timer "sensortex".
 * State.  The windows show NetKinectArray's arrays as of the latest tsdf_process_textures: all seven types after it, on every raw ingest path
 *   (tsdf_upload_raw_frame, _dev, tsdf_upload_wire_frame with RGB8 / DXT1 / DXT5, tsdf_frame_raw_dev).  Type 6 produces the whole Lab image
 *   on request exactly as tsdf_download_preprocessed does, and returns TSDF_ERR_STATE under the same condition.  A raw frame uploaded but not
 *   yet processed: TSDF_ERR_STATE for every type, as before any frame.  For a frame handed over already processed (tsdf_upload_frame, _dev,
 *   _async + tsdf_select_frame_slot, tsdf_frame_dev) types 0, 1, 2 and 4 read the current frame slot; type 1 then shows (r, 0, 0, 1), because
 *   the slot keeps depth.r alone; type 3 shows the image of tsdf_upload_normals once that was called for this kind of frame, TSDF_ERR_STATE
 *   before; types 5 and 6 return TSDF_ERR_STATE.
 *   TSDF_ERR_INVALID_ARGUMENT: type > 6, stream >= num_streams, rect NULL, a non-finite rect or clip value, p_max <= p_min on either axis.
 *   TSDF_ERR_STATE: a viewport origin / offset != 0 (side-by-side stereo renders no GUI, kinect_client.cpp:529-531).  A colour-mask mode != 0
 *   is allowed and ignored: the reference restores the full mask at the end of every draw (recon_integration.cpp:235-236,332-333) and ImGui
 *   renders over the anaglyph picture.  Needs no volume: sparse-pool and Z-slab contexts draw the same.
 *   With stage overlap the draw joins the hole-filling lane and the lane ahead, and the next tsdf_process_textures waits for a window that read
 *   a product it rewrites: the lanes run one after the other for that frame, accepted for a debug view.  Without a call to this entry every
 *   path is what it is without it. */
int32_t tsdf_draw_sensor_texture(tsdf_ctx* ctx, uint32_t type, uint32_t stream, const float rect[4], const float clip[4]);
int32_t tsdf_sensor_view_size(const tsdf_ctx* ctx, float width, float size[2]);

/* ---- draw() host matrices.  Host only, no context, no GPU: the matrix block ReconIntegration::draw()
 * builds before the raymarch -- vol_to_world = translate(bbox_min) * scale(bbox extent) (recon_integration.cpp:66-72),
 * image_to_eye = inverse(scale(w/2, h/2, 1/2) * translate(1,1,1) * projection) (:182-193), NormalMatrix =
 * inverseTranspose(modelview * vol_to_world) (:199), CameraPos in volume space (:202-205) -- exactly the values the draw
 * calls hand to the kernels (formed in double, rounded to fp32 once).  out: 16 + 16 + 16 + 3 floats, column major.
 * Returns TSDF_ERR_INVALID_ARGUMENT for a singular modelview / projection. */
int32_t tsdf_view_matrices(const float modelview[16], const float projection[16], uint32_t view_w, uint32_t view_h,
                           const float bbox_min[3], const float bbox_max[3], float out[51]);

/* ---- inverse calibration volumes: the offline tool source/calib_inverter.cpp.
 * tsdf_frustum_from_volume: kinect::Frustum built from the 8 corner texels of a forward volume (getCornerPoints,
 *   calibration_inverter.cpp:117-133; planes + inside(): frustum.cpp) -> planes[6][4] (near far left right top bottom,
 *   inside = dot(plane, (p,1)) >= 0) and Frustum::getCameraPos(), the value CalibVolumes::getCameraPositions()
 *   (CalibVolumes.cpp:224-230) hands to the quality pass, i.e. the input of tsdf_set_camera_position.  Host only.
 * tsdf_inverse_volume_resolution: res = ceil(bbox extent / voxel_size), source/calib_inverter.cpp:60-63 (default 0.007 m).
 * tsdf_invert_calibration: CalibrationInverter::calculateInverseVolumes for one sensor (calibration_inverter.cpp:68-115):
 *   exact 8 nearest forward samples + inverse-distance weighting per output voxel, -1 outside the frustum, on GPU `device`.
 *   cv_xyz: [rz][ry][rx][3] host floats; cv_xyz_inv: [res_inv z][y][x][4] host floats (write with tsdf_calib_volume_write,
 *   depth limits 0.5 / 4.5 as :112).  gpu_ms (may be NULL): device time of build + query. */
int32_t tsdf_frustum_from_volume(const float* cv_xyz, const uint32_t res[3], float planes[24], float camera_pos[3]);
int32_t tsdf_inverse_volume_resolution(const float bbox_min[3], const float bbox_max[3], float voxel_size, uint32_t res[3]);
int32_t tsdf_invert_calibration(int32_t device, const float* cv_xyz, const uint32_t res_xyz[3], const float bbox_min[3], const float bbox_max[3],
                                const uint32_t res_inv[3], float* cv_xyz_inv, float* gpu_ms);

/* host-only reader of recordings/<sensor>.stream (sys::FileBuffer as used by NetKinectArray::readFromFiles,
 * framework/NetKinectArray.cpp:709-749; framework/io/FileBuffer.cpp:60-62,90-110): raw records [colour][depth] back to back.
 * One record of every sensor's file, concatenated in sensor order, is exactly one wire message for tsdf_upload_wire_frame. */
int32_t tsdf_stream_num_frames(const char* path, uint64_t record_bytes, uint64_t* frames);
int32_t tsdf_stream_read_record(const char* path, uint64_t record_bytes, uint64_t frame, void* out);

/* ---- frame ingest: NetKinectArray::init / readLoop / update,
 * framework/NetKinectArray.cpp:113-142 (sizes), :482-529 (message layout), :225-236 (upload).
 * A message is, per sensor, [colour: colorsize bytes][depth: depthsize bytes]; its first 8 bytes double as the frame's
 * timestamp (:510 -- they overlay the first colour bytes, offset starts at 0 at :513).
 * tsdf_upload_wire_frame copies the message through a pinned double buffer to HBM (asynchronous on the context's stream)
 * and unpacks it on the GPU into what tsdf_process_textures reads; it replaces tsdf_upload_raw_frame for wire input. */
#define TSDF_COLOR_RGB8 0u   /* CalibrationFiles::isCompressedRGB() == 0: w*h*3 bytes                      (:129) */
#define TSDF_COLOR_DXT1 1u   /*  == 1: S3TC DXT1 blocks, w*h/2 bytes                                     (:118-121) */
#define TSDF_COLOR_DXT5 5u   /*  == 5: S3TC DXT5 blocks, w*h bytes                                       (:123-126) */
#define TSDF_DEPTH_F32 0u    /* isCompressedDepth() false: float32 metres                                  (:138-141) */
#define TSDF_DEPTH_U8 1u     /* true: 8 bit, read normalised (c/255); metres = uncompress(), glsl/pre_depth.fs:51-61 */
int32_t tsdf_set_wire_format(tsdf_ctx* ctx, uint32_t color_format, uint32_t depth_format);
int32_t tsdf_wire_sizes(tsdf_ctx* ctx, uint64_t* colorsize, uint64_t* depthsize, uint64_t* message_bytes);
/* per sensor: KinectCalibrationFile::isCompressedDepth(), getNear(), getFar() (NetKinectArray.cpp:343-349) */
int32_t tsdf_set_depth_compression(tsdf_ctx* ctx, uint32_t stream, int32_t compressed, float near_m, float far_m);
int32_t tsdf_upload_wire_frame(tsdf_ctx* ctx, const void* message, uint64_t bytes, double* timestamp /* may be NULL */);
/* what the unpack produced: raw depth [N][H][W] float, colour [N][ch][cw][4] RGBA8 (either may be NULL) */
int32_t tsdf_download_raw_frame(tsdf_ctx* ctx, float* depth_raw, uint8_t* colour_rgba);

/* ---- image pre-processing: NetKinectArray::processTextures(), framework/NetKinectArray.cpp:309-426
 * Alternative to tsdf_upload_frame: hand over the RAW sensor frame (m_depthArray_raw R32F metres [N][H][W], colour RGB8,
 * NetKinectArray.cpp:147-176) and let tsdf_process_textures produce depth / quality / silhouette (and normals, Lab colour)
 * with the reference's passes: pre_morph.fs (3x3 dilate), pre_depth.fs (13x13 bilateral + RGB->Lab), pre_boundary.fs,
 * pre_normal.fs (which also calls mark_brick(): call it between tsdf_clear_bricks and tsdf_update_occupied, like
 * process_textures() in source/kinect_client.cpp:569-577, and do NOT call tsdf_mark_bricks as well), pre_quality.fs. */
int32_t tsdf_upload_raw_frame(tsdf_ctx* ctx, const float* depth_raw_m, const uint8_t* colour_rgb);
/* the same with both arrays already in DEVICE memory (a decoder's or a camera SDK's buffer): no copy, the passes read depth_raw_m where it lies.
 * flags as for tsdf_upload_frame_dev (0 / TSDF_FRAME_ARRAYS_COMPLETE); the arrays must stay untouched until work queued on the context's stream
 * after the next tsdf_integrate() / draw call runs.  Round 4: the raw upload, tsdf_upload_wire_frame and tsdf_process_textures run on the lane
 * ahead (as tsdf_upload_frame / tsdf_mark_bricks do), beside the integrate and the draw of the previous frames. */
int32_t tsdf_upload_raw_frame_dev(tsdf_ctx* ctx, const float* depth_raw_m, const uint8_t* colour_rgb, uint32_t flags);
int32_t tsdf_set_depth_limits(tsdf_ctx* ctx, uint32_t stream, float cv_min_d, float cv_max_d);   /* CalibVolumes::getDepthLimits, CalibVolumes.cpp:91-93 */
int32_t tsdf_set_camera_position(tsdf_ctx* ctx, uint32_t stream, const float xyz[3]);            /* CalibVolumes::getCameraPositions, :224-230 */
/* filterTextures / useProcessedDepths / refineBoundary, NetKinectArray.cpp:466-480 (all default true, :63-69) */
int32_t tsdf_set_preprocess(tsdf_ctx* ctx, int32_t filter_textures, int32_t processed_depth, int32_t refine_boundary);
int32_t tsdf_process_textures(tsdf_ctx* ctx);
/* products, any pointer may be NULL: depth2 [N][H][W], depth_rg [..][2], lab [..][3], depth_b [..][2], silhouette, normals [..][3], quality.
 * lab (the Lab colour image pre_depth.fs writes, read only by pre_boundary.fs) is evaluated by the passes only around the boundary pass's candidate
 * pixels; the whole image is produced by THIS call, from the inputs of the frame that was processed: TSDF_ERR_STATE when a newer raw frame has been
 * uploaded since tsdf_process_textures (ask before the next upload, or pass lab = NULL). */
int32_t tsdf_download_preprocessed(tsdf_ctx* ctx, float* depth2, float* depth_rg, float* lab, float* depth_b, float* silhouette, float* normals, float* quality);

/* ---- brick occupancy: clearOccupiedBricks / mark_brick / updateOccupiedBricks -------------------- */
int32_t tsdf_clear_bricks(tsdf_ctx* ctx);                       /* recon_integration.cpp:271-277 */
int32_t tsdf_mark_bricks(tsdf_ctx* ctx);                        /* pre_normal.fs:22-33 -> inc_bricks.glsl:40-58 */
/* recon_integration.cpp:430-445 without the GPU->CPU->GPU round trip; ratio may be NULL (no sync) */
int32_t tsdf_update_occupied(tsdf_ctx* ctx, float* ratio);

/* ---- the path ---------------------------------------------------------------------------------- */
int32_t tsdf_integrate(tsdf_ctx* ctx);                          /* integrate(), :242-269 */
/* drawF() up to and including draw(): drawDepthLimits() when space skipping and bricks are on (:154-156),
 * then the raymarch (:176-240) into the hole-filling pyramid level 0 or the framebuffer. */
int32_t tsdf_raymarch(tsdf_ctx* ctx, const float modelview[16], const float projection[16]);
int32_t tsdf_fill_colors(tsdf_ctx* ctx);                        /* fillColors(), :279-338 */
/* drawF(): tsdf_raymarch + (colour filling on ? tsdf_fill_colors : nothing), :151-174 */
int32_t tsdf_draw_f(tsdf_ctx* ctx, const float modelview[16], const float projection[16]);
/* One frame of the client's loop in one call (source/kinect_client.cpp:586-599 update + :616-669 draw): [tsdf_upload_frame_dev when depth_rg
 * is not NULL,] clearOccupiedBricks, markBricks (tsdf_upload_frame's brick marking), updateOccupiedBricks (no read-back), integrate, drawF.
 * Exactly the calls above in that order -- same results, same lanes --, for callers whose per-call overhead (an FFI, an interpreter)
 * is of the order of the frame itself.  Stops at the first failing step and returns its code. */
int32_t tsdf_frame_dev(tsdf_ctx* ctx, const float* depth_rg, const float* quality, const float* silhouette, const uint8_t* colour_rgb, uint32_t flags,
                       const float modelview[16], const float projection[16]);
/* ... and from the RAW frame, NetKinectArray::update() + processTextures() in front of the path (kinect_client.cpp:569-577): [tsdf_upload_raw_frame_dev
 * when depth_raw_m is not NULL,] clearOccupiedBricks, tsdf_process_textures (which marks the bricks), updateOccupiedBricks, integrate, drawF.
 * Same results as those calls.  With the lanes on and a new frame given, the first two pre-processing passes (morph, filter: they read the raw frame and write
 * only intermediate images) are queued in front of the lane's wait for the draws of two frames back and the rest behind it -- the order of the calls above
 * would put that wait first; this is what the single call buys beyond the call overhead (c2: 5 700 -> 6 400 frames/s from raw frames). */
int32_t tsdf_frame_raw_dev(tsdf_ctx* ctx, const float* depth_raw_m, const uint8_t* colour_rgb, uint32_t flags, const float modelview[16], const float projection[16]);

/* ---- setters mirroring recon_integration.hpp:43-49,57 and reconstruction.hpp:20-23 --------------- */
int32_t tsdf_set_tsdf_limit(tsdf_ctx* ctx, float limit);
/* setVoxelSize(), recon_integration.cpp:340-353: resolution = ceil(bbox / size); the volume is re-allocated (its content is gone
 * until the next integrate(), as in the reference) and the brick grid re-snapped from the current brick size.  Whole-volume contexts only. */
int32_t tsdf_set_voxel_size(tsdf_ctx* ctx, float size);
int32_t tsdf_set_use_bricks(tsdf_ctx* ctx, int32_t active);
int32_t tsdf_set_space_skip(tsdf_ctx* ctx, int32_t active);
int32_t tsdf_set_color_filling(tsdf_ctx* ctx, int32_t active);
int32_t tsdf_set_min_voxels_per_brick(tsdf_ctx* ctx, uint32_t n);
int32_t tsdf_set_brick_size(tsdf_ctx* ctx, const float size[3]);
int32_t tsdf_set_shade_mode(tsdf_ctx* ctx, int32_t mode);      /* UBO 1 g_shade_mode, shading.glsl:14-21 */
int32_t tsdf_resize(tsdf_ctx* ctx, uint32_t width, uint32_t height);
/* Side-by-side stereo (source/kinect_client.cpp:637-664): each eye is drawn into its own glViewport(x, y, w, h) and the operator
 * is told the same numbers with Reconstruction::setViewportOffset (reconstruction.hpp:23, recon_integration.cpp:527), which
 * tsdf_raymarch.fs subtracts from gl_FragCoord again (:70, :388-389).  tsdf_set_viewport_offset is that setter;
 * tsdf_set_viewport_origin is the glViewport origin the reference reads implicitly through gl_FragCoord (default 0, 0).
 * The context's framebuffer is the viewport's w x h pixels.  Equal origin and offset reproduce the mono frame bit for bit;
 * unequal ones shift the depth-peel lookup and the unprojection exactly as the shader's arithmetic does. */
int32_t tsdf_set_viewport_offset(tsdf_ctx* ctx, float x, float y);
int32_t tsdf_set_viewport_origin(tsdf_ctx* ctx, int32_t x, int32_t y);
/* Anaglyph stereo (kinect_client.cpp:616-633): Reconstruction::setColorMaskMode (reconstruction.hpp:22) -- 0 all channels, 1 red
 * only, 2 green + blue only: glColorMask around the raymarch (fill_holes off, recon_integration.cpp:212-216,235-237) or around
 * the colorfill pass (:321-333).  tsdf_set_framebuffer_clear(0): the client cleared only the depth buffer before this draw
 * (glClear(GL_DEPTH_BUFFER_BIT), :627), so masked channels and background pixels keep the previous draw's colour; 1 (default): the
 * colour buffer was cleared too (:609-610, :620). */
int32_t tsdf_set_color_mask_mode(tsdf_ctx* ctx, uint32_t mode);
int32_t tsdf_set_framebuffer_clear(tsdf_ctx* ctx, int32_t clear_color);

/* ---- getters ----------------------------------------------------------------------------------- */
int32_t tsdf_get_resolution(const tsdf_ctx* ctx, uint32_t res[3], uint32_t res_bricks[3], float brick_size[3]);
int32_t tsdf_num_bricks(const tsdf_ctx* ctx, uint32_t* n);
int32_t tsdf_occupied_ratio(tsdf_ctx* ctx, float* ratio);      /* occupiedRatio(), :478-480; synchronises */
int32_t tsdf_num_lods(const tsdf_ctx* ctx, uint32_t* n);       /* ViewLod::numLods, view_lod.cpp:25 */

/* ---- downloads / uploads of intermediate state (the reference never reads these back; tests do) -- */
int32_t tsdf_download_volume(tsdf_ctx* ctx, float* tsdf);                       /* [rz][ry][rx] */
int32_t tsdf_upload_volume(tsdf_ctx* ctx, const float* tsdf);
int32_t tsdf_download_bricks(tsdf_ctx* ctx, uint32_t* counters, uint8_t* occupied_flags);
int32_t tsdf_upload_brick_counters(tsdf_ctx* ctx, const uint32_t* counters);
/* the 8^3-voxel storage tiles the last culled integrate() computed -- the launch's work units (the reference draws the voxel
 * lists of the occupied bricks, recon_integration.cpp:254-258): x-fastest tile indices relative to tile layer grid[2];
 * grid = {tiles along x, tiles along y, first integrated tile layer, number of integrated tiles}.  ids may be NULL (count only) */
int32_t tsdf_download_active_tiles(tsdf_ctx* ctx, uint32_t* ids, uint32_t capacity, uint32_t* count, uint32_t grid[4]);
/* Which integrate kernel the last tsdf_integrate() launched (tests assert the path they are about; the choice follows the inverse LUTs' texel box per
 * 8^3 tile against the LDS budget, the RR_K1_FORM cap and the projection-cache budget).  out[0] = TSDF_K1_*, out[1] = workgroups of that launch
 * (TSDF_K1_CACHED: of the LDS kernel that takes the tiles the cache does not hold), out[2] = its work items (tiles: the active list of a culled launch,
 * every integrated tile of a dense one), out[3] = 1 culled / 0 dense.  out[1] < out[2]: the workgroups stride over the items.  Read-only; a culled
 * launch's item count is read from the device (synchronises like tsdf_download_active_tiles).  TSDF_ERR_STATE before the first integrate(). */
#define TSDF_K1_GENERIC 0u        /* k_integrate_tiles: every LUT tap from global memory (a tile's texel box exceeds the LDS budget) */
#define TSDF_K1_LDS_DIRECT 1u     /* k_integrate_tiles_lds, 8 taps per voxel out of the LDS box */
#define TSDF_K1_LDS_SEPARABLE 2u  /* k_integrate_tiles_lds, separable x / y passes */
#define TSDF_K1_RECORD 3u         /* k_integrate_tiles_rec: work records written by the pair-mask pass */
#define TSDF_K1_CACHED 4u         /* k_integrate_cached + the separable LDS kernel for uncached tiles (projection cache) */
int32_t tsdf_integrate_form(tsdf_ctx* ctx, uint32_t out[4]);
/* raymarch target level 0: rgba [h][w][4], depth [h][w], nsamples [h][w], depth peels [h][w][4]; any may be NULL */
int32_t tsdf_download_image(tsdf_ctx* ctx, float* rgba, float* depth, float* nsamples, float* peels);
int32_t tsdf_upload_image(tsdf_ctx* ctx, const float* rgba, const float* depth);
int32_t tsdf_download_framebuffer(tsdf_ctx* ctx, float* rgba, float* depth);    /* output of fillColors */
int32_t tsdf_upload_framebuffer(tsdf_ctx* ctx, const float* rgba, const float* depth);    /* its twin: a known framebuffer under an overlay (tests) */
int32_t tsdf_download_atlas(tsdf_ctx* ctx, float* rgba, float* depth);          /* [h][1.5w] pyramid atlas */

/* ---- mesh extraction: the fused surface as an indexed, coloured triangle mesh ---------------------------
 * The reference never exports what it fused (tsdf_download_volume is 4 bytes per voxel and leaves the iso-surfacing to the caller); these entries have
 * no counterpart in it.  They are built on what the raymarch restates: the hit test f > 0 (tsdf_raymarch.fs:96), get_gradient (:140-149),
 * blendColors (:295-330) and vol_to_world / NormalMatrix (recon_integration.cpp:66-72,199).  tests/mesh_reference.py restates the definition in numpy;
 * device and numpy agree bit for bit in counts, positions and indices.
 *
 * Marching tetrahedra on the voxel-centre lattice.
 * Samples.  Voxel (i, j, k) holds f at unit-cube position u = ((i + .5) / rx, (j + .5) / ry, (k + .5) / rz), each component in fp32 as
 *   ((float)i + 0.5f) / (float)rx.  A NaN or infinite value reads as -limit.  A lattice point is INSIDE iff f > 0 (zero and -0 are outside).
 * Cells.  Cell (i, j, k), 0 <= i < rx - 1 (likewise y, z), has corners c_b = (i + bx, j + by, k + bz), b = bx + 2 by + 4 bz.
 * Tetrahedra.  Kuhn's six along the diagonal c0 - c7, in this order: (0,1,3,7), (0,1,5,7), (0,2,3,7), (0,2,6,7), (0,4,5,7), (0,4,6,7).  The split is
 *   translation invariant and face compatible: the mesh is closed wherever the surface does not leave the volume.
 * Vertices.  Every tetrahedron edge runs from a lattice point p to p + d, d = 1..7 as a bit offset, and is owned by p.  It carries a vertex iff exactly
 *   one end is inside: with a = f(p), b = f(p + d), t = a / (a - b), per axis u = u_p + t * (u_q - u_p), world = bbox_min + u * (bbox_max - bbox_min);
 *   fp32, in this operation order.  A vertex exists once, however many triangles use it.
 * Triangles, per tetrahedron (v0, v1, v2, v3).  All or none inside: none.  One inside, or one outside (A): one triangle over the three edges at A, in
 *   vertex order.  Two inside (A before B), two outside (C before D): the quad AC, AD, BD, BC as (AC, AD, BD) and (AC, BD, BC).  The winding makes the
 *   geometric normal point from the inside corners to the outside ones (empty space, f <= 0) for positive bounding-box extents; it is a constant of
 *   (tetrahedron, case), never decided in floating point.  Degenerate triangles (t = 0) are kept.
 * Order.  Vertices by (8^3 storage tile of the owner, x fastest as in tsdf_download_active_tiles; owner inside the tile, x fastest, 0..511; d).
 *   Triangles by (tile of the cell, cell inside the tile, tetrahedron 0..5, triangle 0..1).  Indices are uint32.  No position depends on an atomic: two
 *   extracts of the same volume give identical arrays.
 * Normal (TSDF_MESH_NORMALS).  g = central differences of the trilinear TSDF at u +- limit / 2 per axis, gn = normalize(g) exactly as the raymarch shades a
 *   hit; the world normal is normalize(-gn / (bbox_max - bbox_min)): inverseTranspose(vol_to_world) of the shader's -gn.
 * Colour (TSDF_MESH_COLOURS).  blendColors of the CURRENT frame slot at u, four floats; alpha +1 = valid, -1 = fallback; independent of the shade mode;
 *   NaN stays NaN, as in the frame.
 *
 * tsdf_mesh_extract reads the volume tsdf_download_volume would return at that moment (it waits for an integrate() in flight on its lane), runs on the
 *   context's stream, synchronises and returns the counts (either pointer may be NULL).  The mesh stays in device memory of the context, sized exactly
 *   from the counts, until the next extract, tsdf_set_voxel_size or tsdf_destroy.  It writes no volume set, frame slot, pyramid or lane state.  A tile
 *   whose own class and whose seven +x/+y/+z neighbours' classes say "every voxel is -limit" (sparse pool: no slot) is skipped without reading a voxel.
 *   Timers "mesh_count", "mesh_scan", "mesh_emit".
 *   TSDF_ERR_STATE before the first tsdf_integrate / tsdf_upload_volume; for TSDF_MESH_COLOURS without calibration (cv_xyz_inv, cv_uv) and a frame; on a
 *   Z-slab context (a slab extracts its part of the mesh with tsdf_mesh_slab_extract, below: the parts concatenate to this mesh).  TSDF_ERR_INVALID_ARGUMENT for an unknown flag.
 *   TSDF_ERR_OUT_OF_MEMORY when the vertices do not fit uint32 or the allocation fails (no mesh is kept then).
 * tsdf_mesh_download copies the last extract's arrays: position [V][3], normal [V][3], colour [V][4], triangles [T][3]; any may be NULL.
 *   TSDF_ERR_STATE without an extract, and for an attribute the last extract did not produce.
 * tsdf_mesh_write_ply writes the last extract as a binary little-endian PLY: vertex x y z, then nx ny nz and red green blue alpha (float) where
 *   extracted, then faces as uchar 3 + three int indices.  TSDF_ERR_INVALID_ARGUMENT when the file cannot be written.
 * tsdf_mesh_stats: out = {tiles, tiles skipped by class, tiles with surface, bytes of mesh storage} of the last extract. */
#define TSDF_MESH_NORMALS 1u
#define TSDF_MESH_COLOURS 2u
int32_t tsdf_mesh_extract(tsdf_ctx* ctx, uint32_t flags, uint64_t* n_vertices, uint64_t* n_triangles);
int32_t tsdf_mesh_download(tsdf_ctx* ctx, float* position_xyz, float* normal_xyz, float* colour_rgba, uint32_t* triangles);
int32_t tsdf_mesh_write_ply(tsdf_ctx* ctx, const char* path);
int32_t tsdf_mesh_stats(tsdf_ctx* ctx, uint64_t out[4]);

/* ---- mesh level of detail: the same surface on the lattice of every 2nd / 4th voxel -----------------------
 * A level L has stride s = 1 << L: L = 0, 1, 2 give s = 1, 2, 4; any other level is TSDF_ERR_INVALID_ARGUMENT.  tests/mesh_lod_reference.py restates
 * this in numpy on top of tests/mesh_reference.py; device and numpy agree bit for bit in counts, positions and indices.
 * Lattice.  Level-L lattice point (i, j, k) IS voxel (s i, s j, s k): a point sample, not a filter.  The lattice has cr = ceil(r / s) points per axis.
 *   Voxels beyond the last lattice point belong to no cell: the mesh ends at the last lattice point.  A lattice thinner than 2 on an axis yields zero
 *   counts.
 * Topology.  Everything of the level-0 definition above, applied to the lattice: the reading of NaN / +-inf as -limit, inside iff f > 0, Kuhn's six
 *   tetrahedra, one vertex per crossed edge owned by its lower end p, the winding table, and the order by (8^3 LATTICE tile, x fastest; owner in the
 *   tile; d) and (tile of the cell, cell, tetrahedron, triangle).  The triangle array of level L is, byte for byte, the level-0 triangle array of the
 *   volume vol[::s, ::s, ::s].  "Tile" in the counts, in tsdf_mesh_stats, in max_surface_tiles and in needed_tiles means a lattice tile: 8^3 lattice
 *   points, (8 s)^3 voxels.
 * Vertex position: descent to a voxel edge.  A crossed lattice edge runs from voxel P = s p to P + s d, d its 0/1 offset vector.  For h = s/2, s/4, .., 1:
 *   read the voxel M = P + h d (an exact voxel read, sanitised like every sample); if (f(M) > 0) == (f(P) > 0), set P = M.  After L steps P and P + d
 *   are neighbouring voxels and exactly one of them is inside (the invariant holds at every step).  The vertex is the level-0 vertex of that voxel edge:
 *   a = f(P), b = f(P + d), t = a / (a - b), u = u_P + t * (u_Q - u_P) with the FULL resolution in ((float)x + 0.5f) / (float)rx, then vol_to_world;
 *   fp32 and the operation order of level 0.  So every level-L vertex is bit-identical to a vertex of the level-0 mesh, the position does not depend on
 *   how the truncation limit compares with the stride (the TSDF saturates at +-limit: interpolating along a 4-voxel edge would not give that), and no
 *   trilinear tap is involved.
 * Normal and colour.  Unchanged: the full-resolution gradient and blendColors at the vertex's u.
 * Class skip.  A lattice tile reads voxels in storage tiles [ct s, ct s + s] per axis, (s + 1)^3 of them, clipped to the grid.  When all of them say
 *   "every voxel is -limit" (sparse pool: no slot) the tile is skipped without a voxel read; that is exact.  A surface that lies wholly between lattice
 *   points is not part of a level-L mesh, skipped or not: a coarse level drops what its lattice does not sample, and a surface that leaves the lattice
 *   (between the last lattice point and the volume's face) leaves the mesh open there.
 * tsdf_mesh_extract_lod is tsdf_mesh_extract at a level; level 0 runs what tsdf_mesh_extract runs.  tsdf_mesh_download / _write_ply / _stats serve
 *   whichever extract was last; the stats count lattice tiles.  Error codes as tsdf_mesh_extract (Z-slab context, no volume yet, colours without
 *   calibration and a frame), and TSDF_ERR_INVALID_ARGUMENT for a level above 2. */
int32_t tsdf_mesh_extract_lod(tsdf_ctx* ctx, uint32_t flags, uint32_t level, uint64_t* n_vertices, uint64_t* n_triangles);

/* ---- mesh extraction on Z-slab contexts: parts that join byte for byte ------------------------------------
 * At the multi-GPU configurations no whole-volume context exists; these entries extract the mesh where the volume is.  The mesh above is ordered by
 * 8^3 lattice tile with the tile layer (z) outermost, nothing in it depends on an atomic, and slabs are tile aligned: the whole mesh IS the
 * concatenation of per-slab parts in slab order, and no vertex needs welding.  tests/mesh_slab_reference.py restates the split in numpy on top of
 * tests/mesh_reference.py and tests/mesh_lod_reference.py; the concatenated parts equal tsdf_mesh_extract_lod + tsdf_mesh_download of a whole-volume
 * context byte for byte.
 * Part.  A context that owns lattice tile layers [L0, L1) at level L (stride s = 1 << L, a lattice tile is 8 s voxels per axis: L0 = slab_z0 / (8 s),
 *   L1 = slab_z1 / (8 s), or the lattice's last layer + 1 when the slab reaches the volume's top) extracts
 *   vertices:  those whose owning lattice point lies in these layers, in the order of the whole mesh;
 *   triangles: those of the cells whose origin lies in these layers, in the order of the whole mesh;
 *   indices:   uint32, GLOBAL: into the concatenated vertex array.
 *   Positions (the descent at levels 1 and 2 included), normals and colours are exactly those of the definitions above; the class skip applies as it does
 *   there (a slab's halo layers count as "not clear", so a slab may read a tile the whole volume skips: the result is the same, the statistics are not).
 *   slab_z0 must be a multiple of 8 s, slab_z1 too unless it is the volume's top: TSDF_ERR_INVALID_ARGUMENT otherwise.  Level 0 always qualifies.  A
 *   whole-volume context is the one-slab case: the entries work on it and reproduce tsdf_mesh_extract_lod.
 * What a slab cannot know by itself is two sets of numbers: how many vertices the slabs below it hold (one uint64), and, for the triangles of its top cell
 *   layer, whose corners with lz = 8 are lattice points of the slab above, the per-tile vertex bases of that slab's first tile layer (ntx * nty uint32).
 *   Everything else about those lattice points -- edge mask, inside bit, offset inside their tile -- the slab computes itself: inside a tile, plane 0 comes
 *   first in the vertex order, so the offsets of its 64 lattice points depend on lattice planes 0 and 1 of that layer alone: voxel planes z1 and z1 + s,
 *   s <= 4, inside the halo.
 * Halo.  Precondition: the halo is current -- exchanged or recomputed -- exactly as for a raymarch on the slab.  It covers every voxel a part reads.  With
 *   x = limit / 2 * res_z (the gradient's offset in voxel planes) a context stores H = 8 * ceil((2 x + 2) / 8) >= 2 x + 2 >= 8 planes beyond either face.
 *   Lattice points and the descent's midpoints: an owned edge runs from voxel plane z to z + s <= z1, its midpoints lie between; the seam records read
 *   z1 and z1 + s <= z1 + 4.  Gradient taps: a vertex lies at voxel coordinate c in [z0, z1] (t = a / (a - b) is in [0, 1]); the tap at c + x has the
 *   trilinear footprint floor(c + x), floor(c + x) + 1 <= z1 + x + 1 <= z1 + H - 1, the tap at c - x the footprint floor(c - x) >= z0 - x - 1 >= z0 - H.
 *   So the clamp of Z taps into the stored planes never acts on a finite position, and normals equal the whole volume's bit for bit.  (A slab that stored
 *   no layer above a face below the volume's top would be refused with TSDF_ERR_STATE, never clamped silently; tsdf_create admits no such slab.)
 *
 * tsdf_mesh_slab_extract runs count, scan and the vertex emit over the owned layers, and the records of plane 0 of the first lattice tile layer above
 *   them (the seam layer: a records-only pass of its 64 plane-0 lanes per tile; seam tiles take record slots from the same scan and add nothing to the
 *   counts).  It synchronises and returns the part's counts (either pointer may be NULL).  The part is kept in a state of its own -- tsdf_mesh_download,
 *   _stats, _components, _texture_taps and the others do not see it and keep answering as before -- until the next tsdf_mesh_slab_extract,
 *   tsdf_set_voxel_size or tsdf_destroy.  The call drops the part of an earlier extract BEFORE it looks at its arguments: after a refused extract no part
 *   exists, and _seam, _link, _download and _stats answer TSDF_ERR_STATE (unlike tsdf_mesh_extract_lod, whose refused call leaves the old mesh: here the
 *   table's and the arrays' sizes depend on the level, and a caller must never fill buffers sized for another extract).
 *   Error codes as tsdf_mesh_extract_lod (without its refusal of slab contexts), plus the alignment rule above.
 *   Timers "mesh_slab_count", "mesh_slab_scan", "mesh_slab_emit".
 * tsdf_mesh_slab_seam: out[nty][ntx] (lattice tiles of the extract's level) = the slab-local vertex base of every lattice tile of the slab's FIRST owned
 *   layer: the exclusive scan value, defined for tiles without surface too.  This is what the slab below needs.
 * tsdf_mesh_slab_link writes the triangles.  The first vertex of an own tile is vertex_base + its local base; of a tile of the layer above,
 *   vertex_base + n_vertices + above_seam[tile]: the slab above must follow directly in the concatenation -- slabs are contiguous in z, in slab order, and
 *   above_seam is that slab's tsdf_mesh_slab_seam table of an extract at the same level.  above_seam may be NULL only when the slab reaches the volume's
 *   top (it is not read then): TSDF_ERR_INVALID_ARGUMENT otherwise.  TSDF_ERR_OUT_OF_MEMORY when vertex_base + n_vertices exceeds uint32, or, below the
 *   top, when above_seam[tile] plus that seam tile's plane-0 vertices does behind it (checked on the host before anything is written).  Linking again
 *   with another base is allowed and rewrites the triangles.  TSDF_ERR_STATE before an extract.  Timer "mesh_slab_link".
 * tsdf_mesh_slab_download: the shapes of tsdf_mesh_download; any pointer may be NULL.  TSDF_ERR_STATE before an extract, for an attribute the extract did
 *   not produce, and for the triangles before a link.
 * tsdf_mesh_slab_stats: out = {owned lattice tiles, of those skipped by class, of those with surface, bytes of the part's mesh storage}.
 * Out of scope.  Gaps between slabs.  Mesh streaming, components and texture taps on parts are not these entries' business: each has entries of its
 *   own further down (the part ring; "mesh components on Z-slab contexts", whose labels a new tsdf_mesh_slab_link releases).  The native RCCL
 *   exchange: the two numbers travel by whatever carries the caller's other collectives (rgbd-recon_amd/multigpu.py: SlabDriver.extract_mesh). */
int32_t tsdf_mesh_slab_extract(tsdf_ctx* ctx, uint32_t flags, uint32_t level, uint64_t* n_vertices, uint64_t* n_triangles);
int32_t tsdf_mesh_slab_seam(tsdf_ctx* ctx, uint32_t* out);
int32_t tsdf_mesh_slab_link(tsdf_ctx* ctx, uint64_t vertex_base, const uint32_t* above_seam);
int32_t tsdf_mesh_slab_download(tsdf_ctx* ctx, float* position_xyz, float* normal_xyz, float* colour_rgba, uint32_t* triangles);
int32_t tsdf_mesh_slab_stats(tsdf_ctx* ctx, uint64_t out[4]);

/* ---- mesh streaming: the fused surface every frame, packed, through a pinned ring -------------------------
 * tsdf_mesh_extract is a one-shot export: it allocates, waits for the host twice and leaves 12..40 bytes per vertex in fp32.  A telepresence client hands
 * its geometry to a remote renderer, a recorder or a thin client EVERY frame; these entries deliver the mesh the way tsdf_present delivers the picture:
 * queued behind the frame on the context's stream, compact, copied into a ring of pinned host buffers on the copy stream, picked up while the lanes
 * compute the next frames.  No counterpart in the reference.  tests/mesh_pack_reference.py restates the packing in numpy on top of
 * tests/mesh_reference.py; device and numpy agree byte for byte.
 *
 * What is meshed.  Exactly the mesh of tsdf_mesh_extract above: the same lattice, tetrahedra, one vertex per crossed edge, winding table, vertex and
 *   triangle order, uint32 indices, and the same reading of 0, -0, NaN and infinite voxels.  The triangle array of a streamed frame is byte-identical to
 *   the one tsdf_mesh_extract + tsdf_mesh_download give for the same volume.  The volume is the one tsdf_download_volume would return at the moment of the
 *   tsdf_mesh_stream call, the colours those of the frame slot current then; both are taken as stream dependencies (the context's stream waits for the
 *   integrate lane, and for the lane ahead when colours are asked for), never as a host wait.
 * Packed vertex.  One aligned vector store per vertex; vertex_stride = 8 bytes with flags == 0, 16 bytes with TSDF_MESH_NORMALS and / or
 *   TSDF_MESH_COLOURS (a field that was not asked for is 0).  Little endian.
 *   bytes 0-7   position: four uint16 qx, qy, qz, 0 with q = (uint16) rint(min(max(u, 0), 1) * 65535.0f), u the vertex's UNIT-CUBE coordinate of the
 *               definition above (u = u_p + t * (u_q - u_p), before vol_to_world); the product in fp32, rint = round to nearest, half-way cases to even.
 *               The receiver reconstructs world = bbox_min + (q / 65535) * (bbox_max - bbox_min): at most half a step, 0.5 / 65535 of the extent per axis,
 *               from the fp32 position.
 *   bytes 8-11  normal, octahedral, two int16 ox, oy.  n = the world normal of the definition above; s = (|nx| + |ny|) + |nz|, px = nx / s, py = ny / s;
 *               if nz < 0 (-0 is not): (px, py) = ((1 - |py|) * sg(px), (1 - |px|) * sg(py)), the old values on the right, sg(x) = x >= 0 ? 1 : -1;
 *               o = (int16) rint(min(max(p, -1), 1) * 32767.0f).  If any component of n is NaN (a zero gradient) both codes are -32768, which no finite
 *               normal produces.  Decoding: p = o / 32767, z = 1 - |px| - |py|, for z < 0 the same fold, normalize(px, py, z).
 *   bytes 12-15 colour r, g, b, a: blendColors as above, each channel by tsdf_present's RGBA8 rule (NaN -> 0, clamp, rint(v * 255)): the fallback alpha -1
 *               becomes 0, a valid alpha +1 becomes 255.
 * The ring.  tsdf_mesh_stream_config fixes the flags, the three capacities (vertices, triangles, 8^3 tiles with surface) and the number of slots (2..8);
 *   TSDF_ERR_INVALID_ARGUMENT for an unknown flag, a zero capacity, a slot count out of range, or a payload of more than 4 GiB.  A slot is a device buffer (a 64-byte header, then
 *   max_vertices * stride + max_triangles * 12 bytes), a pinned host buffer of the same size and four events.  The slots and ONE persistent set of
 *   scratch (per-tile counts and bases, the scan's sums, lattice-point records for max_surface_tiles tiles) are allocated by the first tsdf_mesh_stream
 *   after a config (or after tsdf_set_voxel_size); from the second call on tsdf_mesh_stream allocates nothing, frees nothing and never blocks the host:
 *   it waits for no GPU work.  (With the volume sets alternating and a hole-filling worker thread it does wait, as the overlays do, until that thread has
 *   ISSUED the stream wait of the job it was handed this frame -- a few host instructions of another thread, bounded, no device time.)
 * tsdf_mesh_stream(tag) takes the next free slot -- TSDF_ERR_STATE and nothing queued when every slot is queued or held -- and queues count, scan, a
 *   one-lane launch that writes the slot's header, and the two emit launches on the context's stream behind everything queued so far.  The emit kernels
 *   read the needs and the capacities from that header in device memory: when a need exceeds its capacity every workgroup returns at once and the
 *   header says so (overflow bits: 1 vertices, 2 triangles, 4 surface tiles; needed_* always filled; n_vertices = n_triangles = 0).  A frame is never
 *   partial.  The copy stream copies the header as soon as it is written; the payload -- exactly n_vertices * vertex_stride + n_triangles * 12 bytes in one
 *   copy, never the capacity -- is queued behind the emit by whichever of tsdf_mesh_stream, tsdf_mesh_stream_acquire and tsdf_mesh_stream_release is called
 *   first after the header has arrived on the host (each of them looks at every queued frame, oldest first); an acquire with wait != 0 waits for the
 *   header itself.  With a ring of 3 slots and the acquire two frames late no call ever waits.
 * tsdf_mesh_stream_acquire hands frames out in the order of the tsdf_mesh_stream calls.  *out is filled and *ready = 1 when the oldest frame is complete
 *   on the host; the pointers are into the slot's pinned buffer and stay valid until tsdf_mesh_stream_release (triangles follow the vertices directly).
 *   wait != 0 waits for that frame; wait == 0 sets *ready = 0 and returns TSDF_OK while it is not complete (never a partial frame).  ready may be NULL
 *   with wait != 0.  TSDF_ERR_STATE with nothing queued, or with a frame already held.  tsdf_mesh_stream_release frees the held slot (TSDF_ERR_STATE
 *   when none is held).
 * tsdf_mesh_stream_stats: out = {frames queued since the config, of those overflowed (as far as their headers have been seen), payload bytes copied to
 *   the host (headers not counted), device bytes held by slots and scratch}.
 * While frames are queued or held, tsdf_mesh_stream_config and tsdf_set_voxel_size return TSDF_ERR_STATE.  tsdf_destroy drains the ring.  TSDF_ERR_STATE
 *   on a Z-slab context, before the first tsdf_integrate / tsdf_upload_volume, and for TSDF_MESH_COLOURS without calibration and a frame -- as
 *   tsdf_mesh_extract; before any tsdf_mesh_stream_config too.  A lattice thinner than 2 on an axis yields frames with zero counts.  The mesh ring and the
 *   present ring share the copy stream and work side by side.  With the volume sets alternating (stage overlap), the integrate() two frames later that
 *   overwrites the set a frame's mesh kernels read waits for them.  Timers "mesh_stream_count", "mesh_stream_scan", "mesh_stream_emit".
 *   A context that never calls these runs exactly what it ran before they existed; tsdf_mesh_extract and its three companions are untouched. */
typedef struct tsdf_mesh_frame {
  const void*     vertices;      /* packed, n_vertices * vertex_stride bytes, in the slot's pinned buffer */
  const uint32_t* triangles;     /* [n_triangles][3] */
  uint64_t n_vertices, n_triangles;                           /* 0 when overflow != 0 */
  uint64_t needed_vertices, needed_triangles, needed_tiles;   /* what this frame's surface needs, always filled */
  uint64_t tag;
  uint32_t flags, vertex_stride, overflow;                    /* overflow bits: 1 vertices, 2 triangles, 4 surface tiles */
  uint32_t res[3]; float bbox_min[3], bbox_max[3];            /* what the receiver needs to dequantise */
} tsdf_mesh_frame;
#define TSDF_MESH_OVERFLOW_VERTICES  1u
#define TSDF_MESH_OVERFLOW_TRIANGLES 2u
#define TSDF_MESH_OVERFLOW_TILES     4u
int32_t tsdf_mesh_stream_config(tsdf_ctx* ctx, uint32_t flags, uint32_t max_vertices, uint32_t max_triangles, uint32_t max_surface_tiles, uint32_t slots);
int32_t tsdf_mesh_stream(tsdf_ctx* ctx, uint64_t tag);
int32_t tsdf_mesh_stream_acquire(tsdf_ctx* ctx, int32_t wait, tsdf_mesh_frame* out, int32_t* ready);
int32_t tsdf_mesh_stream_release(tsdf_ctx* ctx);
int32_t tsdf_mesh_stream_stats(tsdf_ctx* ctx, uint64_t out[4]);
/* The ring at a level of detail ("mesh level of detail" above): tsdf_mesh_stream_config_lod is tsdf_mesh_stream_config with a level (0, 1, 2;
 * TSDF_ERR_INVALID_ARGUMENT otherwise), tsdf_mesh_stream_config is it with level 0.  Every frame streamed after it is the level's mesh: the packing of what
 * tsdf_mesh_extract_lod gives for the same volume, triangles byte-identical.  max_surface_tiles and needed_tiles count lattice tiles of that level, and
 * the scratch is sized by its lattice-tile count.  tsdf_mesh_frame keeps its layout (res is the volume's resolution: positions are coded in the unit
 * cube at every level).  tsdf_mesh_stream / _acquire / _release / _stats are unchanged.  tsdf_mesh_stream_level reports the configured level
 * (TSDF_ERR_STATE before any config). */
int32_t tsdf_mesh_stream_config_lod(tsdf_ctx* ctx, uint32_t flags, uint32_t level, uint32_t max_vertices, uint32_t max_triangles, uint32_t max_surface_tiles, uint32_t slots);
int32_t tsdf_mesh_stream_level(tsdf_ctx* ctx, uint32_t* level);

/* ---- ray queries: cast caller-given rays into the fused volume --------------------------------------------
 * "What does this ray hit?" -- picking and measuring in a GUI, line-of-sight and range queries, views that are no pinhole.  The reference has
 * no counterpart (its GUI picks nothing); these entries are built on what the draw restates: intersectBox (tsdf_raymarch.fs:363-374), the march
 * (:62-114 with skipSpace off), get_gradient (:140-149), blendColors (:295-330) and vol_to_world (recon_integration.cpp:66-72).
 * tests/ray_reference.py restates the definition in numpy; device and numpy agree byte for byte in every field.  All arithmetic is fp32, every
 * operation rounded where it is written, sums and products left to right.
 *
 * The ray.  tsdf_ray, 32 bytes: origin o, t_min, direction d, t_max.  World coordinates by default; with TSDF_RAYS_UNIT_CUBE the volume's unit-cube
 *   coordinates, used as they come: o_u = o, d_u = d.  A world ray is mapped per axis a: e = bbox_max - bbox_min, o_u = (o - bbox_min) / e (the
 *   difference, then the division), d_u = d / e.  d need not be normalised.
 * Invalid rays.  len2 = d_u.x * d_u.x + d_u.y * d_u.y + d_u.z * d_u.z, len = sqrt(len2).  A ray is INVALID (status 4) when a component of o_u or d_u is
 *   not finite (so whenever one of o or d is not), when len is 0 or not finite (the zero direction, and directions whose squares underflow to zero or
 *   overflow), or when t_min is NaN.  It is never marched: n_samples = 0, t = -1, pos = 0.  A NaN t_max reads as +inf.
 * The march.  dn = d_u * (1.0f / len) (normalize3), sd = limit / 2, step = dn * sd.  intersectBox against the unit cube: inv = 1.0f / step,
 *   tbot = inv * (0.0f - o_u), ttop = inv * (1.0f - o_u), tmn = fmin(ttop, tbot), tmx = fmax(ttop, tbot) per axis (IEEE minNum / maxNum: a NaN operand
 *   -- 0 * inf of an axis-parallel ray -- is ignored), t0 = fmax(fmax(tmn.x, tmn.y), fmax(tmn.x, tmn.z)), t1 = fmin(fmin(tmx.x, tmx.y),
 *   fmin(tmx.x, tmx.z)).  !(t0 <= t1) or t1 < 0: the ray misses the box (status 2).  t_near = t0 < 0 ? 0 : t0: the entry point, or the origin when it is
 *   inside.  The caller's interval is in units of d; one step is sd / len of them: per = len / sd, s_min = t_min * per, s_max = t_max * per;
 *   if s_min > t_near, t_near = s_min; if s_max < t1, t1 = s_max; !(t_near <= t1): the interval misses the box (status 2).  With t_min = 0 and
 *   t_max = +inf neither assignment happens: the draw's arithmetic, bit for bit.  pos = o_u + step * t_near; max_n = ceil(|t1 - t_near|), at most
 *   4.0f / limit + 2.0f (converted to uint32 by truncation.  No ray of the unit cube is longer than sqrt(3) / sd < 4 / limit steps; the bound only cuts
 *   rays whose origin is so far off that t0 and t1 have lost the box to rounding).  prev = -limit.  Up to max_n times: dens = the trilinear TSDF at pos
 *   (LINEAR, CLAMP_TO_EDGE); the sample is counted; dens > 0 is a hit (a NaN density compares as no hit, as in the draw) at
 *   p = (pos - step) - step * (prev / (dens - prev)) and the march ends; otherwise prev = dens, pos = pos + step: chained additions.
 * Skipping.  Empty space is skipped by the exact per-tile classes integrate() leaves ("every voxel of this 8^3 tile is -limit"; sparse pool: the tile has
 *   no slot).  It never changes a bit of the above: skipped samples are accounted for by performing the same additions, and n_samples counts the
 *   definition's samples, skipped or fetched.
 * The answer.  tsdf_ray_hit, 32 bytes.  status: TSDF_RAY_HIT 1, TSDF_RAY_OUTSIDE 2 (the ray's interval misses the volume's box, no sample is taken),
 *   TSDF_RAY_INVALID 4; 0 = marched, nothing hit.  On a hit pos = p in unit-cube coordinates with TSDF_RAYS_UNIT_CUBE, else the mesh section's
 *   vol_to_world, bbox_min + p * e; t = ((p.x - o_u.x) * d_u.x + (p.y - o_u.y) * d_u.y + (p.z - o_u.z) * d_u.z) / len2, so that origin + t * dir is pos
 *   in the caller's units (up to rounding).  Without a hit t = -1 and pos = 0.  pad is 0.
 * The surface.  On request (TSDF_RAY_NORMALS, TSDF_RAY_COLOURS): tsdf_ray_surface, 32 bytes, per ray.  Exactly the mesh section's normal and colour
 *   evaluated at u = p: normal = normalize(-gn / e) with gn = normalize(central differences at u +- limit / 2); rgba = blendColors of the CURRENT frame
 *   slot at u, alpha +1 valid / -1 fallback, independent of the shade mode.  Zeros for a ray without a hit and for an attribute not asked for.
 *
 * tsdf_cast_rays: host arrays, synchronous.  Rays go in and results come out through device staging of the context that grows on demand (to a power of
 *   two of rays) and is then kept.  Timers "rays_march", "rays_surface".
 * tsdf_cast_rays_dev: device arrays.  Queued on the context's stream behind everything queued so far; never waits for the host.  The context's FIRST cast
 *   (either form) allocates the hit list (4 MiB) and its counters; no cast after it allocates anything.  The arrays must stay valid until a later tsdf_sync.
 * Both read the volume tsdf_download_volume would return at that moment (they wait, on the GPU, for an integrate() in flight on its lane) and for
 *   colours the frame slot current then; they write no volume set, frame slot, pyramid or lane state, and the integrate() that later overwrites the
 *   volume set they read waits for them.  n == 0: TSDF_OK, nothing is launched.  surface is NULL exactly when neither attribute flag is set.
 *   TSDF_ERR_INVALID_ARGUMENT: an unknown flag; with n > 0 a NULL ray or hit array, a surface array without an attribute flag or a flag without the
 *   array.  TSDF_ERR_STATE: before the first tsdf_integrate / tsdf_upload_volume; TSDF_RAY_COLOURS without calibration (cv_xyz_inv, cv_uv) and a frame;
 *   on a Z-slab context (a ray crosses slabs: cast on a whole-volume context).  -1 for a NULL context.
 * tsdf_view_rays: the draw's own rays for the pixel rectangle (x0, y0, w, h) of the current view size, row-major, bottom row first: unit-cube rays,
 *   origin = the camera in the unit cube, direction = the UN-normalised direction of the pixel centre (x + .5, y + .5) from the device function the
 *   draw's march calls, t_min = 0, t_max = +inf.  Cast with TSDF_RAYS_UNIT_CUBE they reproduce tsdf_raymarch with space skipping off: sample counts,
 *   hit set and positions.  Picking a pixel is tsdf_view_rays for one pixel, then tsdf_cast_rays.  Synchronous; needs no volume.
 *   TSDF_ERR_INVALID_ARGUMENT for a NULL argument, a singular matrix, an empty rectangle or one outside the view.
 * tsdf_ray_stats: out = {rays, of them hits, samples accounted for, samples whose voxels were fetched} of the last cast (waits for it).
 *   TSDF_ERR_STATE before any cast. */
#define TSDF_RAYS_UNIT_CUBE 1u
#define TSDF_RAY_NORMALS    2u
#define TSDF_RAY_COLOURS    4u
#define TSDF_RAY_HIT     1u
#define TSDF_RAY_OUTSIDE 2u
#define TSDF_RAY_INVALID 4u
typedef struct tsdf_ray { float origin[3]; float t_min; float dir[3]; float t_max; } tsdf_ray;
typedef struct tsdf_ray_hit { float pos[3]; float t; uint32_t n_samples; uint32_t status; uint32_t pad[2]; } tsdf_ray_hit;
typedef struct tsdf_ray_surface { float normal[3]; float pad; float rgba[4]; } tsdf_ray_surface;
int32_t tsdf_cast_rays(tsdf_ctx* ctx, const tsdf_ray* rays, uint64_t n, uint32_t flags, tsdf_ray_hit* hits, tsdf_ray_surface* surface);
int32_t tsdf_cast_rays_dev(tsdf_ctx* ctx, const tsdf_ray* rays_dev, uint64_t n, uint32_t flags, tsdf_ray_hit* hits_dev, tsdf_ray_surface* surface_dev);
int32_t tsdf_view_rays(tsdf_ctx* ctx, const float mv[16], const float proj[16], int32_t x0, int32_t y0, int32_t w, int32_t h, tsdf_ray* rays);
int32_t tsdf_ray_stats(tsdf_ctx* ctx, uint64_t out[4]);

/* ---- ray queries: slab parts -------------------------------------------------------------------------------
 * Where the volume exists only as Z-slabs (tsdf_config::slab_z0 / slab_z1) no context can answer a ray alone: a ray crosses slabs.  Every slab casts
 * the SAME rays and answers for the samples it owns (tsdf_cast_rays_part); the parts merge per ray (tsdf_merge_ray_parts_dev, or the rule below on the
 * host), and the merged arrays are byte for byte what tsdf_cast_rays gives on a whole-volume context.  It is the draw's slab march (owned samples,
 * the smallest sample count wins) for caller-given rays.  tests/ray_part_reference.py restates this section in numpy.
 *
 * Ownership of a sample.  The ray, its mapping, validity, intersectBox, the caller's interval, pos, max_n, step and the chained additions are the ray
 *   section's, unchanged.  Sample k (0-based) is at pos_k.  Its owner plane is fminf(fmaxf(floorf(pos_k.z * (float)rz), 0.0f), (float)(rz - 1)) with
 *   rz the volume's z resolution -- the draw's rule; a NaN z gives plane 0, +-inf clamp.  A context owns the sample iff plane >> 3 lies in its owned tile
 *   layers [own_tz0, own_tz1) = [slab_z0 / 8, (slab_z1 + 7) / 8).  Contiguous slabs that cover the volume own every sample exactly once.
 * A part.  The context examines its owned samples only.  Its hit is its first owned sample with dens > 0.  prev is the density of sample k - 1: for
 *   k = 0 it is -limit; if sample k - 1 is owned it is that sample's own value (it was no hit); otherwise it is fetched at pos_{k-1} from the halo.  The
 *   refinement, t, pos (unit cube or vol_to_world) and the surface (the normal and blendColors at the refined point) are the ray section's arithmetic.
 *   A record that can win the merge has prev <= 0 < dens, so its refined point lies within one step behind the owned sample and the halo covers its
 *   surface taps.  Where sample k - 1 was itself a hit (a neighbour's: such a part record never wins) the refined point can lie anywhere on the ray; its
 *   surface taps are clamped into the context's stored planes, as every z tap of a slab context is.
 *   The part record is a tsdf_ray_hit: on a hit status = TSDF_RAY_HIT and n_samples = k + 1; without one status = 0, n_samples = max_n, t = -1,
 *   pos = 0.  TSDF_RAY_OUTSIDE and TSDF_RAY_INVALID are as in the whole cast, and identical on every slab.  Surface records are zero without a hit.
 * Merge rule.  Parts k = 0 .. K - 1 of contiguous slabs in slab order: per ray the answer is the part record with TSDF_RAY_HIT and the smallest
 *   n_samples; no two parts can tie, a sample has one owner.  If no part hit, the answer is part 0's record.  The surface record travels with the winner.
 *   Why this is the whole cast: the whole march stops at the smallest k with dens_k > 0; each slab finds the smallest such k among its own samples, so
 *   the minimum over the slabs is that k, and its record is built from the same pos_k, dens_k and dens_{k-1} by the same arithmetic.  z is monotonic
 *   along a chain of additions of one step (x + s >= x for s >= 0 in fp32, and the owner plane is monotonic in z), so a slab's samples are one contiguous
 *   run and the kernel may stop behind it.  The merged arrays are byte for byte what tsdf_cast_rays gives on a whole-volume context, provided the halo
 *   is current exactly as for a draw on the slab: exchanged (tsdf_halo_pack_dev / _unpack_dev) or recomputed (slab_recompute_halo).
 * The one-slab case.  A whole-volume context is the one-slab case: it owns every sample, and its part cast equals its tsdf_cast_rays byte for byte.
 *
 * tsdf_cast_rays_part / tsdf_cast_rays_part_dev: the flags, argument checks, error codes, staging, chunking, stream ordering (they wait, on the GPU,
 *   for an integrate() in flight; the integrate() that later overwrites the set they read waits for them) and n == 0 are tsdf_cast_rays' and
 *   tsdf_cast_rays_dev's.  Timers "rays_part_march", "rays_part_surface".  They work on any context: slab or whole, dense or sparse pool.
 *   TSDF_ERR_STATE: before the first tsdf_integrate / tsdf_upload_volume; TSDF_RAY_COLOURS without calibration and a frame.  The _dev form never waits
 *   for the host and allocates nothing after the context's first cast.  Empty space is skipped by the tile classes as in the whole cast, for runs
 *   whose first and last sample are both owned.  After a part cast tsdf_ray_stats gives {rays, hits found in THIS part, owned samples accounted for
 *   (fetched or skipped), samples fetched}.
 * tsdf_merge_ray_parts_dev: device arrays, queued on the context's stream; runs on any context and needs no volume.  Part k's records start at
 *   hit_parts_dev + k * stride_records, the surface parts are laid out the same way.  TSDF_ERR_INVALID_ARGUMENT: parts == 0; with n > 0 a NULL array,
 *   exactly one of the two surface arrays, stride_records < n.  n == 0: TSDF_OK, nothing is launched.  -1 for a NULL context. */
int32_t tsdf_cast_rays_part(tsdf_ctx* ctx, const tsdf_ray* rays, uint64_t n, uint32_t flags, tsdf_ray_hit* hits, tsdf_ray_surface* surface);
int32_t tsdf_cast_rays_part_dev(tsdf_ctx* ctx, const tsdf_ray* rays_dev, uint64_t n, uint32_t flags, tsdf_ray_hit* hits_dev, tsdf_ray_surface* surface_dev);
int32_t tsdf_merge_ray_parts_dev(tsdf_ctx* ctx, const tsdf_ray_hit* hit_parts_dev, const tsdf_ray_surface* surface_parts_dev /* or NULL */, uint32_t parts, uint64_t n,
                                 uint64_t stride_records, tsdf_ray_hit* hits_dev, tsdf_ray_surface* surface_dev /* or NULL */);

/* ---- texture taps: per-stream colour coordinates and blend weights at caller-given points -----------------
 * A mesh carries one blendColors colour per vertex: voxel resolution, where the colour cameras deliver far more.  A receiver that already has the
 * colour images (the wire's DXT frames, a recording) needs, per vertex and stream, only WHERE that stream's colour image is read and the two numbers
 * blendColors weights the read with; with those it reproduces blendColors per fragment by plain projective texturing.  These are the values
 * blendColors (tsdf_raymarch.fs:295-330) forms per stream before it accumulates; vol_to_world is recon_integration.cpp:66-72.  The reference has
 * no counterpart: its client runs blendColors per pixel against the full colour images and the LUT volumes.  tests/texture_tap_reference.py restates the
 * definition in numpy on the oracle's filters; device and numpy agree byte for byte.  All arithmetic is fp32, every operation rounded where it is written.
 *
 * The point.  float xyz[3], 12 bytes.  World coordinates by default: u = (p - bbox_min) / e per axis (the difference, then the division), e = bbox_max -
 *   bbox_min: the ray section's mapping.  With TSDF_TAPS_UNIT_CUBE the volume's unit-cube coordinates, used as they come: u = p.
 * Not evaluated.  A point whose u has a component that is not finite, or with |component| >= 1.0e6f, is not evaluated: every one of its taps is
 *   {0, 0, 0, -1} and its sensor records are zero.  An evaluated dist is an absolute value and never negative, so dist == -1 marks the case.  Every other
 *   point is evaluated, also far outside the cube: the filters clamp to the edge.
 * Per stream i, in stream order, exactly the values blend_colors() forms: pc = texture(cv_xyz_inv[i], u).xyz; pcol = texture(cv_uv[i], pc).xy (both
 *   LINEAR, CLAMP_TO_EDGE); depth = the NEAREST depth of the current frame slot at pc.xy; dist = |depth - pc.z|; quality = dist < limit ? the LINEAR
 *   quality at pc.xy : 0.  A NaN stays a NaN (a NaN dist compares false: quality 0).
 * tsdf_texture_tap, 16 bytes: {u, v, quality, dist} with (u, v) = pcol, unclamped: the coordinates the colour fetch receives, LINEAR, CLAMP_TO_EDGE.
 * The receiver's rule.  With col_i the colour image of stream i read at (u, v) (RGB8 / 255, LINEAR, CLAMP_TO_EDGE):
 *   tw = sum_i quality_i / (dist_i + 0.01f); if tw > 0 the colour is (sum_i col_i * quality_i / (dist_i + 0.01f)) / tw -- per channel, the product,
 *   then the division --, otherwise it is (sum_i col_i / dist_i) / (sum_i 1.0f / dist_i).  The sums run left to right, in stream order, from 0.  This is
 *   blendColors: fed the taps of a unit-cube point it gives the bits of tsdf_ray_surface.rgba / the mesh colour at that point (alpha +1 / -1 = which branch).
 * tsdf_sensor_tap, 16 bytes, with TSDF_TAPS_SENSOR: {x, y, z, depth} = pc and the nearest depth: which sensor pixel looks at the point (x, y), the depth
 *   the point has there (z), the depth the sensor measured (depth).
 * Layout.  [n][N], point-major, N = num_streams: all taps of a point are contiguous, 16 * N bytes.
 *
 * tsdf_texture_taps: host arrays, synchronous, through device staging of the context that grows on demand (to a power of two of points) and is then kept.
 * tsdf_texture_taps_dev: device arrays.  Queued on the context's stream behind everything queued so far; never waits for the host and allocates nothing.
 *   The arrays must stay valid until a later tsdf_sync.
 * Both read calibration and the frame slot current at the call (they wait, on the GPU, for the frame's preparation as a coloured ray cast does) and write
 *   no volume set, frame slot, pyramid or lane state; the upload that later overwrites that slot waits for them.  They need no volume: they work
 *   before the first tsdf_integrate and on a Z-slab context (which holds whole LUTs and frames).  Calls of more than 2^18 points run as several
 *   launches.  Timer "texture_taps".
 * tsdf_mesh_texture_taps: the device form over the position array of the last tsdf_mesh_extract / tsdf_mesh_extract_lod (any level) without a round trip
 *   through the host.  Those are world coordinates -- the STORED fp32 positions: mapping them back does not give the emit kernel's u for every vertex (one
 *   ulp apart for a few per cent), so no bit equality with the mesh's own vertex colours is claimed --, and TSDF_TAPS_UNIT_CUBE is TSDF_ERR_INVALID_ARGUMENT.
 *   It uses the frame slot current at THIS call, not at the extract.  Results go into device arrays of the context sized exactly, kept until the next
 *   extract, the next call of this entry, tsdf_set_voxel_size or tsdf_destroy.  It synchronises and returns the counts (either pointer may be NULL).
 * tsdf_mesh_download_texture_taps: copies those results, [n_vertices][n_streams].  Either pointer may be NULL.  TSDF_ERR_STATE without taps for the
 *   current extract, and for `sensor` when TSDF_TAPS_SENSOR was not asked for.
 * tsdf_texture_tap_stats: out = {points, streams, (point, stream) pairs with quality > 0, pairs not evaluated} of the last call of any of the three forms
 *   (waits for it).  TSDF_ERR_STATE before any call.
 * Errors.  n == 0: TSDF_OK, nothing is launched.  TSDF_ERR_INVALID_ARGUMENT: an unknown flag (also with n == 0); with n > 0 a NULL point or tap array,
 *   `sensor` given without TSDF_TAPS_SENSOR or the flag without the array; more than 2^40 points.  TSDF_ERR_STATE: without calibration (cv_xyz_inv, cv_uv)
 *   of every stream or without a frame; the mesh form without an extract.  -1 for a NULL context. */
#define TSDF_TAPS_UNIT_CUBE 1u
#define TSDF_TAPS_SENSOR    2u
typedef struct tsdf_texture_tap { float u, v, quality, dist; } tsdf_texture_tap;
typedef struct tsdf_sensor_tap { float x, y, z, depth; } tsdf_sensor_tap;
int32_t tsdf_texture_taps(tsdf_ctx* ctx, const float* xyz, uint64_t n, uint32_t flags, tsdf_texture_tap* taps, tsdf_sensor_tap* sensor);
int32_t tsdf_texture_taps_dev(tsdf_ctx* ctx, const float* xyz_dev, uint64_t n, uint32_t flags, tsdf_texture_tap* taps_dev, tsdf_sensor_tap* sensor_dev);
int32_t tsdf_mesh_texture_taps(tsdf_ctx* ctx, uint32_t flags, uint64_t* n_vertices, uint32_t* n_streams);
int32_t tsdf_mesh_download_texture_taps(tsdf_ctx* ctx, tsdf_texture_tap* taps, tsdf_sensor_tap* sensor);
int32_t tsdf_texture_tap_stats(tsdf_ctx* ctx, uint64_t out[4]);

/* ---- mesh components: label the mesh's islands, drop the small ones ---------------------------------------
 * A TSDF fused from noisy depth does not fall as one surface: beside the subject and the floor there is a cloud of small closed blobs where a few voxels
 * crossed zero.  These entries label the connected components of the mesh the last tsdf_mesh_extract / tsdf_mesh_extract_lod left in the context (any
 * level; dense or sparse pool: only the mesh arrays are read) and rebuild the mesh without a set of them, on the device.  No counterpart in the
 * reference.  tests/mesh_component_reference.py restates the definition in numpy; device and numpy agree byte for byte.
 *
 * Connectivity is by index, never by position.  Vertices i and j are adjacent iff some triangle contains both; a component is a class of the transitive
 *   closure.  Coincident vertices with different indices (the mesh keeps degenerate triangles, so there are some) are connected only if triangles
 *   connect them.
 * Representative and numbering.  A component's representative is its smallest vertex index; components are numbered 0 .. C - 1 by increasing
 *   representative, so component 0 contains vertex 0.
 * Unused vertices.  A vertex used by no triangle is a component of its own with n_triangles = 0 (no extract produces one; the definition covers it).
 * Triangles.  A triangle's component is that of its vertices: all three agree.
 * Table.  tsdf_mesh_component, 16 bytes per component: first_vertex (the representative), n_vertices, n_triangles, reserved (0).
 * Keeping a set.  keep[c] != 0: component c stays.  Kept vertices stay in their order, the new index of a vertex is the number of kept vertices before
 *   it; position rows -- and normal and colour rows where extracted -- move bit for bit (NaN payloads included); kept triangles stay in their order,
 *   their three indices remapped, the winding untouched.  The result is a mesh in the definition's order; zero kept components give the empty mesh.
 * Defined despite atomics.  The device labels with a union-find whose links only ever point to a smaller index; whichever lane arrives first, the
 *   roots at the end are the smallest indices, the numbering is a scan and the counts are integer sums: two runs give identical bytes.
 *
 * tsdf_mesh_components labels the current mesh on the context's stream, synchronises and returns C (the pointer may be NULL).  The labels and the table
 *   stay in device memory beside the mesh until the next extract, tsdf_set_voxel_size, a keep / filter or tsdf_destroy; the mesh arrays are untouched.
 *   It may be called again, also after a keep / filter: the components are then those of the filtered mesh.  Timer "mesh_components".
 * tsdf_mesh_download_components copies vertex_component [V], triangle_component [T] and the table [C]; any may be NULL.
 * tsdf_mesh_keep_components (keep: C bytes of host memory) and tsdf_mesh_filter_components (keep[c] = table[c].n_triangles >= min_triangles, decided on
 *   the device) replace the context's mesh with the filtered one, its arrays sized exactly, and return its counts (either pointer may be NULL).
 *   tsdf_mesh_download / _write_ply / _stats serve the filtered mesh afterwards: stats[3], the storage bytes, is updated, the three tile counts stay
 *   those of the extract.  The labels are released (tsdf_mesh_components labels the new mesh), and so are the mesh's texture taps:
 *   tsdf_mesh_download_texture_taps answers TSDF_ERR_STATE until tsdf_mesh_texture_taps runs again.  The new arrays are allocated before anything is
 *   replaced: TSDF_ERR_OUT_OF_MEMORY leaves mesh and labels exactly as they were.  When every component is kept the arrays stay in place.
 *   Timer "mesh_filter".
 * tsdf_mesh_component_stats: out = {components, triangles of the largest component -- both of the last tsdf_mesh_components of the current mesh, 0
 *   before it and after a keep / filter --, vertices removed, triangles removed by the last keep / filter of this extract (0 before one)}.
 * Errors.  TSDF_ERR_STATE without an extract (a Z-slab context extracts no mesh, so always there); for download, keep and filter without components of
 *   the current mesh.  TSDF_ERR_INVALID_ARGUMENT for a NULL keep or a NULL out.  -1 for a NULL context.
 * The streamed ring (tsdf_mesh_stream) filters by the same rule inside the frame: "mesh streaming: the filtered frame" below.
 * Out of scope.  Z-slab contexts keep answering TSDF_ERR_STATE here: tsdf_mesh_slab_extract's parts are labelled where they are by "mesh components
 *   on Z-slab contexts" below, and the joined labels are these.  Welding by position.  Geometric measures per component (area, volume, bounding box) are not
 *   these entries' business: "mesh component measures" further down computes them beside the labels and filters by them.
 *   A context that never calls these entries runs exactly what it ran before they existed. */
typedef struct tsdf_mesh_component { uint32_t first_vertex, n_vertices, n_triangles, reserved /* 0 */; } tsdf_mesh_component;
int32_t tsdf_mesh_components(tsdf_ctx* ctx, uint64_t* n_components);
int32_t tsdf_mesh_download_components(tsdf_ctx* ctx, uint32_t* vertex_component, uint32_t* triangle_component, tsdf_mesh_component* table);
int32_t tsdf_mesh_keep_components(tsdf_ctx* ctx, const uint8_t* keep, uint64_t* n_vertices, uint64_t* n_triangles);
int32_t tsdf_mesh_filter_components(tsdf_ctx* ctx, uint32_t min_triangles, uint64_t* n_vertices, uint64_t* n_triangles);
int32_t tsdf_mesh_component_stats(tsdf_ctx* ctx, uint64_t out[4]);

/* ---- mesh components on Z-slab contexts: part labels that join byte for byte -------------------------------
 * At the multi-GPU configurations the concatenated mesh exists only in host memory; these entries label it where its parts are.  No counterpart in the
 * reference.  tests/mesh_slab_component_reference.py restates the split, the lists, the merge and the link in numpy.
 *
 * Definition.  Take the whole volume's mesh at a level -- the concatenation of the linked parts of "mesh extraction on Z-slab contexts" -- and its
 *   components, their numbering and their 16-byte table as "mesh components" defines them.  A part's results are
 *   vertex_component [the part's n_vertices]:    GLOBAL component numbers;
 *   triangle_component [the part's n_triangles]: GLOBAL numbers;
 *   table: the rows of the components whose representative (smallest vertex index) the part owns, in order; n_vertices and n_triangles are the WHOLE
 *          component's counts, whatever slabs it spans.
 *   Concatenated in slab order the three arrays are byte for byte what tsdf_mesh_components + tsdf_mesh_download_components give on a whole-volume
 *   context after tsdf_mesh_extract_lod at that level.  A whole-volume context is the one-slab case.
 * Two facts.  Every triangle of a part has an own vertex: corner 0 of its cell is in every Kuhn tetrahedron, so every emitted triangle has a vertex on an
 *   edge at corner 0, which the cell's origin owns; and indices into the slab above are all larger than own indices.  So the smallest index of every
 *   component of a part taken alone -- a LOCAL component -- is an own vertex, its local root.  And: two local components of one slab can be joined through
 *   another slab only (two columns that meet in the slab above), so merging neighbouring slabs pair by pair is not enough: the merge is transitive
 *   over all seams.
 * Protocol.  Three steps per slab and one host merge; no float anywhere, and arrival order decides nothing (flags and scans; the union-find's links only
 *   point to a smaller index).
 * 1. tsdf_mesh_slab_components labels the linked part on the context's stream, over the own vertices plus the span of indices into the slab above that
 *   tsdf_mesh_slab_link's check knows, synchronises, and builds three lists on the device, every index in them GLOBAL:
 *   down records (only when slab_z0 > 0): for every own vertex owned by a lattice point of plane 0 of the first owned lattice tile layer -- the vertices
 *          the slab below can index -- {vertex, root}, ascending by vertex.  tsdf_mesh_seam_vertex, 8 bytes.
 *   up records: for every vertex of the slab above that a triangle of the part uses, {vertex, root}, root its local root (an own vertex), ascending by
 *          vertex.
 *   root records: for every distinct root in the two lists {root, rank, n_vertices, n_triangles}: rank = the local roots with a smaller index, the
 *          counts the local component's own vertices and the part's triangles in it; ascending by root.  tsdf_mesh_seam_root, 16 bytes.
 *   out = {local components, down records, up records, root records}.  Timer "mesh_slab_components".
 *   tsdf_mesh_slab_component_seam copies the three lists (sized by out[1 .. 3]); any pointer may be NULL.
 * 2. tsdf_mesh_merge_component_seams is a pure host function: no context, no device.  Per slab, in slab order (tsdf_mesh_component_seams): vertex_base,
 *   n_vertices, the local component count and the three lists.  A union-find over all root records, the smaller root on top, joins each up record
 *   (g, r) of slab k with the down record (g, r') of slab k + 1; down records no up record matches are ignored.  Output per slab: component_base[k] =
 *   the components whose representative lies in the slabs below, and one tsdf_mesh_component_link (32 bytes) per root record, in the same order, slab
 *   after slab: {root, final_root, component, 0, n_vertices, n_triangles, 0, 0} -- the final component's global number and the WHOLE component's totals.
 *   A surviving boundary root is numbered component_base + rank - (removed roots of that slab with a smaller index), removed = under a smaller final
 *   root; this is what step 3's scan gives.  *n_components = the total.  TSDF_ERR_INVALID_ARGUMENT, nothing written: an up record without its down
 *   record, a list that is not strictly ascending, a root outside its slab, slabs out of order.  rgbd-recon_amd/binding.py has its numpy twin.
 * 3. tsdf_mesh_slab_link_components takes the slab's component_base and its links.  The host validates before any launch -- a bad index never reaches a
 *   scatter --: n_links equals the exported root count; links[i].root is exported root i; final_root <= root; final_root == root, or final_root <
 *   vertex_base, or it is another exported root of this slab.  TSDF_ERR_INVALID_ARGUMENT otherwise, the state untouched.  Then, on the device: the links
 *   are scattered to their roots, the own final representatives flagged and scanned for the numbering, and vertex_component, triangle_component (any of
 *   the three vertices: they agree) and the owned table rows written, boundary components with the links' totals.  *n_owned (may be NULL) = the rows.
 *   It may be called again with other links.  Timer "mesh_slab_components_link".
 *   tsdf_mesh_slab_download_components copies the three results; any pointer may be NULL.
 * tsdf_mesh_slab_component_stats: out = {local components, components owned (0 before step 3), seam records down + up, local roots removed}.
 * Lifetime.  The labels belong to the linked part: released by the next tsdf_mesh_slab_extract, by a new tsdf_mesh_slab_link (they hold global
 *   indices), tsdf_set_voxel_size and tsdf_destroy.  An empty part (zero vertices) launches nothing and answers zeros.
 * Errors.  TSDF_ERR_STATE before a link; for _seam and _link_components before step 1; for _download_components before step 3; for _stats without a
 *   part.  -1 for a NULL context.  TSDF_ERR_INVALID_ARGUMENT for a NULL out, and for NULL links with n_links > 0.  TSDF_ERR_OUT_OF_MEMORY leaves the
 *   state as it was.  tsdf_mesh_components keeps answering TSDF_ERR_STATE on a Z-slab context.
 * Out of scope.  Filtering the parts themselves (a per-part compaction and a second link with a per-seam-vertex remap: the links carry the whole
 *   component's totals so that every slab can decide a keep rule without another exchange; the joined mesh is filtered on the host, binding.py:
 *   drop_mesh_components).  Filtered part rings.  The native RCCL exchange: the lists travel by whatever carries the caller's other collectives
 *   (rgbd-recon_amd/multigpu.py: SlabDriver.mesh_components). */
typedef struct tsdf_mesh_seam_vertex { uint32_t vertex, root; } tsdf_mesh_seam_vertex;
typedef struct tsdf_mesh_seam_root { uint32_t root, rank, n_vertices, n_triangles; } tsdf_mesh_seam_root;
typedef struct tsdf_mesh_component_link { uint32_t root, final_root, component, reserved0 /* 0 */, n_vertices, n_triangles, reserved1 /* 0 */, reserved2 /* 0 */; } tsdf_mesh_component_link;
typedef struct tsdf_mesh_component_seams {
  uint64_t vertex_base, n_vertices, n_local, n_down, n_up, n_roots;
  const tsdf_mesh_seam_vertex* down; const tsdf_mesh_seam_vertex* up; const tsdf_mesh_seam_root* roots;
} tsdf_mesh_component_seams;
int32_t tsdf_mesh_slab_components(tsdf_ctx* ctx, uint64_t out[4]);
int32_t tsdf_mesh_slab_component_seam(tsdf_ctx* ctx, tsdf_mesh_seam_vertex* down, tsdf_mesh_seam_vertex* up, tsdf_mesh_seam_root* roots);
int32_t tsdf_mesh_merge_component_seams(const tsdf_mesh_component_seams* slabs, uint32_t n_slabs, uint64_t* component_base, tsdf_mesh_component_link* links, uint64_t* n_components);
int32_t tsdf_mesh_slab_link_components(tsdf_ctx* ctx, uint64_t component_base, const tsdf_mesh_component_link* links, uint64_t n_links, uint64_t* n_owned);
int32_t tsdf_mesh_slab_download_components(tsdf_ctx* ctx, uint32_t* vertex_component, uint32_t* triangle_component, tsdf_mesh_component* table);
int32_t tsdf_mesh_slab_component_stats(tsdf_ctx* ctx, uint64_t out[4]);

/* ---- mesh streaming: the filtered frame -------------------------------------------------------------------
 * The ring of "mesh streaming" above with the keep rule of "mesh components" inside it: a streamed frame is already the mesh without its small
 * components, decided and compacted on the device.  The ring's guarantees stay whole: no host wait, no allocation after the first call, never a partial
 * frame, identical bytes on every run.  No counterpart in the reference.  tests/mesh_stream_filter_reference.py composes the definition from the
 * extraction's, the components' and the packing's numpy references; device and numpy agree byte for byte.
 *
 * tsdf_mesh_stream_config_filter is tsdf_mesh_stream_config_lod with min_triangles; with min_triangles == 0 it IS that call (which is this one with
 *   0): no filter, and tsdf_mesh_stream runs the launches, events and copies it ran before this entry existed.  min_triangles >= 1 selects the filtered
 *   path; 1 keeps every component and still goes through the filter.  Argument checks and error codes are tsdf_mesh_stream_config_lod's.
 *   tsdf_mesh_stream_min_triangles reports the configured value (TSDF_ERR_STATE before any config, TSDF_ERR_INVALID_ARGUMENT for a NULL pointer).
 * The filtered frame.  Take the mesh tsdf_mesh_extract_lod(flags, level) defines for the volume; label its components by index; drop every component
 *   whose table entry has n_triangles < min_triangles; kept vertices and triangles stay in their order, indices are remapped to the number of kept
 *   vertices before them, the winding is untouched; pack what is left by the mesh streaming section's rule.  Packing is per vertex, so packed rows move
 *   bit for bit: pack(keep(mesh)) == pack(mesh)[kept].
 * tsdf_mesh_frame keeps its 112-byte layout.  n_vertices and n_triangles are the FILTERED counts, and the payload copied to the host is exactly
 *   n_vertices * vertex_stride + n_triangles * 12 bytes of them.  needed_vertices / needed_triangles / needed_tiles stay the needs of the UNFILTERED
 *   mesh, and the three capacities bound the unfiltered mesh: it is emitted whole on the device (into a raw buffer of the configuration, not the
 *   slot) before anything is dropped, so a frame whose filtered mesh would fit still overflows when the unfiltered one does not.  An overflow is what
 *   it is without a filter: the bits, the needs, zero counts, no filter run.  A frame whose every component is dropped has zero counts, overflow == 0
 *   and no payload copy.  There is no component capacity and no fourth overflow bit: the filter keeps one triangle count per vertex, not a table.
 * tsdf_mesh_stream_frame_filter: out = {components of the unfiltered mesh, components kept, vertices removed, triangles removed} of the frame
 *   currently HELD (between tsdf_mesh_stream_acquire and tsdf_mesh_stream_release); all four 0 for an overflowed frame.  TSDF_ERR_STATE when no frame
 *   is held or when the ring is configured without a filter; TSDF_ERR_INVALID_ARGUMENT for a NULL out.  The four words travel in a 64-byte record in
 *   front of the slot's 64-byte header, in the header's copy; header and payload are where they were.
 * Protocol.  count, scan, raw header, emit (into the raw buffer) as before; draw_done is recorded again right behind the emit, so an integrate()
 *   that overwrites the volume set never waits for the filter, which reads no volume.  Then the filter: every launch is sized by the configured
 *   capacities and reads the frame's counts from the raw header on the device, so the host never learns a count before the final header arrives.  The
 *   slot's final header is written by a last one-lane launch and copied to the host behind it; the payload copy is queued, as ever, by whichever call
 *   first sees the header on the host.  The raw buffer (header + capacity-sized payload) and the filter's scratch (13 bytes per capacity vertex and
 *   the scans' block sums) are allocated by the first tsdf_mesh_stream after a config, counted in tsdf_mesh_stream_stats' device bytes and freed
 *   with the ring.  Timer "mesh_stream_filter": everything between the emit and the final header, the header's launch included. */
int32_t tsdf_mesh_stream_config_filter(tsdf_ctx* ctx, uint32_t flags, uint32_t level, uint32_t min_triangles, uint32_t max_vertices, uint32_t max_triangles,
                                       uint32_t max_surface_tiles, uint32_t slots);
int32_t tsdf_mesh_stream_min_triangles(tsdf_ctx* ctx, uint32_t* min_triangles);
int32_t tsdf_mesh_stream_frame_filter(tsdf_ctx* ctx, uint64_t out[4]);

/* ---- mesh streaming: compact triangles ---------------------------------------------------------------------
 * The ring of "mesh streaming" with triangles of 6 bytes instead of 12: three 16-bit corner codes that name a vertex by its lattice tile and its place
 * inside it, and a table with one 16-byte row per lattice tile of the frame.  The mesh, its order, its winding and its packed vertices are unchanged;
 * decoding gives, byte for byte, the uint32 triangle array of the same frame -- at every level, and of the filtered frame with a filter.  No
 * counterpart in the reference.  tests/mesh_compact_reference.py restates the format in numpy; device and numpy agree byte for byte.
 *
 * Why 15 bits name a corner.  The mesh is ordered by 8^3 lattice tile; a vertex is owned by the lower end of its edge; the corners of a cell lie in the
 *   cell's tile or in one of its +x / +y / +z neighbours.  (a) offset < 3584: a tile has 512 lattice points, a point owns at most 7 edges, so a tile
 *   owns at most 512 * 7 = 3584 vertices and an offset inside it fits 12 bits.  (b) A tile with triangles has a row: every one of Kuhn's tetrahedra
 *   contains the cell's origin c0, so a tetrahedron with mixed signs has a crossed edge at c0; that edge is owned by c0, and c0 lies in the cell's own
 *   tile -- the tile of every triangle owns a vertex.  Hence the rows are exactly the needed_tiles tiles max_surface_tiles bounds: there is no fourth
 *   capacity and no fourth overflow bit.  The neighbour code 7 never occurs (corner 7 of a cell owns no edge of that cell).
 * Payload.  In this order: the packed vertices, n_vertices * vertex_stride bytes, unchanged; zero padding up to a multiple of 16 (eight bytes
 *   or none); the tile table, n_tile_rows rows of 16 bytes; the triangles, n_triangles rows of 6 bytes.  Little endian.  The
 *   payload copied to the host is exactly these bytes, never the capacity; a frame without a vertex has no payload.
 * Tile-table row.  {uint32 tile, first_vertex, first_triangle, n_triangles}: one row per lattice tile that owns at least one vertex of the frame,
 *   ascending by tile; tile is the linear id, x fastest, in the level's lattice-tile grid tiles[a] = ceil(ceil(res[a] / s) / 8), s = 1 << level.  The
 *   tile's vertices are [first_vertex, the next row's first_vertex) -- the last row's end at n_vertices --, its triangles (those of its cells)
 *   [first_triangle, first_triangle + n_triangles), both in the frame's order.
 * Triangle row.  Three uint16 corner codes in the corner order of the uint32 array.  Bits 0..11: index - first_vertex of the owner tile's row.  Bits
 *   12..14: dx + 2 dy + 4 dz, the owner tile's position relative to the tile of the triangle's cell, each component 0 or 1.  Bit 15: 0.
 * Decoding, for corner code `code` of a triangle in row r (rows[] the table, n its length):
 *     owner = rows[r].tile + ((code >> 12) & 1) + ((code >> 13) & 1) * tiles[0] + ((code >> 14) & 1) * tiles[0] * tiles[1];
 *     lo = r; hi = n;                       // the owner's row: rows ascend by tile, and owner >= rows[r].tile
 *     while (hi - lo > 1) { mid = (lo + hi) / 2; if (rows[mid].tile <= owner) lo = mid; else hi = mid; }
 *     index = rows[lo].first_vertex + (code & 0xfff);
 * tsdf_mesh_stream_config_compact is tsdf_mesh_stream_config_filter with index_format.  TSDF_MESH_INDEX_U32 (0): it IS that call (which is this one
 *   with 0, as the two older config entries are): the launches, events and copies of before.  TSDF_MESH_INDEX_TILE16 (1): the format above.  Any other
 *   value: TSDF_ERR_INVALID_ARGUMENT.  Every other check and error code is tsdf_mesh_stream_config_filter's.  With format 1 a slot is the 64-byte header
 *   + align16(max_vertices * vertex_stride) + max_surface_tiles * 16 + max_triangles * 6 bytes, and the 4 GiB bound applies to that size.
 *   tsdf_mesh_stream_index_format reports the configured format (TSDF_ERR_STATE before any config, TSDF_ERR_INVALID_ARGUMENT for a NULL pointer).
 * tsdf_mesh_frame keeps its 112 bytes.  In a frame of format 1 `triangles` is NULL; n_vertices, n_triangles, the needs, overflow and the rest mean
 *   what they mean in format 0, and the three capacities overflow as they do there (zero counts, zero rows, no payload copy).
 * tsdf_mesh_stream_frame_compact fills *out for the frame currently HELD: the table, the codes, the number of rows, the level's tile grid and the
 *   level.  The pointers go into the slot's pinned buffer and are valid until tsdf_mesh_stream_release.  An overflowed frame and a frame whose every
 *   component was dropped have zero rows.  TSDF_ERR_STATE when no frame is held or the ring has format 0; TSDF_ERR_INVALID_ARGUMENT for a NULL out.
 * tsdf_mesh_stream_stats counts the payload bytes that were copied: the compact sizes.
 * With a filter (min_triangles >= 1) the device's raw buffer keeps the unfiltered uint32 frame and its tile table; the kept triangles are coded against
 *   the filtered table: a row stays iff it keeps a vertex, first_vertex counts the kept vertices before it, first_triangle and n_triangles are
 *   recounted over the kept triangles (a kept triangle keeps its three vertices, so its row stays).  The filtered row count travels in the 64-byte
 *   record in front of the header.  tsdf_mesh_stream_frame_filter answers as before.
 * Protocol: that of the ring.  The table is one launch more in the emit (a lane per lattice tile writes its row at the tile's surface ordinal), and with
 *   a filter one single-workgroup launch more in the filter (the rows that stay); no host wait and no allocation after the first call is added.
 * Out of scope: a compact form for tsdf_mesh_download and the PLY; slab parts (a Z-slab context refuses the ring as before); texture taps in the ring;
 *   any change to the vertex packing; entropy coding. */
#define TSDF_MESH_INDEX_U32    0u
#define TSDF_MESH_INDEX_TILE16 1u
typedef struct tsdf_mesh_tile_row { uint32_t tile, first_vertex, first_triangle, n_triangles; } tsdf_mesh_tile_row;
typedef struct tsdf_mesh_compact {
  const tsdf_mesh_tile_row* table;   /* n_tile_rows rows, ascending by tile */
  const uint16_t* triangles;         /* n_triangles (of the tsdf_mesh_frame) rows of three corner codes */
  uint64_t n_tile_rows;
  uint32_t tiles[3];                 /* the level's lattice-tile grid */
  uint32_t level;
} tsdf_mesh_compact;
int32_t tsdf_mesh_stream_config_compact(tsdf_ctx* ctx, uint32_t flags, uint32_t level, uint32_t min_triangles, uint32_t index_format, uint32_t max_vertices,
                                        uint32_t max_triangles, uint32_t max_surface_tiles, uint32_t slots);
int32_t tsdf_mesh_stream_index_format(tsdf_ctx* ctx, uint32_t* index_format);
int32_t tsdf_mesh_stream_frame_compact(tsdf_ctx* ctx, tsdf_mesh_compact* out);

/* ---- mesh streaming: slab parts ----------------------------------------------------------------------------
 * Where the volume exists only as Z-slabs, every slab context streams ITS PART of the compact frame above, every frame, through a ring of its own; the
 * receiver joins the parts by concatenation and two running sums.  A part is complete without a number from another slab: no exchange, no link step, no
 * host wait.  Why that is possible: a TSDF_MESH_INDEX_TILE16 corner code is not global -- it is the offset inside the owner tile | (dx, dy, dz) << 12.  For
 * a corner in the slab above (dz = 1, lattice plane 0 of the seam layer) the slab computes that offset itself from its halo, exactly as
 * tsdf_mesh_slab_extract computes its seam records ("mesh extraction on Z-slab contexts": plane 0 comes first in a tile, so its offsets depend on lattice
 * planes 0 and 1 alone); the owner tile's first_vertex lives in the owner's table row, which the slab above writes.  No counterpart in the reference.
 * tests/mesh_part_reference.py restates parts and join in numpy on top of the slab, packing and compact references; device and numpy agree byte for byte.
 *
 * tsdf_mesh_stream_config_part selects a ring whose frames are this context's part.  The index format is always TSDF_MESH_INDEX_TILE16; there is no filter
 *   (components cross slabs).  The checks and error codes are tsdf_mesh_stream_config_lod's, plus the alignment rule of tsdf_mesh_slab_extract, applied
 *   at config time: slab_z0 must be a multiple of 8 << level, slab_z1 too unless it is the volume's top; TSDF_ERR_INVALID_ARGUMENT otherwise.  A
 *   whole-volume context is the one-slab case: every frame of its part ring equals the frame of its compact ring byte for byte.
 *   tsdf_mesh_stream / _acquire / _release / _stats / _frame_compact / _level / _index_format serve the part ring unchanged; tsdf_mesh_frame keeps its
 *   112 bytes.  A Z-slab context configured through any of the four other config entries keeps answering TSDF_ERR_STATE from tsdf_mesh_stream, and a
 *   context that never calls this entry runs, launch for launch, what it ran before.
 * The part of a context that owns lattice tile layers [L0, L1) (as "mesh extraction on Z-slab contexts" defines them):
 *   vertices:   those owned by lattice points of these layers, in the order of the whole mesh, packed by the rule of "mesh streaming" (8 or 16 bytes).
 *               Normals and colours as on a slab extract.  Halo: the precondition and the argument of "mesh extraction on Z-slab contexts" hold as they
 *               stand there -- the halo is current, exchanged or recomputed, exactly as for a raymarch on the slab, and it covers every voxel a part reads.
 *               A slab that stores no layer above a face below the volume's top is refused by tsdf_mesh_stream with TSDF_ERR_STATE.
 *   table rows: one per OWNED lattice tile that owns a vertex, ascending.  `tile` is the linear id in the WHOLE level's lattice-tile grid
 *               (tsdf_mesh_compact.tiles); first_vertex and first_triangle are PART-LOCAL.
 *   triangles:  those of the cells whose origin lies in the owned layers: three corner codes each, exactly the codes of the whole-volume compact frame.
 *   Payload layout as in "compact triangles": vertices, zero padding to 16, rows, codes.
 * Capacities and overflow are per part, with the three bits of "mesh streaming".  needed_tiles and the rows count OWNED surface tiles only.  The seam
 *   layer's records need slots too: the ring allocates max_surface_tiles + ntx * nty record slots (the seam layer is one tile layer; none at the top), so
 *   a seam tile never causes an overflow and there is no fourth capacity.  needed_vertices, needed_tiles and the counts exclude the seam tiles; the
 *   subtraction happens on the device.
 * Join rule.  For parts k = 0 .. K-1 of contiguous slabs in slab order, all with overflow == 0:
 *     vertices:  concatenate the packed vertices;
 *     rows:      concatenate the rows with first_vertex += sum of n_vertices_j over j < k and first_triangle += sum of n_triangles_j over j < k;
 *     codes:     concatenate the codes unchanged.
 *   The result is, byte for byte, the frame a whole-volume context streams with tsdf_mesh_stream_config_compact(..., TSDF_MESH_INDEX_TILE16, ...).
 *   Only the top part decodes alone: below the top, codes with dz = 1 name rows of the next part, so the unit of decoding is the joined frame.  If any
 *   part overflowed, the frame is dropped whole.
 * tsdf_mesh_stream_frame_part fills *out for the frame currently HELD: layers = {L0, L1}, the level, top = 1 when the slab reaches the volume's top, and
 *   seam_tiles = the seam tiles with surface in this frame (it travels in a 64-byte record in front of the header, in the header's copy, as the filter's
 *   record does).  TSDF_ERR_STATE when no frame is held or the ring is not a part ring; TSDF_ERR_INVALID_ARGUMENT for a NULL out.
 * Protocol: that of the ring -- the same stream dependencies, events, pump and payload size rule; after the first call nothing is allocated and no call
 *   waits for the GPU.  Timers as "mesh streaming".
 * Out of scope: the filter, components and texture taps on parts; a uint32 part format; carrying parts over the native RCCL exchange; gaps between slabs;
 *   any change to the vertex packing or to the existing entries' behaviour. */
typedef struct tsdf_mesh_part { uint32_t layers[2]; uint32_t level; uint32_t top; uint32_t seam_tiles; uint32_t reserved[3]; } tsdf_mesh_part; /* 32 bytes */
int32_t tsdf_mesh_stream_config_part(tsdf_ctx* ctx, uint32_t flags, uint32_t level, uint32_t max_vertices, uint32_t max_triangles, uint32_t max_surface_tiles,
                                     uint32_t slots);
int32_t tsdf_mesh_stream_frame_part(tsdf_ctx* ctx, tsdf_mesh_part* out);   /* of the frame currently HELD */

/* ---- mesh streaming: texture taps in the frame -------------------------------------------------------------
 * A streamed frame carries one blendColors colour per vertex: voxel resolution.  With TSDF_MESH_STREAM_TAPS every frame of the ring also carries, per
 * vertex and stream, the texture tap of "texture taps" above, packed to 8 bytes, so that a receiver that has the colour images textures the streamed
 * mesh at camera resolution by plain projective texturing -- without a second, unpacked mesh and without the calibration volumes.  One pass serves
 * every form of the ring (uint32 indices, level of detail, filtered, tile-local compact, slab parts).  No counterpart in the reference.
 * tests/mesh_tap_pack_reference.py restates packing and pass in numpy on top of tests/texture_tap_reference.py and tests/mesh_pack_reference.py; device
 * and numpy agree byte for byte.
 *
 * The point.  A streamed vertex carries its position as three uint16 codes q (bytes 0-5 of the packed vertex, at either stride).  The taps of a streamed
 *   vertex are taken at the position the RECEIVER reconstructs from those codes, not at the emit kernel's fp32 u: per axis u_q = (float) q / 65535.0f,
 *   one fp32 division, used as a unit-cube coordinate.  The pass therefore reads the frame's final packed rows (after the filter's scatter where there
 *   is one), needs nothing from the emit, and the receiver can check it.  u_q is at most half a code step, 0.5 / 65535 of the extent per axis, from the
 *   vertex's u.  At a depth discontinuity that is enough to flip dist < limit, or the nearest depth pixel, for a stream.  Measured with the numpy
 *   reference on the "3-streams" scene of tests/test_gpu_texture_taps.py at 37 x 43 x 35, 5 108 vertices: the receiver's rule on taps at u_q against
 *   taps at the exact u differs by 0.027 / 255 in the mean colour and by 22.7 / 255 at the worst single vertex; the branch (alpha) is the same at every
 *   vertex.  So no per-vertex closeness to the vertex colour is claimed: the caveat tsdf_mesh_texture_taps states already.
 * The values.  Per stream i, in stream order, exactly the four values of tsdf_texture_tap at the unit-cube point u_q by the definition of "texture
 *   taps": pc, pcol, the NEAREST depth, dist, quality gated by dist < limit; the frame slot is the one current at the tsdf_mesh_stream call.  u_q lies in
 *   [0, 1], so every pair is evaluated: the not-evaluated record cannot occur.
 * The packed tap, tsdf_packed_tap, 8 bytes, little endian: the fp32 tap at 16 bits a field.
 *   bytes 0-1, 2-3  u, v as uint16: (uint16) rint(min(max(x, 0), 1) * 65535.0f) -- the position's rule: the product in fp32, half-way cases to even; a
 *                   NaN coordinate packs as 0.  Clamping the coordinate to [0, 1] does not change a LINEAR, CLAMP_TO_EDGE fetch: outside [0, 1] both
 *                   texels of an axis are the edge texel, as they are at 0 and at 1 (for every coordinate whose product with the image size is finite).
 *   bytes 4-5, 6-7  quality, dist as IEEE binary16: converted from fp32 with round to nearest even, overflow to +-inf, binary16 subnormals kept, every
 *                   NaN 0x7E00.  (numpy's astype(float16) is this rule for every value that is not a NaN.)
 * Layout.  [n_vertices][N], vertex-major, N = num_streams, 8 * N bytes per vertex, in the order of the frame's vertices: of a filtered frame the
 *   FILTERED vertices, of a part the part's vertices.  Parts therefore join by concatenation, like the vertices.
 * The receiver's rule is unchanged: unpack with u = code / 65535.0f for the coordinates and the halfs widened to fp32 for the weights, then the rule of
 *   "texture taps" (blend_from_taps in the binding serves as it is).
 * Where the block lives.  At a fixed place in the slot, behind the payload's CAPACITY: align16(payload capacity of max_vertices, max_triangles,
 *   max_surface_tiles) bytes behind the payload's first byte, max_vertices * N * 8 bytes long.  It travels in a copy of its own, of exactly
 *   n_vertices * N * 8 bytes, queued with the payload copy.  The payload's layout, its single exact-size copy and tsdf_mesh_frame do not change.  The
 *   4 GiB bound of a configuration applies to the slot including this block (header, payload capacity, padding, block).
 *
 * tsdf_mesh_stream_config_taps amends the current configuration, after any of the five config entries: TSDF_MESH_STREAM_TAPS turns the block on, 0 turns
 *   it off.  Every tsdf_mesh_stream_config* call resets it to off, so the five entries mean exactly what they meant.  A change of the flag drops slots
 *   already allocated, as a re-config does; the next tsdf_mesh_stream allocates again.  tsdf_mesh_stream_tap_flags reports the flag.
 * tsdf_mesh_stream with the flag on needs calibration (cv_xyz_inv, cv_uv) of every stream and a frame, whatever the vertex flags, and takes the lane
 *   ahead as a stream dependency, as a coloured frame does; it never waits for the host and allocates nothing after the first call.  One more launch per
 *   frame, sized by max_vertices, which reads n_vertices from the slot's header on the device: behind the emit, on a filtered ring behind the final
 *   header (whose copy does not wait for it).  A frame that overflowed or is empty has no tap bytes.  It works on a Z-slab context through a part ring: a
 *   slab holds whole LUTs and frames.  A ring without the flag queues exactly the launches and copies it queued before.
 * tsdf_mesh_stream_frame_taps fills *out for the frame currently HELD: taps points into the slot's pinned buffer and is valid until the release;
 *   n_streams = N, tap_bytes = 8.  taps is non-NULL and n_vertices 0 for a held frame without vertices.
 * tsdf_mesh_stream_stats: out[2] counts the tap bytes copied too, out[3] the larger slots.  Timer "mesh_stream_taps".
 * Errors.  tsdf_mesh_stream_config_taps: TSDF_ERR_STATE before any config and while frames are queued or held (the rule of the config entries);
 *   TSDF_ERR_INVALID_ARGUMENT for any other bit, and when the slot with the block exceeds 4 GiB (the flag stays as it was).  tsdf_mesh_stream:
 *   TSDF_ERR_STATE without calibration or a frame, nothing queued.  tsdf_mesh_stream_frame_taps: TSDF_ERR_STATE when no frame is held or the ring has
 *   no taps; TSDF_ERR_INVALID_ARGUMENT for a NULL out.  tsdf_set_voxel_size and tsdf_destroy: the ring's rules. */
#define TSDF_MESH_STREAM_TAPS 1u
typedef struct tsdf_packed_tap { uint16_t u, v, quality_h, dist_h; } tsdf_packed_tap;   /* 8 bytes */
typedef struct tsdf_mesh_taps { const tsdf_packed_tap* taps; uint64_t n_vertices; uint32_t n_streams, tap_bytes; } tsdf_mesh_taps;   /* 24 bytes */
int32_t tsdf_mesh_stream_config_taps(tsdf_ctx* ctx, uint32_t tap_flags);
int32_t tsdf_mesh_stream_tap_flags(tsdf_ctx* ctx, uint32_t* tap_flags);
int32_t tsdf_mesh_stream_frame_taps(tsdf_ctx* ctx, tsdf_mesh_taps* out);   /* of the frame currently HELD */

/* ---- mesh component measures: exact area, volume and bounds per island --------------------------------------
 * "Mesh components" above knows an island by its counts alone, and a triangle count changes meaning with the resolution.  These entries give every
 * component of the labelled mesh its surface area, its signed volume, its bounds and its vertex centroid, on the device, and filter by them: "drop
 * everything smaller than 5 cm", "drop closed voids inside the subject".  Float sums by atomics would differ from run to run, so the measures are
 * DEFINED on an integer grid and summed in integers: exact, independent of the order, two runs give identical bytes.  No counterpart in the reference.
 * tests/mesh_measure_reference.py restates the definition in numpy and Python integers; device and numpy agree byte for byte.
 *
 * The measures belong to the labelled mesh of the last tsdf_mesh_components: any level, and also the mesh a keep / filter left once it has been
 *   labelled again.
 * Measure grid.  ext = bbox_max - bbox_min in fp32, as vol_to_world forms it; E = max(ext.x, ext.y, ext.z); scale = 1048576.0 / (double) E, one IEEE
 *   double division done on the host; unit = 1.0 / scale.  The grid is isotropic: one unit is the same length on every axis (areas and volumes mean
 *   nothing otherwise), 2^20 units along the longest edge of the box.
 * Grid coordinate of a vertex, per axis a: d = (double) position[a] - (double) bbox_min[a]; q = rint(d * scale), half-way cases to even, clamped to
 *   [0, 1048576]; NaN gives 0 (no extract produces one; the definition covers it).  Three double operations, each correctly rounded, none contracted
 *   into an fma.  q needs 21 bits; the three coordinates pack into one uint64 as qx | qy << 21 | qz << 42.
 * Per triangle (i0, i1, i2), in exact integer arithmetic: e1 = q1 - q0, e2 = q2 - q0; c = e1 x e2 (each component below 2^43); n2 = c . c (below 2^88);
 *   a2 = floor(sqrt(n2)), the doubled area in unit^2, rounded down; v6 = det(q0, q1, q2), six times the signed volume of the tetrahedron from the grid
 *   origin (bbox_min) in unit^3, |v6| < 2^63.  A triangle with an index that is not a vertex (no extract and no keep writes one) has a2 = v6 = 0.
 * Per component one row, tsdf_mesh_component_measure, 80 bytes, little endian:
 *   q_min[3], q_max[3]       uint32         bounds of the component's vertices' grid coordinates
 *   area2                    uint64         sum of a2 over the component's triangles
 *   volume6_lo, volume6_hi   uint64, int64  sum of v6 as one two's-complement 128-bit integer
 *   sum_q[3]                 uint64         sum of q over the component's vertices: the vertex centroid is sum_q / n_vertices
 *   reserved                 uint64         0
 *   A component without triangles has area2 = 0 and volume6 = 0.
 * Winding.  The normals point into empty space: a closed surface round solid matter has volume6 > 0, a closed void inside matter volume6 < 0.  For an
 *   OPEN component volume6 depends on the origin: it is the volume of the cone from bbox_min over the surface, not a property of the surface alone.
 * Conversion, tsdf_mesh_measure_grid {unit, origin = bbox_min, bits = 20}: area = area2 * unit^2 / 2; volume = volume6 * unit^3 / 6; world position
 *   = origin + q * unit.
 * Why 20 bits.  A unit is E / 2^20, about 2.1 um for the 2.2 m box: coarser than an fp32 ulp of the positions there, and 2 000 units per voxel at 512^3.
 *   Rounding each triangle's doubled area down to a whole unit^2 costs below 1e-6 of its area there, and v6 still fits one signed 64-bit word.
 *
 * tsdf_mesh_component_measures computes the rows on the context's stream (a fill of the rows and three launches: vertices, triangles, finish; no host
 *   wait between them), synchronises like tsdf_mesh_components and fills *grid (may be NULL).  Timer "mesh_component_measures": fill and launches.  The rows and a scratch of 8 bytes per
 *   vertex (the packed coordinates) live beside the labels and die with them: next extract, keep / filter, a new tsdf_mesh_components,
 *   tsdf_set_voxel_size, destroy.  It may be called again.  It allocates before it replaces anything: TSDF_ERR_OUT_OF_MEMORY leaves the state as it was.
 *   Mesh, labels and table are untouched.
 * tsdf_mesh_download_component_measures copies the C rows.
 * tsdf_mesh_measure_grid_info fills *grid without a mesh: the grid is a property of the box.
 * tsdf_mesh_filter_components_measured: a component stays iff every clause of the rule holds: n_triangles >= min_triangles; max over the axes of
 *   (q_max[a] - q_min[a]) >= min_extent; area2 >= min_area2; |volume6| >= min_abs_volume6; with TSDF_MESH_RULE_POSITIVE_VOLUME, volume6 > 0.  The
 *   thresholds are grid integers, so the decision is exact, and it is taken on the device.  The rebuilt mesh is what tsdf_mesh_keep_components gives for
 *   those flags: the same scans and scatter, the same lifetime rules and stats, the timer "mesh_filter".  An all-zero rule keeps everything.
 * Errors.  TSDF_ERR_STATE without labels of the current mesh (so always on a Z-slab context), and for download / filter without measures of them;
 *   TSDF_ERR_INVALID_ARGUMENT for NULL rows, a NULL rule or a NULL grid of _grid_info, for rule.reserved != 0 and for an unknown flag.  -1 for a NULL context.
 * Unchanged.  tsdf_mesh_component_stats keeps its four words.  A context that never calls these entries runs exactly what it ran before they existed.
 * Out of scope.  Z-slab parts: a part's triangles index vertices of the slab above, whose positions it does not hold; the sums are additive, so a
 *   later change can export per-slab partial rows and add them through the existing links.  A measure rule inside the streamed filter ring: it keeps
 *   one triangle count per vertex, not a table.  Area-weighted centroids and inertia.  Welding. */
#define TSDF_MESH_RULE_POSITIVE_VOLUME 1u
typedef struct tsdf_mesh_component_measure {
  uint32_t q_min[3], q_max[3]; uint64_t area2; uint64_t volume6_lo; int64_t volume6_hi; uint64_t sum_q[3]; uint64_t reserved /* 0 */;
} tsdf_mesh_component_measure;                                              /* 80 bytes */
typedef struct tsdf_mesh_measure_grid { double unit; float origin[3]; uint32_t bits /* 20 */; } tsdf_mesh_measure_grid;   /* 24 bytes */
typedef struct tsdf_mesh_measure_rule { uint32_t min_triangles, min_extent; uint64_t min_area2, min_abs_volume6; uint32_t flags, reserved /* 0 */; } tsdf_mesh_measure_rule;   /* 32 bytes */
int32_t tsdf_mesh_component_measures(tsdf_ctx* ctx, tsdf_mesh_measure_grid* grid /* may be NULL */);
int32_t tsdf_mesh_download_component_measures(tsdf_ctx* ctx, tsdf_mesh_component_measure* rows /* [C] */);
int32_t tsdf_mesh_measure_grid_info(tsdf_ctx* ctx, tsdf_mesh_measure_grid* grid);   /* needs no mesh */
int32_t tsdf_mesh_filter_components_measured(tsdf_ctx* ctx, const tsdf_mesh_measure_rule* rule, uint64_t* n_vertices, uint64_t* n_triangles);

/* ---- frame read-out: the swap ------------------------------------------------------------------------
 * The client ends a frame with glfwSwapBuffers (source/kinect_client.cpp:533): an RGBA8 window goes to a display (GLFW's default framebuffer has 8
 * bits per channel and the client sets no window hint that changes it, :942-951).  This device has no display; tsdf_present is the swap for a host
 * that wants to SEE the frame: it converts the finished framebuffer to what the window would hold -- or to the DXT1 blocks of the system's wire format
 * (TSDF_COLOR_DXT1), 1/8 of that --, copies it into a ring of pinned host buffers on the context's copy stream, and hands finished frames out in
 * order while the lanes work on the next ones.  (tsdf_download_framebuffer stays what it was: synchronous, fp32, 20 bytes per pixel, for tests.)
 * tests/present_reference.py restates the definition in numpy; device and numpy agree byte for byte.
 *
 * RGBA8.  Per channel u = (uint8) rint(min(max(v, 0), 1) * 255.0f): the product in fp32, rint = round to nearest, half-way cases to even; NaN maps to
 *   0, -inf to 0, +inf to 255.  This is the float -> unsigned-normalised conversion of GL 4.4 section 2.3.5.2; GL only RECOMMENDS round-to-nearest
 *   there, an implementation may do otherwise, this library always rounds so.  Alpha is converted like the colour channels: the framebuffer's
 *   alpha = -1 "fallback" pixels become 0.  Four bytes r, g, b, a per pixel, w * h * 4 bytes.
 * Row order.  Bottom row first (row j = GL window row j, the library's convention); with TSDF_PRESENT_TOP_DOWN output row j is window row h - 1 - j.
 *   DXT1 blocks are cut from the image in its OUTPUT orientation.
 * DXT1.  Opaque four-colour mode only.  ceil(w / 4) x ceil(h / 4) blocks, row-major over blocks, 8 bytes each: c0 (u16, little endian), c1 (u16 LE),
 *   index word (u32 LE) with texel i = 4 y + x at bits 2i .. 2i + 1.  Texels outside the image replicate the last column / row (clamped coordinates).
 * DXT1 encoder.  On the converted 8-bit r, g, b (alpha is dropped), in integer arithmetic only:
 *   1. lo[c], hi[c] = per-channel min / max over the block's 16 texels;
 *   2. inset[c] = (hi[c] - lo[c]) >> 4, lo' = lo + inset, hi' = hi - inset;
 *   3. endpoint A = hi', endpoint B = lo' -- except that for c in {r, b} with cov = 16 * sum(c * g) - sum(c) * sum(g) < 0 (sums over the 16
 *      texels; fits 32 bits) A takes lo'[c] and B takes hi'[c]: the block's diagonal (a channel that falls where green rises);
 *   4. each endpoint is quantised r >> 3, g >> 2, b >> 3 and packed 565 (r in the high bits);
 *   5. c0 = the larger of A565 and B565, c1 = the smaller;
 *   6. c0 == c1: the index word is 0;
 *   7. otherwise both are expanded by bit replication ((r5 << 3) | (r5 >> 2), (g6 << 2) | (g6 >> 4)), p2 = (2 p0 + p1) / 3 and p3 = (p0 + 2 p1) / 3 in
 *      integer division -- the palette this library's own DXT1 decoder (tsdf_upload_wire_frame) produces --, and a texel's index is the k = 0..3 with
 *      the smallest summed squared r, g, b difference, the lowest k among equals.
 *
 * The ring.  tsdf_present_config sets format, flags and the number of slots (2..8; a context starts with RGBA8, no flags, 3 slots); each slot is a
 *   device buffer, a pinned host buffer and a ready event, allocated by the first tsdf_present.  tsdf_present(tag) takes the next free slot --
 *   TSDF_ERR_STATE and nothing queued when every slot is queued or held --, queues the conversion on the context's stream behind everything queued so
 *   far (the hole filling and any overlay since: the finished frame) and the copy on the copy stream behind it.  It never blocks the host, and the
 *   framebuffer is free for the next frame as soon as the conversion has run (the copy reads the slot's device buffer).
 *   tsdf_present_acquire hands out the oldest presented frame not yet released, in the order of the tsdf_present calls: *data points at the slot's
 *   pinned buffer (valid until tsdf_present_release), *bytes its size, *tag the tag, size = {w, h}; bytes, tag and size may be NULL.  wait != 0: the call
 *   waits for that frame's copy.  wait == 0: while the copy has not finished the call returns TSDF_OK with *data = NULL (never a partial frame).
 *   TSDF_ERR_STATE with nothing queued, or with a frame already held.  tsdf_present_release frees the held slot (TSDF_ERR_STATE when none is held).
 *   While frames are queued or held, tsdf_present_config and tsdf_resize return TSDF_ERR_STATE.  tsdf_destroy drains the ring.
 *   Timer "present" brackets the conversion kernel.  A context that never calls these runs exactly what it ran before they existed. */
#define TSDF_PRESENT_RGBA8 0u
#define TSDF_PRESENT_DXT1  1u
#define TSDF_PRESENT_TOP_DOWN 1u
int32_t tsdf_present_config(tsdf_ctx* ctx, uint32_t format, uint32_t flags, uint32_t slots);
int32_t tsdf_present_size(tsdf_ctx* ctx, uint64_t* bytes);     /* of one frame at the current view size and format */
int32_t tsdf_present(tsdf_ctx* ctx, uint64_t tag);
int32_t tsdf_present_acquire(tsdf_ctx* ctx, int32_t wait, const void** data, uint64_t* bytes, uint64_t* tag, uint32_t size[2]);
int32_t tsdf_present_release(tsdf_ctx* ctx);

/* ---- multi-GPU hooks (one context per rank; the collective itself is the caller's: RCCL) ---------- */
/* Halo = whole storage tile layers (8 voxel planes) next to the slab faces; sizes in bytes per face. */
int32_t tsdf_halo_info(const tsdf_ctx* ctx, uint32_t* layers, uint64_t* bytes_per_face);
/* copy this slab's lowest / highest `layers` tile layers into device buffers (either may be NULL) */
int32_t tsdf_halo_pack_dev(tsdf_ctx* ctx, void* lo_face_dev, void* hi_face_dev);
/* fill the halo below / above the slab from the neighbours' faces (NULL: keep) */
int32_t tsdf_halo_unpack_dev(tsdf_ctx* ctx, const void* below_dev, const void* above_dev);
/* partial image of this slab: [rgba 16 B | depth 4 B | nsamples 4 B] planar, 24 * w * h bytes */
int32_t tsdf_export_partial_dev(tsdf_ctx* ctx, void* dst_dev);
/* nearest-hit select over n gathered partial images into this context's raymarch target */
int32_t tsdf_composite_dev(tsdf_ctx* ctx, const void* gathered_dev, uint32_t n);
/* The same exchange in compact form: one 32-byte record {pixel, nsamples, depth, pad, rgba} per ray that hit inside this
 * slab, behind a 32-byte header {records written = min(hits, capacity), hits, overflow flag, ...}.  dst must hold
 * 32 + 32 * capacity bytes (a whole-volume context also ships one record per ray of its second march pass, hit or not: a miss is the
 * clear colour at depth 1 with the ray's sample count).  The hit list stays valid until the next tsdf_raymarch: a second call with a larger capacity
 * re-exports the same frame (how the slab driver repairs an under-sized gather without a per-frame host synchronisation). */
int32_t tsdf_export_hits_dev(tsdf_ctx* ctx, void* dst_dev, uint32_t capacity);
/* n record buffers, stride_bytes apart, composited into this context's raymarch target (rank 0) */
int32_t tsdf_composite_hits_dev(tsdf_ctx* ctx, const void* gathered_dev, uint32_t n, uint64_t stride_bytes);
/* ---- native multi-GPU exchange: one context per rank, one RCCL communicator, every collective on the context's
 * stream.  The reference's caller is C++ (source/kinect_client.cpp:569-614); with these it drives N GPUs without Python:
 *   rank 0: tsdf_comm_unique_id(id) -> the caller carries the 128 bytes to the other ranks (its own channel: the ZMQ socket, MPI, a file)
 *   every rank: tsdf_create(slab ...) ; tsdf_comm_init(ctx, id, rank, world, flags)
 *   per frame: tsdf_broadcast_frame(ctx, root, ...)   the frame arrives in ONE process (NetKinectArray.cpp:482-529)
 *              clear / mark / update bricks, integrate   (every rank that owns a slab)
 *              tsdf_halo_exchange(ctx)                   unless the contexts recompute their halo layers (slab_recompute_halo)
 *              tsdf_raymarch(ctx, mv, proj)
 *              tsdf_composite_gather(ctx)                hit records -> rank 0: nearest hit per pixel + fillColors(); no host sync
 *   before reading the frame: tsdf_composite_finish(ctx, &regathered)
 * TSDF_COMM_DEDICATED_COMPOSITOR: rank 0 holds no slab (its context only needs the view): it takes part in the collectives with empty
 * buffers, composites and fills holes while ranks 1 .. N-1 already work on the next frame.
 * RCCL is bound at run time (dlopen; a copy already loaded by the process -- torch's -- is reused). */
#define TSDF_COMM_ID_BYTES 128
#define TSDF_COMM_DEDICATED_COMPOSITOR 1u
int32_t tsdf_comm_unique_id(uint8_t id[TSDF_COMM_ID_BYTES]);
int32_t tsdf_comm_init(tsdf_ctx* ctx, const uint8_t id[TSDF_COMM_ID_BYTES], uint32_t rank, uint32_t world, uint32_t flags);
int32_t tsdf_comm_destroy(tsdf_ctx* ctx);
int32_t tsdf_broadcast_frame(tsdf_ctx* ctx, uint32_t root, const float* depth_rg, const float* quality, const float* silhouette, const uint8_t* colour_rgb);
int32_t tsdf_halo_exchange(tsdf_ctx* ctx);
int32_t tsdf_composite_gather(tsdf_ctx* ctx);
int32_t tsdf_composite_finish(tsdf_ctx* ctx, uint32_t* regathered);
/* gathers that tsdf_composite_finish had to repeat / frames that were composited from truncated record lists (0 in a healthy run) */
int32_t tsdf_comm_stats(tsdf_ctx* ctx, uint32_t* regathers, uint32_t* overflowed_frames);
/* Round 4 (VERDICT r03 "next" 5): the per-frame verdict behind `overflowed_frames` -- was frame `frame` (counted from 0 at the first
 * tsdf_composite_gather) composited from truncated record lists and not repaired?  *truncated 0 = complete, 1 = pixels may be missing.  Known at once
 * for the latest three frames, from a ring of the last 64 otherwise; TSDF_ERR_STATE = not gathered yet / too old.  The reference has no counterpart
 * (it renders on one GPU); multigpu.py's SlabDriver.frame_status is the same rule over torch.distributed. */
int32_t tsdf_comm_frame_status(tsdf_ctx* ctx, uint64_t frame, int32_t* truncated);
/* bounds of the per-frame gather size guess: at least min_records (default 4096), at most max_records (0: one per view pixel).  The frame
 * never depends on the guess (tsdf_composite_finish repairs a gather that was too small). */
int32_t tsdf_comm_set_capacity_limits(tsdf_ctx* ctx, uint32_t min_records, uint32_t max_records);

/* A whole-volume context marches in two passes: rays still running after `samples` samples are finished and shaded by a
 * wave-per-ray pass (0 switches the second pass off; the default is 24, or RR_MARCH_CAP).  A tuning knob: results do not depend on the
 * value, and tsdf_export_hits_dev ships the second pass's rays as well. */
int32_t tsdf_set_march_cap(tsdf_ctx* ctx, uint32_t samples);

/* ---- timers: the reference's TimerDatabase names: "2integrate", "3recon", "draw",
 * "holefill", "brickdraw", plus "bricks" (clear + mark + update).
 * "2integrate" brackets exactly the integrate kernel launch, "draw" exactly the raymarch kernel -------------------------------------------------------------- */
int32_t tsdf_enable_timers(tsdf_ctx* ctx, int32_t active);
/* every recorded event costs a few microseconds of stream time: restrict recording to a comma-separated list of timer names
 * (e.g. "2integrate") while measuring throughput; NULL or "" = all */
int32_t tsdf_set_timer_filter(tsdf_ctx* ctx, const char* names);
/* caller-defined intervals on the context's stream (recorded only while timers are enabled and `name` passes the filter),
 * and the individual samples of any timer since it was last read (resets it) */
int32_t tsdf_timer_reserve(tsdf_ctx* ctx, const char* name, uint32_t n);   /* create n event pairs now instead of on first use */
int32_t tsdf_timer_begin(tsdf_ctx* ctx, const char* name);
int32_t tsdf_timer_end(tsdf_ctx* ctx, const char* name);
/* Stage overlap (default on; RR_OVERLAP_FILL=0 in the environment turns it off at creation).  A frame's kernels form four chains that
 * touch disjoint state, and the context runs them on four HIP streams of its own, tied by events:
 *   the lane ahead      what a NEW frame needs before integrate(): its re-layout (tsdf_upload_frame / _dev) and the brick passes
 *                       (clear / mark / update) run while the context's stream still works on the previous frame; the frame slots and the
 *                       brick state exist twice and alternate
 *   the integrate lane  integrate() of frame f + 1 runs beside the draw of frame f: the volume, its tile classes and the tile lists exist
 *                       twice and alternate per integrate() (the TSDF is rebuilt from scratch every frame, recon_integration.cpp:249-250,
 *                       so nothing is carried from one set to the other).  Dense storage (whole volume, or a Z-slab that recomputes its halo); twice the volume
 *                       memory, allocated on the first integrate(); RR_DEEP=0 in the environment at creation keeps integrate() on the
 *                       context's stream and one volume
 *   the context's stream  depth limits, march, shading (and every collective / export)
 *   the fill lane       fillColors() of a draw runs beside the next frame's integrate() / draw; two pyramids alternate per draw
 * integrate() / draws wait (on the GPU) for the lanes they depend on, every download and tsdf_sync() for all of them.  Results are
 * identical either way.  The lane ahead is not used after an explicit frame-slot call (tsdf_select_frame_slot, tsdf_frame_staging, tsdf_upload_frame_async)
 * or with the pre-processing path.  tsdf_set_stage_overlap(ctx, 0) puts everything back on the one stream (synchronises first);
 * tsdf_timer_end_after_fill records a caller timer's end behind the hole filling in flight (a frame's latency). */
int32_t tsdf_set_stage_overlap(tsdf_ctx* ctx, int32_t on);
int32_t tsdf_timer_end_after_fill(tsdf_ctx* ctx, const char* name);
int32_t tsdf_timer_samples(tsdf_ctx* ctx, const char* name, float* out_ms, uint32_t capacity, uint32_t* count);
/* where every invocation of `name` since the last reset lies on the device's clock: begin and end in ms after the first begin of timer
 * `origin` (a timeline of the lanes; does not reset the timers) */
int32_t tsdf_timer_spans(tsdf_ctx* ctx, const char* name, const char* origin, float* begin_ms, float* end_ms, uint32_t capacity, uint32_t* count);
int32_t tsdf_timer_ms(tsdf_ctx* ctx, const char* name, float* last_ms);   /* synchronises on that timer */
/* every invocation since the previous call: count and summed device time; resets the timer */
int32_t tsdf_timer_stats(tsdf_ctx* ctx, const char* name, uint32_t* count, float* total_ms);

#ifdef __cplusplus
}
#endif
#endif /* RGBD_RECON_HIP_H */
