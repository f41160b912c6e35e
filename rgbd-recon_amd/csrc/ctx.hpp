// Host-side state of one context (private to the library: abi.cpp, comm.cpp).
#pragma once
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "tsdf_common.hpp"
#include "image_tiles.hpp"
#include "lane_ahead.hpp"
#include "draw_lanes.hpp"
#include "frame_intake.hpp"
#include "result_paths.hpp"
#include "volume_sets.hpp"
#include "slab_exchange.hpp"
#include "ray_staging.hpp"
#include "texture_taps.hpp"
#include "mesh_cc_seams.hpp"

using namespace rr;

extern thread_local std::string g_create_error;

// One named timer = a pool of event pairs, one pair per invocation since the last tsdf_timer_stats()
struct Timer { std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; size_t used = 0; bool open = false; };
constexpr size_t kMaxTimerPairs = 8192;

struct BrickRange { uint32_t lo[3], hi[3]; };

struct tsdf_ctx {
  tsdf_config cfg{};
  std::string err;
  int device = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  // volume
  int res[3]{};
  float vox[3]{};
  Volume vol{};
  TileState tiles{};
  int halo_layers = 0;
  // bricks
  float brick_req[3]{};          // requested size (setBrickSize argument)
  Bricks br{};
  std::vector<BrickRange> ranges;
  uint8_t* d_brick_tables = nullptr;   // the 21 voxel <-> brick <-> tile tables as one blob (BrickPlan, grid_plan.hpp); Bricks's table members point into it
  uint32_t* d_occ_counts = nullptr;   // three occupied-brick count words: two used alternately (see Bricks::num_occupied), one spare (lane_ahead.hpp)
  uint32_t min_voxels = 10;      // recon_integration.cpp:59
  size_t counter_words = 0;
  // two counter buffers: while frame f uses one, integrate(f)'s classify launch zeroes the other (part D of k_classify_lists), and
  // clearOccupiedBricks() of frame f + 1 is a pointer swap instead of a fill launch (which one is in use: lane_ahead.hpp)
  uint32_t* d_counters[2]{};
  uint32_t* h_num_occupied = nullptr;   // pinned
  // calibration + frame
  StreamTable luts{};
  void* lut_alloc[TSDF_MAX_STREAMS][3]{};   // per stream: cv_xyz_inv, cv_uv, cv_xyz device copies (freed when the stream is re-calibrated)
  bool have_calib[TSDF_MAX_STREAMS]{};
  // the stream's per-tile LUT box against the integrate kernel's LDS budget: 0 = does not fit (global-memory kernel), 1 = the box fits
  // (direct 8-tap form), 2 = the separable passes' rows and planes fit as well (the fastest form)
  int lut_dz[TSDF_MAX_STREAMS]{};   // the most z-planes of the stream's inverse LUT any 8^3 tile of the volume touches
  int lds_ok[TSDF_MAX_STREAMS]{};
  int k1_form_cap = 3;           // RR_K1_FORM: 3 = no cap (separable LDS form; + the projection cache where a budget was given), 2 = separable LDS form, 1 = direct 8-tap form, 0 = global-memory kernel
  // projection cache (ProjCache, tsdf_common.hpp): pool + slot table allocated by the first integrate() that can use it, dropped with
  // the volume, invalidated by tsdf_set_calibration
  ProjCache proj{}; uint32_t* d_proj_words = nullptr; int proj_parity = 0; size_t proj_budget = 0; bool proj_failed = false; uint32_t* d_item_stats = nullptr;
  bool last_integrate_cached = false;
  IntegratePlan last_k1{};       // tsdf_integrate_form: the plan the last integrate() launched by (form -1: none since the volume was set up)
  FrameImages frame{};           // the CURRENT frame slot's images (what mark / integrate / draw read)
  // The frame intake: the state and its protocol are frame_intake.hpp's -- which of the two frame slots is current and what each holds, the two
  // pinned host rings, the raw frame and what the passes made of it, the read fences.  Here: the buffers and events it indexes
  FrameIntake intake{};
  struct FrameSlot { float4* dqs = nullptr; float* depth = nullptr; uchar4* color = nullptr; float4* ranges = nullptr; hipEvent_t ready = nullptr, released = nullptr; };
  FrameSlot slots[2];
  hipStream_t copy_stream = nullptr;
  uint8_t* h_stage[2]{}; hipEvent_t stage_done[2]{};   // pinned host staging ring of the async upload
  float* d_stage_depth = nullptr; float* d_stage_q = nullptr; float* d_stage_s = nullptr; uint8_t* d_stage_col = nullptr;
  uint8_t* d_astage = nullptr;   // device staging of the async upload (its own: the copy stream runs beside the compute stream)
  // pre-processing state (NetKinectArray side)
  PreParams pre{};
  float* d_raw = nullptr; float* d_depth2 = nullptr; float2* d_depth_rg = nullptr; float4* d_lab = nullptr; float2* d_depth_b = nullptr; float4* d_normal = nullptr;
  uint32_t* d_pre_blocks = nullptr; uint32_t pre_cand_cap = 0;   // [count | cand_list[cap] | blk_flag[blocks]] (PreBuffers)
  const uint8_t* pending_rgb = nullptr;   // RGB8 colour of the raw frame uploaded last (d_stage_col or the caller's array), while intake.raw says it is pending
  const float* raw_src = nullptr;   // the caller's raw depth (tsdf_upload_raw_frame_dev), while intake.raw says the passes read from it
  hipEvent_t read_fence[kReadFences]{};   // the read fences' events (frame_intake.hpp)
  bool have_limits[TSDF_MAX_STREAMS]{}, have_cam[TSDF_MAX_STREAMS]{};
  // the frustum overlay (tsdf_draw_frustums): per stream the forward LUT's corner samples and Frustum::getCameraPos, captured by tsdf_set_calibration
  float frustum_corner[TSDF_MAX_STREAMS][8][3]{}; float frustum_cam[TSDF_MAX_STREAMS][3]{}; bool have_frustum[TSDF_MAX_STREAMS]{};
  unsigned long long* d_calibvis_skipped = nullptr; uint64_t calibvis_points = 0;   // the TSDF overlay: grid points of the last draw, device count of those the empty-space test removed
  // frame ingest (readLoop / update): wire formats, pinned double buffer (the reference's double_pbo), device copy of the message
  uint32_t color_format = TSDF_COLOR_RGB8, depth_format = TSDF_DEPTH_F32;
  uint8_t* h_wire[2]{}; hipEvent_t wire_done[2]{};
  uint8_t* d_wire = nullptr; size_t wire_capacity = 0;
  // view
  int vw = 0, vh = 0;
  Atlas atlas{};
  float4* d_peels = nullptr; float* d_nsamples = nullptr;
  float4* d_peels_alt = nullptr;   // the second peel image (image_tiles.hpp); d_peels is the latest draw's (what tsdf_download_image returns)
  void* d_hits = nullptr; uint32_t* d_hit_counters = nullptr; int hit_parity = 0;
  // image-space dirty tiles: the state and its protocol are image_tiles.hpp's -- three masks in rotation, two peel images, two pyramids, when
  // the hole filling may keep to the dirty tiles, what the texture view may show.  Here: the buffers it indexes
  ImageTiles tiles_img{};
  uint8_t* d_touched[3]{};
  float4* atlas_color[2]{}; float* atlas_depth[2]{};   // the two pyramids (round 3; which one a draw takes: draw_lanes.hpp); c->atlas points at the one the latest draw used
  // per pyramid the tile byte mask the march leaves for the hole filling (k_inpaint.hip), and scratch masks of levels 1 / 2
  uint8_t* d_fill_mask[2]{}; uint8_t* d_lvl_mask[2]{}; uint64_t n_fills = 0, n_fills_by_tiles = 0;
  uint32_t* d_tri_z = nullptr; float4* d_tri_acc = nullptr; float min_length = 0.0125f;   // triangle-grid back-end; KinectCalibrationFile.cpp:96 default
  float2* d_mvt_vtx = nullptr; bool have_mvt = false;   // MVT back-end: the last draw's vertex stage, [N][W+1][H+1] (filtered depth m, lateral quality)
  uint32_t* d_pair_masks = nullptr;   // per work item of the integrate launch: this frame's (tile, stream) pair classes (k_pair_masks)
  uint4* d_work_recs = nullptr; bool use_recs = true;   // per work item of the integrate launch: the 16-byte record k_pair_masks leaves for k_integrate_tiles_rec (RR_K1_REC=0: off, A/B)
  float4* d_tile_bounds = nullptr; bool tile_bounds_valid = false;   // static per (stored tile, stream) LUT-box bounds, built on the first dense integrate after a calibration
  bool culled_ranges = true;      // RR_K1_CULLED_RANGES=0: no uniform-pair shortcut in culled launches (A/B hook; dense storage with a bounds table of at most 512 MiB only)
  bool use_ranges = true;         // RR_K1_RANGES=0: the dense integrate evaluates every voxel of every stream (A/B and test hook, read at creation)
  int march_box = 1;              // the dense march: 1 = LDS voxel boxes, 2 = two boxes per wave with the next one prefetched (round 4), 0 = gathers from global memory as in round 1; RR_MARCH_BOX overrides (A/B and test hook, read at creation)
  void* d_long = nullptr; uint32_t march_cap = 24;   // rays still running after march_cap samples go to the wave-per-ray pass (RR_MARCH_CAP, 0 = off)
  bool last_two_pass = false;     // the last march handed its long rays to the wave-per-ray pass (they are not on the hit list)
  bool own_miss_counts = false;   // this context has marched at this view size: its sample-count image holds the miss counts (-count, or count after a composite)
  unsigned long long* d_comp_key = nullptr;   // per-pixel bid of the compact composite (rank 0, allocated on first use)   // raymarch hit list (k_march -> k_shade)
  float4* d_fb_c = nullptr; float* d_fb_d = nullptr;
  float* d_linear = nullptr;     // scratch for volume up/download
  // frame read-out (tsdf_present): the window after the swap (kinect_client.cpp:533) as RGBA8 or DXT1, through a ring of slots -- device buffer (the
  // conversion kernel's output, on the context's stream), pinned host buffer (the copy stream's, behind `converted`), `ready` behind the copy.  Slots
  // are taken and handed out in order: which is written, which handed out, what is queued or held is the ResultRing's (result_paths.hpp; three slots until
  // tsdf_present_config).  Here: what it indexes, allocated by the first tsdf_present at a view size / format (`bytes`: for what; 0: nothing exists).
  struct PresentSlot { void* dev = nullptr; void* host = nullptr; hipEvent_t converted = nullptr, ready = nullptr; uint64_t tag = 0; };
  struct Present { PresentSlot slot[kMaxResultSlots]; ResultRing ring{3, 0, 0, false}; uint32_t format = 0, flags = 0; size_t bytes = 0; } present;
  bool async_upload_ready = false;   // ensure_async_upload ran through (copy_stream alone may be the read-out's)
  // mesh extraction (tsdf_mesh_extract): the arrays of the last extract, sized exactly from its counts, kept until the next extract, tsdf_set_voxel_size or
  // destroy; flags = the attributes it produced; stats = {tiles, tiles skipped by class, tiles with surface, bytes of mesh storage}.  Everything else an
  // extract allocates (per-tile counts, the lattice-point records) is gone when it returns.
  // MeshStore: the four arrays in device memory with the counts and flags that size them; abi.cpp's mesh_store_* allocate, free, size and download them
  // for the whole mesh and for a slab's part alike.
  struct MeshStore : MeshArrays { uint64_t nv = 0, nt = 0; uint32_t flags = 0; MeshStore() : MeshArrays{nullptr, nullptr, nullptr, nullptr} {} };
  struct Mesh : MeshStore { bool valid = false; uint64_t stats[4] = {0, 0, 0, 0}; } mesh;
  // a Z-slab's part of the mesh (tsdf_mesh_slab_extract): a state of its own, so that everything built on `mesh` keeps refusing on a slab context.  The
  // vertex arrays and the triangle array (sized from the counts; the triangles are written by tsdf_mesh_slab_link, `linked` says whether they have been),
  // and what a link needs again: the scratch over owned + seam tiles, the records, the device copy of the table it was handed.  seam_cnt: the seam
  // tiles' plane-0 vertex counts on the host (the link's index check).  All of it lives until the next slab extract, tsdf_set_voxel_size or destroy.
  struct MeshSlabPart : MeshStore { uint32_t* records = nullptr; uint32_t* above = nullptr;
                                    MeshScratch scratch{}; MeshSlab slab{}; int ntx = 0, nty = 0; std::vector<uint32_t> seam_cnt;
                                    bool valid = false, linked = false; uint64_t stats[4] = {0, 0, 0, 0};
                                    uint64_t vertex_base = 0, index_end = 0; } mslab;   // of the last link: the part's indices lie in [vertex_base, index_end)
  // the components of a slab's linked part (tsdf_mesh_slab_components / _link_components): they hold global indices, so they live until the next slab
  // extract OR link, tsdf_set_voxel_size or destroy.  Step 1 leaves label (the local root of every index of the part's index space, as a local index),
  // rank and the local table (a row per local component) and the three seam lists -- the root records on the host too: step 3 checks its links
  // against them --, step 3 the three result arrays.  Everything else a call allocates is gone when it returns.
  struct MeshSlabComponents { uint32_t* label = nullptr; uint32_t* rank = nullptr; tsdf_mesh_component* local = nullptr;
                              tsdf_mesh_seam_vertex* down = nullptr; tsdf_mesh_seam_vertex* up = nullptr; tsdf_mesh_seam_root* roots = nullptr;
                              std::vector<tsdf_mesh_seam_root> host_roots;
                              uint32_t* vertex = nullptr; uint32_t* triangle = nullptr; tsdf_mesh_component* table = nullptr;
                              uint64_t n_index = 0, n_local = 0, n_down = 0, n_up = 0, n_owned = 0, removed = 0; bool labelled = false, linked = false; } mslabc;
  // mesh components (tsdf_mesh_components): the labels and the table of the current mesh, beside it in device memory; released with the mesh and by a
  // keep / filter (the mesh they labelled is gone then).  n / largest: components and the largest one's triangles of that labelling; removed_*: what the
  // last keep / filter of this extract took away.  Everything else a call allocates is gone when it returns.
  // measure / packed (tsdf_mesh_component_measures): a row per component and the vertices' packed grid coordinates, beside the labels and released with them.
  struct MeshComponents { uint32_t* vertex = nullptr; uint32_t* triangle = nullptr; tsdf_mesh_component* table = nullptr; uint64_t n = 0, largest = 0;
                          uint64_t removed_vertices = 0, removed_triangles = 0; bool valid = false;
                          tsdf_mesh_component_measure* measure = nullptr; unsigned long long* packed = nullptr; bool measured = false; } mcomp;
  // mesh streaming (tsdf_mesh_stream): the mesh of every frame, packed, through a ring like the read-out's.  A slot's buffers start with the frame's 64-byte
  // MeshStreamHeader, the payload (packed vertices, then triangles) follows.  Events: header_written (context's stream, behind the header launch: the copy
  // stream's header copy waits for it), emitted (context's stream, behind the emit: the payload copy waits for it), header_ready / ready (copy stream, behind
  // the header / payload copy).  payload_issued: a later call has seen the header on the host and queued the payload copy (or found nothing to copy);
  // payload_bytes what it queued.  One persistent set of scratch serves every frame: the mesh launches of consecutive frames follow each other on the
  // context's stream.  The ring's protocol is the ResultRing's, as the read-out's.  Allocated by the first tsdf_mesh_stream after a config or a new grid.
  // With a filter (min_triangles >= 1, tsdf_mesh_stream_config_filter) the emit writes into filter.raw, header_written is recorded behind the filter's
  // final header and emitted behind its scatter; a slot's buffers then begin `lead` = 64 bytes in front of dev / host with the frame's
  // MeshStreamFilterRecord, so that record and header travel as one copy and the payload stays 64 bytes behind the header.
  // index_format 1 (tsdf_mesh_stream_config_compact): the payload is vertices, padding, tile table, 6-byte triangles (result_paths.hpp: MeshFrameLayout);
  // table_rows is what the pump read for the slot's frame: the header's needed_tiles, with a filter the record's table_rows.
  // tap_flags (tsdf_mesh_stream_config_taps): a slot ends with the block of packed texture taps, at MeshFrameLayout::tap_offset behind the payload's first
  // byte; taps_written (context's stream, behind the tap launch: the block's copy waits for it), tap_bytes what the pump queued beside the payload.
  struct MeshStreamSlot { uint8_t* dev = nullptr; uint8_t* host = nullptr; hipEvent_t header_written = nullptr, emitted = nullptr, header_ready = nullptr, ready = nullptr;
                          hipEvent_t taps_written = nullptr; size_t tap_bytes = 0;
                          uint64_t tag = 0; size_t payload_bytes = 0; bool payload_issued = false; int res[3] = {0, 0, 0}; size_t lead = 0; uint64_t table_rows = 0; };
  struct MeshStream {
    MeshStreamSlot slot[kMaxResultSlots];
    ResultRing ring{};
    MeshScratch scratch{}; uint32_t* records = nullptr;
    uint32_t flags = 0, level = 0, max_vertices = 0, max_triangles = 0, max_tiles = 0;   // level: tsdf_mesh_stream_config_lod (the scratch is sized by its lattice tiles)
    uint32_t min_triangles = 0;     // 0: no filter, the frame is emitted into its slot
    uint32_t index_format = 0;      // 0: uint32 triangles, 1: tile-local 6-byte triangles and a tile table
    uint32_t tap_flags = 0;         // TSDF_MESH_STREAM_TAPS: packed texture taps behind every frame (off after every config entry)
    MeshFrameLayout layout() const { return MeshFrameLayout{index_format, flags ? 16u : 8u}; }
    // part (tsdf_mesh_stream_config_part): every frame is this context's PART of the tile-local frame -- the owned lattice tile layers `slab` names (set with
    // the allocation), count and emit by k_mesh_slab.hip, the scratch over owned + seam tiles, max_tiles + slab.n_seam record slots, and a slot's buffers
    // begin `lead` = 64 bytes in front with the frame's MeshStreamPartRecord.  The one mode a Z-slab context streams in.
    bool part = false; MeshSlab slab{};
    MeshStreamFilter filter{};      // the raw buffer and the filter's scratch (null without a filter)
    bool configured = false, allocated = false;
    uint64_t frames = 0, overflowed = 0, bytes_copied = 0, device_bytes = 0;
  } mstream;
  // ray queries (tsdf_cast_rays / _dev, tsdf_view_rays): the synchronous form's device staging (result_paths.hpp: grown on demand, then kept), the hit
  // list k_rays_march compacts for k_rays_surface (kRayChunk records, allocated with the counters by the context's first cast; no cast after it
  // allocates), `words` = {hits, samples accounted for, samples fetched} as three 64-bit counters of the cast, then the list's 32-bit count at byte 32
  struct Rays { tsdf_ray* d_rays = nullptr; tsdf_ray_hit* d_hits = nullptr; tsdf_ray_surface* d_surf = nullptr; CallStaging staging{};
                RayHitRec* d_list = nullptr; unsigned long long* d_words = nullptr; uint64_t last_n = 0; bool cast = false; } rays;
  // texture taps (tsdf_texture_taps / _dev, tsdf_mesh_texture_taps): the synchronous form's device staging (result_paths.hpp: grown on demand, then kept),
  // the mesh form's results for the current extract (sized exactly; released with the mesh), `words` = {pairs with quality > 0, pairs not evaluated} of the
  // last call as kTapStatSlots pairs of 64-bit counters which the host sums (allocated with the context: no call allocates them), and the last call's point count
  struct TextureTaps { float* d_xyz = nullptr; tsdf_texture_tap* d_taps = nullptr; tsdf_sensor_tap* d_sensor = nullptr; CallStaging staging{};
                       tsdf_texture_tap* mesh_taps = nullptr; tsdf_sensor_tap* mesh_sensor = nullptr; uint64_t mesh_nv = 0; bool mesh_valid = false, mesh_has_sensor = false;
                       unsigned long long* d_words = nullptr; uint64_t last_n = 0; bool called = false; } taps;
  bool have_volume = false;          // integrate() or tsdf_upload_volume has written the volume since it was set up (what the mesh extraction may read)
  // flags (recon_integration.cpp:54-57)
  bool fill_holes = true, use_bricks = true, skip_space = true;
  bool draw_bricks = false;   // setDrawBricks (recon_integration.cpp:57,160-173): tsdf_draw_f ends with the occupied-brick wireframes
  int shade_mode = 0;
  // stereo modes of the client (source/kinect_client.cpp:616-669): viewport origin + viewport_offset uniform (side by side),
  // colour mask + "colour buffer not cleared before this draw" (anaglyph)
  int vp_org[2]{}; float vp_off[2]{};
  uint32_t color_mask_mode = 0; bool keep_color = false;
  // Stage overlap (round 3): the hole filling of draw f on `fill_stream` beside whatever the caller queues next, its calls issued by a helper thread
  // (abi.cpp: FillWorker), and a fourth lane, integrate() of frame f + 1 on `integ_stream` beside the draw of frame f.  The state and its protocol are
  // draw_lanes.hpp's -- which volume set and which pyramid are in use, what is in flight on the two lanes, which job of the helper a wait has to see
  // issued first.  Here: the streams, the events it indexes (fill_done[pyramid], draw_done[set]; integ_done; integ_gate: work queued on the context's
  // stream that the integrate lane must not overtake), the helper and the two volume sets
  DrawLanes lanes{};
  hipStream_t fill_stream = nullptr; hipEvent_t fill_done[2] = {nullptr, nullptr};
  struct FillWorker; FillWorker* fill_worker = nullptr; bool fill_thread = true;
  // The volume sets: the state and its protocol are volume_sets.hpp's -- which tile list and count word an integrate() writes and which it trusts, the
  // frame stamp, when it walks every tile.  Here: the buffers its indices select -- per set the volume, the class of every stored tile (owned + halo), the
  // stamps, the two active-tile lists and their two device counts (k_classify_lists).  vset[lanes.set()] is the set in use, bound into `vol` and `tiles`
  // (abi.cpp: bind_volume_set); setup_volume allocates it, the first integrate() on the lane the other one: contexts that integrate every stored layer,
  // with dense storage only; off with stage overlap off, with the projection cache, and with RR_DEEP=0.
  struct VolSet { float* data = nullptr; uint8_t* cls = nullptr; uint32_t* stamp = nullptr; uint32_t* list[2]{}; uint32_t* counts = nullptr; TileHistory history{}; } vset[2];
  hipStream_t integ_stream = nullptr; hipEvent_t integ_done = nullptr, integ_gate = nullptr, draw_done[2] = {nullptr, nullptr};
  bool deep = true;
  hipStream_t pre_lane = nullptr; bool pre_on_integ = false;   // the stream the current frame's preparation runs on (pre_stream, or integ_stream: RR_PRE_ON_INTEG)
  bool overlap_fill = true;      // RR_OVERLAP_FILL=0 / tsdf_set_stage_overlap(ctx, 0): everything on the one stream, as in rounds 1 and 2
  // ... and a third lane AHEAD of the context's stream (round 3), preparing frame f + 1 on `pre_stream` while the context's stream still works on frame f:
  // the state and its protocol are lane_ahead.hpp's -- the gate between the lanes and its deferred wait, which of the two frame slots, counter buffers
  // and occupancy sets the lane writes, what is zero already.  Here: the stream, the events (pre_gate[]: the two gate events it indexes) and the buffers
  LaneAhead ahead{};
  hipStream_t pre_stream = nullptr; hipEvent_t pre_done = nullptr, pre_gate[2] = {nullptr, nullptr}, src_ready = nullptr;
  uint8_t* d_flags[2]{}; uint32_t* d_occupied[2]{};                             // the two occupancy sets (Bricks::flags / occupied point at the latest update's)
  // The native multi-GPU exchange (comm.cpp: one RCCL communicator per context, every collective on the context's stream): the state and its protocol
  // are slab_exchange.hpp's -- who owns a slab, exports, sends and receives, which rows of the gathered halo are a rank's neighbours, and of the compact
  // composite which ring slot a frame's hit counts land in, the capacity it is gathered with, when tsdf_composite_finish gathers it again, which frames
  // were left truncated.  Here: the communicator and the buffers and events it indexes
  struct Comm {
    void* comm = nullptr;                     // ncclComm_t
    SlabRoles roles{};
    GatherBook book{};
    float* d_halo_send = nullptr; float* d_halo_gath = nullptr; size_t halo_floats = 0;   // 2 faces / world x 2 faces
    float* d_hitbuf = nullptr; float* d_hitparts = nullptr; size_t hit_floats = 0;        // 32-byte header + one 32-byte record per view pixel; rank 0: x world
    int32_t* d_counts = nullptr;              // [world][2]: records written, rays hit
    int32_t* h_counts[GatherBook::kRing] = {}; hipEvent_t counts_evt[GatherBook::kRing] = {};   // the ring of pinned copies of d_counts, an event behind each copy
    float* d_frame_stage = nullptr; size_t frame_stage_bytes = 0;                          // tsdf_broadcast_frame: the four arrays as delivered
  } comm;
  bool timers_on = false;
  std::string timer_filter;      // ",name,name," or empty = all
  std::map<std::string, Timer> timers;
};

#define CHECK_CTX(c) do { if (!(c)) return TSDF_ERR_INVALID_ARGUMENT; } while (0)
#define FAIL(c, code, ...) do { char _b[512]; snprintf(_b, sizeof(_b), __VA_ARGS__); (c)->err = _b; return (code); } while (0)
#define HIP_TRY(c, expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { FAIL(c, _e == hipErrorOutOfMemory ? TSDF_ERR_OUT_OF_MEMORY : TSDF_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); } } while (0)

// helpers defined in abi.cpp
namespace rrhost {
hipStream_t pre_enter(tsdf_ctx* c, bool defer_gate = false);     // (defer_gate: tsdf_frame_raw_dev's first calls; see lane_ahead.hpp) the lane a frame-preparing call queues its work on (the context's stream when the lane is off); opens the lane's frame
void pre_leave(tsdf_ctx* c, hipStream_t lane);   // ... and after queuing it
hipError_t join_pre(tsdf_ctx* c);       // GPU side: the context's stream waits for the lane; called by every consumer of a frame's images / brick state
void timer_begin(tsdf_ctx* c, const char* name);
void timer_end(tsdf_ctx* c, const char* name);
hipError_t join_fill(tsdf_ctx* c);      // GPU side: the context's stream waits for the hole filling in flight on the second stream
hipError_t join_integ(tsdf_ctx* c);     // GPU side: the context's stream waits for the integrate in flight on the fourth lane
hipError_t sync_ctx(tsdf_ctx* c);       // host side: both streams
RayTarget ray_target(tsdf_ctx* c);
}  // namespace rrhost
// file_io.cpp: binary little-endian PLY of host arrays (nrm / col may be null); 0 or TSDF_ERR_INVALID_ARGUMENT with *err set
int32_t rr_write_mesh_ply(const char* path, uint64_t nv, uint64_t nt, const float* pos, const float* nrm, const float* col, const uint32_t* tri, std::string* err);
