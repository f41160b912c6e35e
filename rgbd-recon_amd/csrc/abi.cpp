// C-ABI implementation (include/rgbd_recon_hip.h): host-side state of the HIP TSDF core.
// Mirrors the host logic of kinect::ReconIntegration (framework/reconstruction/recon_integration.cpp):
// setVoxelSize/setBrickSize/divideBox (:340-406,:462-472), draw() matrix set-up (:182-205),
// ViewLod::setResolution (framework/rendering/view_lod.cpp:24-50), the per-frame call order of
// source/kinect_client.cpp:569-599,614.  All device work goes to one HIP stream.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "tsdf_common.hpp"
#include "grid_plan.hpp"
#include "mesh_measure.hpp"

using namespace rr;

#include "ctx.hpp"

thread_local std::string g_create_error;

namespace rrhost {       // host-side helpers (shared with comm.cpp through ctx.hpp where declared there)

static_assert(kAtlasMaxLods == TSDF_MAX_LODS, "grid_plan.hpp mirrors TSDF_MAX_LODS");

// ---- small double-precision matrix kit (column-major), results rounded once to float
void mat_mul_d(const double* a, const double* b, double* o) {
  double r[16];
  for (int c = 0; c < 4; ++c)
    for (int row = 0; row < 4; ++row) {
      double s = 0;
      for (int k = 0; k < 4; ++k) s += a[k * 4 + row] * b[c * 4 + k];
      r[c * 4 + row] = s;
    }
  memcpy(o, r, sizeof(r));
}
// Gauss-Jordan with partial pivoting on [M | I]
bool mat_inv_d(const double* m, double* o) {
  double a[4][8];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) { a[r][c] = m[c * 4 + r]; a[r][4 + c] = (r == c) ? 1.0 : 0.0; }
  for (int col = 0; col < 4; ++col) {
    int piv = col;
    for (int r = col + 1; r < 4; ++r) if (fabs(a[r][col]) > fabs(a[piv][col])) piv = r;
    if (a[piv][col] == 0.0) return false;
    if (piv != col) for (int k = 0; k < 8; ++k) std::swap(a[piv][k], a[col][k]);
    const double inv = 1.0 / a[col][col];
    for (int k = 0; k < 8; ++k) a[col][k] *= inv;
    for (int r = 0; r < 4; ++r) if (r != col) {
      const double f = a[r][col];
      if (f != 0.0) for (int k = 0; k < 8; ++k) a[r][k] -= f * a[col][k];
    }
  }
  for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) o[c * 4 + r] = a[r][4 + c];
  return true;
}
Mat4 to_mat4(const double* d) { Mat4 r; for (int i = 0; i < 16; ++i) r.m[i] = (float)d[i]; return r; }

void release_view(tsdf_ctx* c) {
  for (int k = 0; k < 2; ++k) { hipFree(c->atlas_color[k]); hipFree(c->atlas_depth[k]); c->atlas_color[k] = nullptr; c->atlas_depth[k] = nullptr; }
  c->lanes.view_released();
  hipFree(c->d_peels); hipFree(c->d_peels_alt); c->d_peels_alt = nullptr; hipFree(c->d_nsamples); hipFree(c->d_fb_c); hipFree(c->d_fb_d);
  hipFree(c->d_long); c->d_long = nullptr;
  hipFree(c->d_tri_z); hipFree(c->d_tri_acc); c->d_tri_z = nullptr; c->d_tri_acc = nullptr;
  for (int k = 0; k < 3; ++k) { hipFree(c->d_touched[k]); c->d_touched[k] = nullptr; }
  for (int k = 0; k < 2; ++k) { hipFree(c->d_fill_mask[k]); hipFree(c->d_lvl_mask[k]); c->d_fill_mask[k] = nullptr; c->d_lvl_mask[k] = nullptr; }
  c->tiles_img.reset();
  hipFree(c->d_hits); hipFree(c->d_hit_counters); hipFree(c->d_comp_key); c->d_hits = nullptr; c->d_hit_counters = nullptr; c->d_comp_key = nullptr;
  c->atlas.color = nullptr; c->atlas.depth = nullptr; c->d_peels = nullptr; c->d_nsamples = nullptr; c->d_fb_c = nullptr; c->d_fb_d = nullptr;
}
// the read-out ring's buffers and events (nothing may be in flight: an idle ring, or behind a synchronisation of both streams)
void release_present(tsdf_ctx* c) {
  for (auto& S : c->present.slot) {
    hipFree(S.dev); if (S.host) hipHostFree(S.host);
    if (S.converted) hipEventDestroy(S.converted);
    if (S.ready) hipEventDestroy(S.ready);
    S = tsdf_ctx::PresentSlot{};
  }
  c->present.bytes = 0; c->present.ring.reset();
}
// the copy stream: made by whichever of the asynchronous upload, the frame read-out and the mesh stream needs it first
int32_t ensure_copy_stream(tsdf_ctx* c) { if (!c->copy_stream) HIP_TRY(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking)); return TSDF_OK; }
// Has the copy stream reached `e`?  wait: the host waits for it; otherwise it asks, and *reached = false while the result is still travelling ("not
// ready" is no error: it must not stay behind as the thread's last one)
int32_t event_reached(tsdf_ctx* c, hipEvent_t e, bool wait, bool* reached) {
  const hipError_t rc = wait ? hipEventSynchronize(e) : hipEventQuery(e);
  *reached = rc == hipSuccess;
  if (!wait && rc == hipErrorNotReady) { (void)hipGetLastError(); return TSDF_OK; }
  HIP_TRY(c, rc);
  return TSDF_OK;
}
// {bbox_min, extent} of the volume's box, as the ray queries and the texture taps map between world coordinates and the unit cube
void box_origin_extent(const tsdf_ctx* c, float lo[3], float ext[3]) { for (int a = 0; a < 3; ++a) { lo[a] = c->cfg.bbox_min[a]; ext[a] = c->cfg.bbox_max[a] - lo[a]; } }
// Grow the staging of a call's synchronous form to n elements (nothing queued reads it: every call that uses it synchronises): `in` and `out` by the one
// capacity, `extra` by its own when the call wants it; *_bytes per element
int32_t staging_reserve(tsdf_ctx* c, CallStaging& G, uint64_t n, bool want_extra, void** in, uint64_t in_bytes, void** out, uint64_t out_bytes, void** extra, uint64_t extra_bytes) {
  if (const uint64_t cap = G.grow(n)) {
    hipFree(*in); hipFree(*out); *in = nullptr; *out = nullptr; G.grown(0);
    HIP_TRY(c, hipMalloc(in, (size_t)(cap * in_bytes)));
    HIP_TRY(c, hipMalloc(out, (size_t)(cap * out_bytes)));
    G.grown(cap);
  }
  if (const uint64_t cap = G.grow_extra(n, want_extra)) {
    hipFree(*extra); *extra = nullptr; G.extra_grown(0);
    HIP_TRY(c, hipMalloc(extra, (size_t)(cap * extra_bytes)));
    G.extra_grown(cap);
  }
  return TSDF_OK;
}
void release_bricks(tsdf_ctx* c) {
  for (int k = 0; k < 2; ++k) { hipFree(c->d_counters[k]); hipFree(c->d_flags[k]); hipFree(c->d_occupied[k]); c->d_counters[k] = nullptr; c->d_flags[k] = nullptr; c->d_occupied[k] = nullptr; }
  c->br.counters = nullptr; c->br.flags = nullptr; c->br.num_occupied = nullptr; c->br.occupied = nullptr;
  hipFree(c->d_brick_tables); c->d_brick_tables = nullptr;
}

// resize(), recon_integration.cpp:482-500; the atlas: AtlasPlan (grid_plan.hpp)
int32_t setup_view(tsdf_ctx* c, uint32_t w, uint32_t h) {
  const AtlasPlan P = AtlasPlan::of(w, h);
  if (!P.ok) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "view size %ux%u out of range", w, h);
  release_view(c);
  c->vw = (int)w; c->vh = (int)h;
  Atlas& A = c->atlas;
  A.num_lods = P.num_lods; A.aw = P.aw; A.h = P.h;
  memcpy(A.off, P.off, sizeof(A.off)); memcpy(A.res, P.res, sizeof(A.res));
  const size_t na = (size_t)A.aw * A.h, nv = (size_t)w * h;
  HIP_TRY(c, hipMalloc(&A.color, na * sizeof(float4)));
  HIP_TRY(c, hipMalloc(&A.depth, na * sizeof(float)));
  c->atlas_color[0] = A.color; c->atlas_depth[0] = A.depth;                         // (pyramid 0 since release_view; the second one: on the first overlapped draw)
  HIP_TRY(c, hipMalloc(&c->d_peels, nv * sizeof(float4)));
  HIP_TRY(c, hipMalloc(&c->d_peels_alt, nv * sizeof(float4)));
  HIP_TRY(c, hipMalloc(&c->d_nsamples, nv * sizeof(float)));
  HIP_TRY(c, hipMalloc(&c->d_fb_c, nv * sizeof(float4)));
  HIP_TRY(c, hipMalloc(&c->d_fb_d, nv * sizeof(float)));
  HIP_TRY(c, hipMalloc(&c->d_hits, nv * 16));
  HIP_TRY(c, hipMalloc(&c->d_long, nv * sizeof(LongRay)));
  const size_t n_img_tiles = (size_t)((c->vw + 7) / 8) * ((c->vh + 7) / 8);
  for (int k = 0; k < 3; ++k) { HIP_TRY(c, hipMalloc(&c->d_touched[k], n_img_tiles)); HIP_TRY(c, hipMemsetAsync(c->d_touched[k], 0, n_img_tiles, c->stream)); }
  for (int k = 0; k < 2; ++k) { HIP_TRY(c, hipMalloc(&c->d_fill_mask[k], n_img_tiles)); HIP_TRY(c, hipMalloc(&c->d_lvl_mask[k], n_img_tiles)); }
  if (const char* e = getenv("RR_FILL_TILES")) c->tiles_img.fill_tiles = atoi(e) != 0;          // A/B and test hook
  HIP_TRY(c, hipMalloc(&c->d_hit_counters, 4 * sizeof(uint32_t)));
  HIP_TRY(c, hipMemsetAsync(c->d_hit_counters, 0, 4 * sizeof(uint32_t), c->stream));
  if (const char* e = getenv("RR_MARCH_CAP")) c->march_cap = (uint32_t)atoi(e);
  if (const char* e = getenv("RR_MARCH_BOX")) c->march_box = atoi(e);
  if (const char* e = getenv("RR_K1_FORM")) c->k1_form_cap = atoi(e);     // A/B and test hook, read when the context is created
  if (const char* e = getenv("RR_IMAGE_TILES")) c->tiles_img.use_history = atoi(e) != 0;
  c->hit_parity = 0;
  c->own_miss_counts = false;
  // the atlas starts as ViewLod::enable() leaves it (colour (0,1,0,0), depth 1); regions no kernel writes keep that
  launch_clear_image(c->stream, A.color, A.depth, na, make_float4(0.0f, 1.0f, 0.0f, 0.0f), 1.0f);
  launch_clear_image(c->stream, c->d_fb_c, c->d_fb_d, nv, make_float4(0, 0, 0, 0), 1.0f);
  HIP_TRY(c, hipMemsetAsync(c->d_peels, 0, nv * sizeof(float4), c->stream));
  HIP_TRY(c, hipMemsetAsync(c->d_peels_alt, 0, nv * sizeof(float4), c->stream));
  HIP_TRY(c, hipMemsetAsync(c->d_nsamples, 0, nv * sizeof(float), c->stream));
  return TSDF_OK;
}

// The brick grid: BrickPlan (grid_plan.hpp).  A refused plan's message, with nothing touched
int32_t refuse_bricks(tsdf_ctx* c, const BrickPlan& P, const float req[3]) {
  switch (P.error) {
    case BrickPlan::kNotPositive: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "brick size must be > 0");
    case BrickPlan::kRoundsToZero: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "brick size %g rounds to zero voxels", req[P.error_axis]);
    case BrickPlan::kTooManyBricks: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "more than 65535 bricks along one axis");
    case BrickPlan::kDegenerateOverlap: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "degenerate brick/voxel overlap on axis %d", P.error_axis);
    default: return TSDF_OK;
  }
}
// ... and an accepted one's: release, allocate and upload (the 21 tables as one blob), bind
int32_t build_bricks(tsdf_ctx* c, const BrickPlan& P, const float req[3]) {
  release_bricks(c);
  memcpy(c->brick_req, req, sizeof(float) * 3);
  Bricks& B = c->br;
  for (int a = 0; a < 3; ++a) { B.size[a] = P.size[a]; B.res[a] = P.res[a]; B.bbox_min[a] = c->cfg.bbox_min[a]; }
  B.n = P.n;
  const std::vector<uint8_t> blob = P.blob();
  HIP_TRY(c, hipMalloc(&c->d_brick_tables, blob.size()));
  HIP_TRY(c, hipMemcpy(c->d_brick_tables, blob.data(), blob.size(), hipMemcpyHostToDevice));
  for (int a = 0; a < 3; ++a) {
    auto u16 = [&](int t) { return (const uint16_t*)(c->d_brick_tables + P.offset(t, a)); };
    auto u8 = [&](int t) { return (const uint8_t*)(c->d_brick_tables + P.offset(t, a)); };
    B.vox_first[a] = u16(BrickPlan::kVoxFirst); B.vox_count[a] = u8(BrickPlan::kVoxCount);
    B.tile_b0[a] = u16(BrickPlan::kTileB0); B.tile_b1[a] = u16(BrickPlan::kTileB1); B.tile_full[a] = u8(BrickPlan::kTileFull);
    B.brick_t0[a] = u16(BrickPlan::kBrickT0); B.brick_t1[a] = u16(BrickPlan::kBrickT1);
  }
  for (tsdf_ctx::VolSet& s : c->vset) s.history.invalidate();            // a new brick grid: walk every tile once
  c->tiles.uniform = P.uniform ? 1 : 0;
  c->counter_words = P.counter_words;
  for (int k = 0; k < 2; ++k) {
    HIP_TRY(c, hipMalloc(&c->d_counters[k], c->counter_words * sizeof(uint32_t)));
    HIP_TRY(c, hipMemset(c->d_counters[k], 0, c->counter_words * sizeof(uint32_t)));
  }
  c->ahead.new_brick_grid();
  B.counters = c->d_counters[0];
  if (!c->d_occ_counts) HIP_TRY(c, hipMalloc(&c->d_occ_counts, 3 * sizeof(uint32_t)));
  HIP_TRY(c, hipMemset(c->d_occ_counts, 0, 3 * sizeof(uint32_t)));      // a new grid: no occupied list yet
  B.num_occupied = c->d_occ_counts + c->ahead.occ_set();
  for (int k = 0; k < 2; ++k) {
    HIP_TRY(c, hipMalloc(&c->d_flags[k], (size_t)B.n));
    HIP_TRY(c, hipMalloc(&c->d_occupied[k], (size_t)B.n * sizeof(uint32_t)));
    HIP_TRY(c, hipMemset(c->d_flags[k], 0, (size_t)B.n));
  }
  B.flags = c->d_flags[c->ahead.occ_set()]; B.occupied = c->d_occupied[c->ahead.occ_set()];
  // the fills above run on the NULL stream, asynchronously with respect to the host, and the context's streams are non-blocking: finished
  // before any of them touches the new tables
  HIP_TRY(c, hipDeviceSynchronize());
  return TSDF_OK;
}
int32_t setup_bricks(tsdf_ctx* c, const float req[3]) {
  const BrickPlan P = BrickPlan::of(c->cfg.bbox_min, c->cfg.bbox_max, c->res, c->vox, req);
  if (int32_t rc = refuse_bricks(c, P, req)) return rc;
  return build_bricks(c, P, req);
}

void timer_begin(tsdf_ctx* c, const char* name) {
  if (!c->timers_on) return;
  if (!c->timer_filter.empty() && c->timer_filter.find(std::string(",") + name + ",") == std::string::npos) return;
  Timer& t = c->timers[name];
  if (t.used == t.ev.size()) {
    if (t.ev.size() >= kMaxTimerPairs) { t.used = t.ev.size() - 1; }      // saturate: overwrite the last pair
    else { hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b); t.ev.emplace_back(a, b); }
  }
  hipEventRecord(t.ev[t.used].first, c->stream);
  t.open = true;
}
void timer_end(tsdf_ctx* c, const char* name) {
  if (!c->timers_on) return;
  auto it = c->timers.find(name);
  if (it == c->timers.end() || !it->second.open) return;
  Timer& t = it->second;
  hipEventRecord(t.ev[t.used].second, c->stream);
  t.used++;
  t.open = false;
}

void timer_begin_on(tsdf_ctx* c, const char* name, hipStream_t st) { hipStream_t keep = c->stream; c->stream = st; timer_begin(c, name); c->stream = keep; }
void timer_end_on(tsdf_ctx* c, const char* name, hipStream_t st) { hipStream_t keep = c->stream; c->stream = st; timer_end(c, name); c->stream = keep; }

// ---- the helper thread that issues the fill lane's calls (why: draw_lanes.hpp)
}  // namespace rrhost
struct tsdf_ctx::FillWorker {
  struct Job { Atlas atlas; const uint8_t* tile_mask; uint8_t* lvl_mask[2]; int vw, vh; float4* fb_c; float* fb_d; int mask_mode, keep; hipEvent_t wait_ev, done_ev; };
  static constexpr uint64_t kRing = 16;
  Job ring[kRing];
  std::atomic<uint64_t> submitted{0}, issued{0};
  std::atomic<bool> stop{false}, asleep{false};
  std::atomic<int> hip_error{0};
  std::mutex m; std::condition_variable cv;
  int device = 0; hipStream_t stream = nullptr;
  std::thread th;
  static void relax() { __builtin_ia32_pause(); }
  void run() {
    (void)hipSetDevice(device);
    uint64_t done = 0;
    for (;;) {
      int spins = 0;
      while (submitted.load(std::memory_order_acquire) == done) {
        if (stop.load()) return;
        if (++spins < 20000) { relax(); continue; }                       // ~1 ms of spinning, then sleep until the next job is announced
        std::unique_lock<std::mutex> lk(m);
        asleep.store(true);
        cv.wait_for(lk, std::chrono::milliseconds(10), [&] { return submitted.load() != done || stop.load(); });
        asleep.store(false);
        spins = 0;
      }
      const Job& j = ring[done % kRing];
      hipError_t e = hipStreamWaitEvent(stream, j.wait_ev, 0);
      rr::launch_inpaint_pyramid(stream, j.atlas, j.tile_mask, j.lvl_mask);
      rr::launch_colorfill(stream, j.atlas, j.vw, j.vh, j.fb_c, j.fb_d, j.mask_mode, j.keep, j.tile_mask);
      const hipError_t e2 = hipEventRecord(j.done_ev, stream), e3 = hipGetLastError();
      if (e == hipSuccess) e = e2 != hipSuccess ? e2 : e3;
      if (e != hipSuccess) hip_error.store((int)e);
      ++done;
      issued.store(done, std::memory_order_release);
    }
  }
  uint64_t submit(const Job& j) {
    const uint64_t n = submitted.load(std::memory_order_relaxed);
    while (n - issued.load(std::memory_order_acquire) >= kRing) relax();
    ring[n % kRing] = j;
    submitted.store(n + 1);
    if (asleep.load()) { { std::lock_guard<std::mutex> lk(m); } cv.notify_one(); }
    return n + 1;
  }
  void wait_issued(uint64_t n) const { while (issued.load(std::memory_order_acquire) < n) relax(); }
  void drain() const { wait_issued(submitted.load()); }
};
namespace rrhost {
static hipError_t fill_worker_error(tsdf_ctx* c) {
  if (!c->fill_worker) return hipSuccess;
  const int e = c->fill_worker->hip_error.exchange(0);
  return (hipError_t)e;
}
// stage overlap: GPU-side join (the context's stream waits for the hole filling that is still in flight) and host-side sync of both streams
static hipError_t wait_fill(tsdf_ctx* c, int pyramid, DrawLanes::FillJoin J) {
  if (!J.wait) return hipSuccess;
  if (c->fill_worker) { c->fill_worker->wait_issued(J.job); const hipError_t e = fill_worker_error(c); if (e != hipSuccess) return e; }   // (its record must have been issued before this wait is)
  return hipStreamWaitEvent(c->stream, c->fill_done[pyramid], 0);
}
hipError_t join_fill(tsdf_ctx* c) {
  const hipError_t a = wait_fill(c, 0, c->lanes.join_fill(0)), b = wait_fill(c, 1, c->lanes.join_fill(1));
  return a != hipSuccess ? a : b;
}
// record draw_done[set] on the context's stream, behind whatever last read the set (DrawLanes::draw_end)
static hipError_t record_draw_end(tsdf_ctx* c, DrawLanes::DrawEnd D) {
  if (c->fill_worker) c->fill_worker->wait_issued(D.wait_job);           // (a job that waits for the event's PREVIOUS record must have issued that wait)
  return hipEventRecord(c->draw_done[D.set], c->stream);
}
// the one doorway of whoever writes the framebuffer beside the hole filling (the point / triangle draws, the overlays, the texture views): wait for
// the hole filling in flight, and tell the tile history that the framebuffer is no longer the hole filling's alone (image_tiles.hpp)
static hipError_t begin_framebuffer_write(tsdf_ctx* c) {
  c->tiles_img.framebuffer_written();
  return join_fill(c);
}
// ---- the lane ahead: its state and protocol are lane_ahead.hpp's (tsdf_ctx::ahead); here the streams, the events and what is queued on them
bool pipelined(const tsdf_ctx* c) { return c->overlap_fill && !c->ahead.blocked(); }
inline int alt_of(int x) { return x ^ 1; }
bool deep_ok(const tsdf_ctx* c);
static void wait_gate(tsdf_ctx* c, int gate) { if (gate >= 0) hipStreamWaitEvent(c->pre_lane, c->pre_gate[gate], 0); }
hipStream_t pre_enter(tsdf_ctx* c, bool defer_gate) {
  if (!pipelined(c)) return c->stream;
  if (!c->pre_stream) {                                                   // (a context created with RR_OVERLAP_FILL=0 and switched on later)
    if (hipStreamCreateWithFlags(&c->pre_stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&c->pre_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->pre_gate[0], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->pre_gate[1], hipEventDisableTiming) != hipSuccess) { c->ahead.lane_unavailable(); return c->stream; }
  }
  if (c->ahead.at_frame_start()) {                                        // the lane's first call of a new frame
    // which stream: the lane ahead's own -- or, with the integrate lane in use, that one: a frame's preparation and its integrate() then
    // follow each other without a cross-stream hand-over (15-35 us each on this machine) at the price of not
    // overlapping the preparation of frame f + 2 with the integrate of frame f + 1
    c->pre_lane = (c->pre_on_integ && deep_ok(c)) ? c->integ_stream : c->pre_stream;
    // ... on the context's stream, which waits for an integrate() on the fourth lane only when a DRAW joins it.  Frames integrated back to back with no
    // draw in between leave that integrate out of every gate, while it may still read the frame slot / brick counters / occupancy set this frame is about to
    // overwrite (the copies alternate): the lane waits for the integrate lane itself then.  (In the per-frame order upload .. integrate, draw the flag is
    // clear here -- the draw has joined the lane -- and nothing is added.)
    const LaneAhead::Open O = c->ahead.open_frame(defer_gate, c->lanes.integ_in_flight() && c->integ_stream && c->pre_lane != c->integ_stream);
    wait_gate(c, O.overdue);
    wait_gate(c, O.wait);
    if (O.wait_integ) {
      hipEventRecord(c->integ_done, c->integ_stream);
      hipStreamWaitEvent(c->pre_lane, c->integ_done, 0);
    }
    hipEventRecord(c->pre_gate[O.record], c->stream);
  } else wait_gate(c, c->ahead.later_call(defer_gate));
  return c->pre_lane;
}
void pre_leave(tsdf_ctx* c, hipStream_t lane) { c->ahead.call_queued(lane != c->stream); }
// a consumer has been queued (LaneAhead::consume); the context's stream, and `also` if given, wait for what the lane holds.  false: it holds nothing
static bool consume_pre(tsdf_ctx* c, hipStream_t also, hipError_t* e) {
  *e = hipSuccess;
  if (!c->ahead.consume()) return false;
  *e = hipEventRecord(c->pre_done, c->pre_lane);
  if (*e == hipSuccess && also && also != c->pre_lane) *e = hipStreamWaitEvent(also, c->pre_done, 0);
  if (*e == hipSuccess) *e = hipStreamWaitEvent(c->stream, c->pre_done, 0);
  return true;
}
hipError_t join_pre(tsdf_ctx* c) {
  wait_gate(c, c->ahead.take_deferred_gate());
  hipError_t e;
  consume_pre(c, nullptr, &e);
  return e;
}
// leave the pipelined mode for good (explicit frame-slot calls, the pre-processing path): drain the lanes, everything on the context's stream from now on
hipError_t block_pipeline(tsdf_ctx* c) {
  if (!c->ahead.block()) return hipSuccess;
  hipError_t e = hipStreamSynchronize(c->stream);
  if (c->pre_stream) { const hipError_t f = hipStreamSynchronize(c->pre_stream); if (e == hipSuccess) e = f; }
  if (c->integ_stream) { const hipError_t f = hipStreamSynchronize(c->integ_stream); if (e == hipSuccess) e = f; c->lanes.integ_lane_drained(); }
  return e;
}
// ---- the fourth lane: its state and protocol are draw_lanes.hpp's (tsdf_ctx::lanes)
static hipError_t wait_integ(tsdf_ctx* c) {
  const hipError_t e = hipEventRecord(c->integ_done, c->integ_stream);
  return e != hipSuccess ? e : hipStreamWaitEvent(c->stream, c->integ_done, 0);
}
hipError_t join_integ(tsdf_ctx* c) { return c->lanes.join_integ() ? wait_integ(c) : hipSuccess; }
// the context holds every tile layer of the volume (false: a Z-slab)
static bool whole_volume(const tsdf_ctx* c) { return c->vol.own_tz0 == 0 && c->vol.own_tz1 == (c->res[2] + 7) / 8; }
bool deep_ok(const tsdf_ctx* c) {
  // (a Z-slab context too, when it recomputes its halo layers itself: an EXCHANGED halo is written into the volume from outside between integrate() and the draw)
  return c->deep && !c->lanes.second_set_failed() && pipelined(c) && c->integ_stream && (whole_volume(c) || c->cfg.slab_recompute_halo != 0) && !c->vol.slot && c->proj_budget == 0;
}
// ---- the volume sets: tsdf_ctx::vset; what an integrate() may trust of a set is volume_sets.hpp's (VolSet::history)
static tsdf_ctx::VolSet& set_in_use(tsdf_ctx* c) { return c->vset[c->lanes.set()]; }
// Set s as the kernels get it: its volume and classes into V, its stamps and the classes of the integrated tiles into S, with list / count 0 (a culled
// integrate() selects its own: TileHistory::begin).  Host pointers only: kernels already queued keep the pointers they were launched with
static void bind_volume_set(const tsdf_ctx::VolSet& s, Volume& V, TileState& S) {
  V.data = s.data; V.cls = s.cls;
  S.cls = s.cls + class_offset(V.tz0, V.int_tz0, V.nty, V.ntx); S.stamp = s.stamp;
  S.list = s.list[0]; S.count = s.counts;
}
static void free_volume_set(tsdf_ctx::VolSet& s) {
  hipFree(s.data); hipFree(s.cls); hipFree(s.stamp); hipFree(s.list[0]); hipFree(s.list[1]); hipFree(s.counts);
  s = tsdf_ctx::VolSet{};
}
// Allocate set s for the grid c->vol / c->tiles describe and initialise it on `lane`: the volume (the sparse pool where there is one) zeroed, every stored
// tile kTileMixed (halo layers keep this value for good), no tile stamped, both lists empty.  On failure nothing of the set is left
static hipError_t alloc_volume_set(tsdf_ctx* c, tsdf_ctx::VolSet& s, hipStream_t lane) {
  const Volume& V = c->vol;
  const size_t nvox = (V.slot ? (size_t)V.pool_tiles : (size_t)V.n_stored_tiles) * TILE_VOX, n = (size_t)c->tiles.n;
  hipError_t e = hipMalloc(&s.data, nvox * sizeof(float));
  if (e == hipSuccess) e = hipMalloc(&s.stamp, n * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc(&s.cls, (size_t)V.n_stored_tiles);
  for (int k = 0; k < 2 && e == hipSuccess; ++k) e = hipMalloc(&s.list[k], n * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc(&s.counts, 2 * sizeof(uint32_t));
  if (e != hipSuccess) { (void)hipGetLastError(); free_volume_set(s); return e; }
  launch_fill_u32(lane, (uint32_t*)s.data, 0u, nvox);
  hipMemsetAsync(s.cls, kTileMixed, (size_t)V.n_stored_tiles, lane);
  hipMemsetAsync(s.counts, 0, 2 * sizeof(uint32_t), lane);
  hipMemsetAsync(s.stamp, 0, n * sizeof(uint32_t), lane);
  s.history.reset();
  return hipSuccess;
}
// the other set, initialised on `lane` like setup_volume initialises the one in use; false = no memory for it (the context stays on one volume)
bool ensure_other_set(tsdf_ctx* c, hipStream_t lane) {
  tsdf_ctx::VolSet& s = c->vset[c->lanes.set() ^ 1];
  if (s.data) return true;
  if (alloc_volume_set(c, s, lane) != hipSuccess) { c->lanes.second_set_unavailable(); return false; }
  return true;
}
// projection cache: the pool and its tables, on the first integrate() that can use them, and this frame's turn of its slow-item counters.  Capacity = the
// budget, at most one slot per stored tile; a failed allocation (another context holds the memory) just leaves this context on the LUT path (*proj stays null)
static int32_t ensure_proj_cache(tsdf_ctx* c, const ProjCache** proj) {
  if (!c->proj.data) {
    int dz_max = 1;
    for (uint32_t i = 0; i < c->cfg.num_streams; ++i) dz_max = std::max(dz_max, c->lut_dz[i]);
    const size_t slot_bytes = (size_t)c->cfg.num_streams * dz_max * 64 * 3 * sizeof(float);
    const size_t cap = std::min<size_t>((size_t)c->vol.n_stored_tiles, c->proj_budget / slot_bytes);
    bool ok = cap > 0;
    ok = ok && hipMalloc((void**)&c->proj.slot, (size_t)c->vol.n_stored_tiles * sizeof(uint32_t)) == hipSuccess;
    ok = ok && hipMalloc((void**)&c->proj.items, (size_t)c->tiles.n * sizeof(uint32_t)) == hipSuccess;
    ok = ok && hipMalloc((void**)&c->d_proj_words, 4 * sizeof(uint32_t)) == hipSuccess;
    ok = ok && hipMalloc((void**)&c->proj.data, cap * slot_bytes) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      hipFree(c->proj.slot); hipFree(c->proj.items); hipFree(c->d_proj_words); hipFree(c->proj.data);
      c->proj = ProjCache{}; c->d_proj_words = nullptr; c->proj_failed = true;
      return TSDF_OK;
    }
    HIP_TRY(c, hipMemsetAsync(c->proj.slot, 0xff, (size_t)c->vol.n_stored_tiles * sizeof(uint32_t), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_proj_words, 0, 4 * sizeof(uint32_t), c->stream));
    c->proj.cap = (uint32_t)cap; c->proj.slot_floats = (uint32_t)(slot_bytes / sizeof(float)); c->proj.alloc = c->d_proj_words; c->proj.dz_max = (uint32_t)dz_max;
    c->proj_parity = 0;
  }
  for (uint32_t i = 0; i < c->cfg.num_streams; ++i) c->proj.inv_rz[i] = c->luts.s[i].inv_res[2];
  c->proj.n_slow = c->d_proj_words + 1 + c->proj_parity; c->proj.n_slow_next = c->d_proj_words + 1 + (c->proj_parity ^ 1);
  c->proj_parity ^= 1;
  *proj = &c->proj;
  return TSDF_OK;
}
hipError_t sync_ctx(tsdf_ctx* c) {
  hipError_t e = hipStreamSynchronize(c->stream);
  if (c->integ_stream) { const hipError_t f = hipStreamSynchronize(c->integ_stream); if (e == hipSuccess) e = f; }
  if (c->pre_stream) { const hipError_t f = hipStreamSynchronize(c->pre_stream); if (e == hipSuccess) e = f; c->ahead.lane_synchronised(); }
  if (c->fill_worker) { c->fill_worker->drain(); const hipError_t f = fill_worker_error(c); if (e == hipSuccess) e = f; }
  if (c->fill_stream) { const hipError_t f = hipStreamSynchronize(c->fill_stream); if (e == hipSuccess) e = f; }
  c->lanes.host_synchronised(c->integ_stream != nullptr);
  return e;
}

// draw() matrix block, recon_integration.cpp:182-205 (+ vol_to_world :66-72)
// The matrices alone (no context): shared by make_view_params and the host-only tsdf_view_matrices.
bool view_matrices(const float* bbox_min, const float* bbox_max, int vw, int vh, const float* mv16, const float* pr16, ViewParams* P, Mat4* v2w_out) {
  double mv[16], pr[16], v2w[16] = {0}, sc[16] = {0}, tr[16] = {0}, t0[16], t1[16];
  for (int i = 0; i < 16; ++i) { mv[i] = mv16[i]; pr[i] = pr16[i]; }
  for (int a = 0; a < 3; ++a) {
    v2w[a * 5] = (double)(bbox_max[a] - bbox_min[a]);    // float subtraction like :66-68
    v2w[12 + a] = bbox_min[a];
  }
  v2w[15] = 1.0;
  if (v2w_out) *v2w_out = to_mat4(v2w);
  memcpy(P->mv.m, mv16, 64); memcpy(P->proj.m, pr16, 64);
  if (!mat_inv_d(v2w, t0)) return false;
  P->v2w_inv = to_mat4(t0);
  double mvi[16];
  if (!mat_inv_d(mv, mvi)) return false;
  P->mv_inv = to_mat4(mvi);
  sc[0] = vw * 0.5; sc[5] = vh * 0.5; sc[10] = 0.5; sc[15] = 1.0;                        // :187-191
  tr[0] = tr[5] = tr[10] = tr[15] = 1.0; tr[12] = tr[13] = tr[14] = 1.0;                 // :184-186
  mat_mul_d(tr, pr, t0); mat_mul_d(sc, t0, t1);
  if (!mat_inv_d(t1, t0)) return false;
  P->img_to_eye = to_mat4(t0);                                                            // :192-194
  double m[16], mi[16], mit[16];
  mat_mul_d(mv, v2w, m);
  P->mv_v2w = to_mat4(m);
  if (!mat_inv_d(m, mi)) return false;
  for (int col = 0; col < 4; ++col) for (int r = 0; r < 4; ++r) mit[col * 4 + r] = mi[r * 4 + col];
  P->normal = to_mat4(mit);                                                               // :199
  double mvt[16];
  for (int col = 0; col < 4; ++col) for (int r = 0; r < 4; ++r) mvt[col * 4 + r] = mv[r * 4 + col];
  P->glnormal_inv = to_mat4(mvt);                    // inverse(inverseTranspose(MV)), shading.glsl:65
  // camera position: inverse(MV) * (0,0,0,1), then inverse(vol_to_world) * that, in fp32 on rounded matrices (:202-205)
  const Mat4& I = P->mv_inv;
  const float cw[4] = {I.m[12], I.m[13], I.m[14], I.m[15]};
  for (int a = 0; a < 3; ++a) P->cam_world[a] = cw[a];
  const Mat4& W = P->v2w_inv;
  for (int r = 0; r < 3; ++r) P->cam_vol[r] = W.m[r] * cw[0] + W.m[4 + r] * cw[1] + W.m[8 + r] * cw[2] + W.m[12 + r] * cw[3];
  return true;
}

bool make_view_params(const tsdf_ctx* c, const float* mv16, const float* pr16, ViewParams* P) {
  if (!view_matrices(c->cfg.bbox_min, c->cfg.bbox_max, c->vw, c->vh, mv16, pr16, P, nullptr)) return false;
  P->w = c->vw; P->h = c->vh;
  P->shade_mode = c->shade_mode;
  P->skip = (c->skip_space && c->use_bricks) ? 1 : 0;                                     // :154, :510-513
  // with hole filling the raymarch is rasterised into the pyramid's level-0 viewport (0, 0, w, h) (ViewLod::enable, view_lod.cpp:68):
  // gl_FragCoord then carries no window origin, while the shader still subtracts viewport_offset ("currently not working",
  // recon_integration.cpp:528-530; the client switches hole filling off for side-by-side stereo, kinect_client.cpp:645-647)
  for (int a = 0; a < 2; ++a) { P->vp_org[a] = c->fill_holes ? 0 : c->vp_org[a]; P->vp_off[a] = c->vp_off[a]; }
  return true;
}

// frame slots: device images of one frame {packed depth/quality/silhouette, depth plane, RGBA8 colour}
int32_t alloc_frame_slot(tsdf_ctx* c, int k) {
  tsdf_ctx::FrameSlot& S = c->slots[k];
  if (S.dqs) return TSDF_OK;
  const size_t np = (size_t)c->cfg.num_streams * c->cfg.depth_w * c->cfg.depth_h, nc = (size_t)c->cfg.num_streams * c->cfg.color_w * c->cfg.color_h;
  HIP_TRY(c, hipMalloc((void**)&S.dqs, np * sizeof(float4)));
  HIP_TRY(c, hipMalloc((void**)&S.depth, np * sizeof(float)));
  HIP_TRY(c, hipMalloc((void**)&S.color, nc * sizeof(uchar4)));
  HIP_TRY(c, hipMalloc((void**)&S.ranges, (size_t)c->cfg.num_streams * ((c->cfg.depth_w + 7) / 8) * ((c->cfg.depth_h + 7) / 8) * sizeof(float4)));
  // (finished before anything else touches the slot: it may be written on another lane right away, and hipMemset itself is asynchronous
  // with respect to the host and not ordered against non-blocking streams)
  HIP_TRY(c, hipMemsetAsync(S.color, 0, nc * sizeof(uchar4), c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipEventCreateWithFlags(&S.ready, hipEventDisableTiming));
  HIP_TRY(c, hipEventCreateWithFlags(&S.released, hipEventDisableTiming));
  return TSDF_OK;
}
void use_frame_slot(tsdf_ctx* c, int k) {
  c->intake.slots.made_current(k);
  c->frame.dqs = c->slots[k].dqs; c->frame.depth = c->slots[k].depth; c->frame.color = c->slots[k].color;
  c->frame.ranges = c->use_ranges ? c->slots[k].ranges : nullptr; c->frame.rcw = ((int)c->cfg.depth_w + 7) / 8; c->frame.rch = ((int)c->cfg.depth_h + 7) / 8;
}

// draw() without hole filling writes the default framebuffer through glColorMask (recon_integration.cpp:212-216): with a mask, or
// with a colour buffer the client did not clear, the march renders into the (otherwise unused) atlas and a merge pass follows
bool masked_direct(const tsdf_ctx* c) { return !c->fill_holes && (c->color_mask_mode != 0 || c->keep_color); }

RayTarget ray_target(tsdf_ctx* c) {
  RayTarget R{};
  if (masked_direct(c)) { R.color = c->atlas.color; R.depth = c->atlas.depth; R.stride = c->atlas.aw; R.clear[0] = R.clear[1] = R.clear[2] = R.clear[3] = 0; }
  else if (c->fill_holes) { R.color = c->atlas.color; R.depth = c->atlas.depth; R.stride = c->atlas.aw; R.clear[0] = 0; R.clear[1] = 1; R.clear[2] = 0; R.clear[3] = 0; }
  else { R.color = c->d_fb_c; R.depth = c->d_fb_d; R.stride = c->vw; R.clear[0] = R.clear[1] = R.clear[2] = R.clear[3] = 0; }
  R.nsamples = c->d_nsamples;
  R.peels = c->d_peels;
  return R;
}

// setVoxelSize()'s device side, recon_integration.cpp:340-348: the volume for the current c->res (tile-major storage, slot table of a
// sparse pool, per-tile state and work lists).  Called by tsdf_create and tsdf_set_voxel_size; everything it allocates is released first.
// the mesh form's texture taps belong to one extract (nothing queued reads them: tsdf_mesh_texture_taps synchronises)
void release_mesh_texture_taps(tsdf_ctx* c) {
  tsdf_ctx::TextureTaps& X = c->taps;
  hipFree(X.mesh_taps); hipFree(X.mesh_sensor);
  X.mesh_taps = nullptr; X.mesh_sensor = nullptr; X.mesh_nv = 0; X.mesh_valid = false; X.mesh_has_sensor = false;
}
// the labels and the table of a mesh (nothing queued reads them: tsdf_mesh_components, keep and filter synchronise); what a keep / filter removed stays on record
void release_mesh_components(tsdf_ctx* c) {
  tsdf_ctx::MeshComponents& K = c->mcomp;
  hipFree(K.vertex); hipFree(K.triangle); hipFree(K.table); hipFree(K.measure); hipFree(K.packed);
  K.vertex = nullptr; K.triangle = nullptr; K.table = nullptr; K.n = 0; K.largest = 0; K.valid = false;
  K.measure = nullptr; K.packed = nullptr; K.measured = false;
}
// The four arrays of a mesh (tsdf_ctx::MeshStore), for the whole mesh, a slab's part and a filtered mesh in the making.  Allocate: the arrays that `flags`
// names for nv vertices and nt triangles, each at least one element long (a part may own triangles and no vertex); false: out of memory, what was
// allocated stays in A for the caller's free.  The counts and flags are the caller's to set.
static bool mesh_store_allocate(MeshArrays& A, uint64_t nv, uint64_t nt, uint32_t flags) {
  const size_t v = std::max<size_t>((size_t)nv, 1), t = std::max<size_t>((size_t)nt, 1);
  bool ok = hipMalloc((void**)&A.pos, v * 3 * sizeof(float)) == hipSuccess && hipMalloc((void**)&A.tri, t * 3 * sizeof(uint32_t)) == hipSuccess;
  if (ok && (flags & TSDF_MESH_NORMALS)) ok = hipMalloc((void**)&A.nrm, v * 3 * sizeof(float)) == hipSuccess;
  if (ok && (flags & TSDF_MESH_COLOURS)) ok = hipMalloc((void**)&A.col, v * 4 * sizeof(float)) == hipSuccess;
  return ok;
}
static void mesh_store_free(MeshArrays& A) {
  hipFree(A.pos); hipFree(A.nrm); hipFree(A.col); hipFree(A.tri);
  A = MeshArrays{nullptr, nullptr, nullptr, nullptr};
}
static uint64_t mesh_store_bytes(const tsdf_ctx::MeshStore& M) {
  return M.nv * (3 + ((M.flags & TSDF_MESH_NORMALS) ? 3 : 0) + ((M.flags & TSDF_MESH_COLOURS) ? 4 : 0)) * sizeof(float) + M.nt * 3 * sizeof(uint32_t);
}
// into the caller's arrays, each of which may be null
static hipError_t mesh_store_download(const tsdf_ctx::MeshStore& M, float* position_xyz, float* normal_xyz, float* colour_rgba, uint32_t* triangles) {
  hipError_t e = hipSuccess;
  if (M.nv) {
    if (position_xyz) e = hipMemcpy(position_xyz, M.pos, (size_t)M.nv * 3 * sizeof(float), hipMemcpyDeviceToHost);
    if (!e && normal_xyz) e = hipMemcpy(normal_xyz, M.nrm, (size_t)M.nv * 3 * sizeof(float), hipMemcpyDeviceToHost);
    if (!e && colour_rgba) e = hipMemcpy(colour_rgba, M.col, (size_t)M.nv * 4 * sizeof(float), hipMemcpyDeviceToHost);
  }
  if (!e && M.nt && triangles) e = hipMemcpy(triangles, M.tri, (size_t)M.nt * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost);
  return e;
}
void release_mesh(tsdf_ctx* c) {
  mesh_store_free(c->mesh);
  c->mesh = tsdf_ctx::Mesh{};
  release_mesh_texture_taps(c);
  release_mesh_components(c);
  c->mcomp = tsdf_ctx::MeshComponents{};
}
// What the mesh launches need besides their output, per lattice tile of `level`: six arrays (the lattice-point records are sized by each caller: from the
// counts, or from the stream's capacity).  The first error, or hipSuccess with what the six take added to *bytes (may be null).
hipError_t mesh_scratch_allocate(MeshScratch& S, int n_tiles, int level, uint64_t* bytes) {
  const size_t n = (size_t)n_tiles;
  S.n_tiles = n_tiles; S.level = level;
  const struct { void** p; size_t bytes; } arrays[6] = {
    {(void**)&S.tile_cnt, n * sizeof(uint2)}, {(void**)&S.tile_skip, n}, {(void**)&S.tile_vbase, n * sizeof(uint32_t)}, {(void**)&S.tile_tbase, n * sizeof(unsigned long long)},
    {(void**)&S.tile_rec, n * sizeof(uint32_t)}, {(void**)&S.sums, (size_t)(mesh_scan_blocks(n_tiles) + 1) * 4 * sizeof(uint64_t)}};
  for (const auto& A : arrays) { if (const hipError_t e = hipMalloc(A.p, A.bytes)) return e; if (bytes) *bytes += A.bytes; }
  return hipSuccess;
}
void mesh_scratch_free(MeshScratch& S, uint32_t*& records) {            // ... and the records
  hipFree(S.tile_cnt); hipFree(S.tile_skip); hipFree(S.tile_vbase); hipFree(S.tile_tbase); hipFree(S.tile_rec); hipFree(S.sums); hipFree(records);
  S = MeshScratch{}; records = nullptr;
}
// the mesh ring's slots and scratch (nothing may be in flight: an idle ring, or behind a synchronisation of the streams); the configuration stays
void release_mesh_stream(tsdf_ctx* c) {
  tsdf_ctx::MeshStream& R = c->mstream;
  for (auto& S : R.slot) {
    if (S.dev) hipFree(S.dev - S.lead);
    if (S.host) hipHostFree(S.host - S.lead);
    for (hipEvent_t e : {S.header_written, S.emitted, S.header_ready, S.ready, S.taps_written}) if (e) hipEventDestroy(e);
    S = tsdf_ctx::MeshStreamSlot{};
  }
  mesh_scratch_free(R.scratch, R.records);
  MeshStreamFilter& F = R.filter;
  hipFree(F.raw); hipFree(F.parent); hipFree(F.label); hipFree(F.count); hipFree(F.keep); hipFree(F.vertex_sums); hipFree(F.triangle_sums); hipFree(F.words); hipFree(F.tri_local);
  F = MeshStreamFilter{};                                                // (raw_table lies inside raw's allocation)
  R.allocated = false; R.ring.reset(); R.device_bytes = 0;
}
// the components of a slab's linked part (nothing queued reads them: every entry that launches synchronises)
void release_mesh_slab_components(tsdf_ctx* c) {
  tsdf_ctx::MeshSlabComponents& K = c->mslabc;
  hipFree(K.label); hipFree(K.rank); hipFree(K.local); hipFree(K.down); hipFree(K.up); hipFree(K.roots); hipFree(K.vertex); hipFree(K.triangle); hipFree(K.table);
  K = tsdf_ctx::MeshSlabComponents{};
}
// a slab's part of the mesh and what its link needs (nothing queued reads them: extract, link and download synchronise)
void release_mesh_slab(tsdf_ctx* c) {
  release_mesh_slab_components(c);
  tsdf_ctx::MeshSlabPart& P = c->mslab;
  mesh_store_free(P); hipFree(P.above);
  mesh_scratch_free(P.scratch, P.records);
  P = tsdf_ctx::MeshSlabPart{};
}
void release_volume(tsdf_ctx* c) {
  release_mesh(c); c->have_volume = false;                             // (a mesh belongs to the grid it was extracted from)
  release_mesh_slab(c);
  release_mesh_stream(c);                                              // (... and the streaming scratch is sized by its tiles)
  for (tsdf_ctx::VolSet& s : c->vset) free_volume_set(s);              // (both callers have synchronised the stream)
  hipFree(c->vol.slot);
  hipFree(c->d_linear); hipFree(c->d_tile_bounds); hipFree(c->d_pair_masks); c->d_pair_masks = nullptr; hipFree(c->d_work_recs); c->d_work_recs = nullptr;
  hipFree(c->proj.data); hipFree(c->proj.slot); hipFree(c->proj.items); hipFree(c->d_proj_words); hipFree(c->d_item_stats);
  c->proj = ProjCache{}; c->d_proj_words = nullptr; c->d_item_stats = nullptr; c->proj_failed = false; c->last_integrate_cached = false;
  c->last_k1 = IntegratePlan{};
  c->lanes.volume_released();                                          // (the index of the set in use stays: setup_volume allocates that one)
  c->vol.data = nullptr; c->vol.slot = nullptr; c->tiles.stamp = nullptr; c->d_linear = nullptr; c->d_tile_bounds = nullptr;
  c->tile_bounds_valid = false;
}
// The tile layers of the context's slab in a volume of res voxels: SlabPlan (grid_plan.hpp); a refused plan's message, with nothing touched
SlabPlan plan_volume(const tsdf_ctx* c, const int res[3]) {
  const float limit = c->vol.limit > 0.0f ? c->vol.limit : c->cfg.limit;   // (re-created by setVoxelSize: keeps the current setTsdfLimit value)
  return SlabPlan::of(res, c->cfg.slab_z0, c->cfg.slab_z1, limit, c->cfg.slab_recompute_halo != 0, c->cfg.sparse_pool_tiles);
}
int32_t refuse_volume(tsdf_ctx* c, const SlabPlan& P) {
  switch (P.error) {
    case SlabPlan::kRange: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "slab range must be tile (8) aligned and inside the volume");
    case SlabPlan::kThinnerThanHalo: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "slab thinner than its halo");
    case SlabPlan::kStorageTiles: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "more than 2^31 storage tiles");
    case SlabPlan::kSparseNeedsRecompute: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "a sparse slab context needs slab_recompute_halo (exchanged halo layers have no pool slots)");
    case SlabPlan::kSparsePool: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "sparse_pool_tiles must be below 2^23 (16 GiB of tiles)");
    case SlabPlan::kVoxels: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "a context stores at most 2^32 voxels (32-bit tap offsets); split the volume into Z-slabs or use a sparse pool");
    default: return TSDF_OK;
  }
}
// ... and an accepted one's, for the voxel grid G it was made from: release, allocate, bind
int32_t build_volume(tsdf_ctx* c, const VoxelGrid& G, const SlabPlan& P) {
  int32_t rc;
  auto tryhip = [&](hipError_t e, const char* what) -> int32_t {
    if (e == hipSuccess) return TSDF_OK;
    c->err = std::string(what) + ": " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? TSDF_ERR_OUT_OF_MEMORY : TSDF_ERR_HIP;
  };
  release_volume(c);
  Volume& V = c->vol;
  for (int a = 0; a < 3; ++a) { c->res[a] = V.res[a] = G.res[a]; c->vox[a] = G.vox[a]; }
  V.ntx = P.ntx; V.nty = P.nty;
  V.div_layer = FastDiv{P.div_layer.m, P.div_layer.k}; V.div_row = FastDiv{P.div_row.m, P.div_row.k};
  if (!(V.limit > 0.0f)) V.limit = c->cfg.limit;
  V.own_tz0 = P.own_tz0; V.own_tz1 = P.own_tz1; V.tz0 = P.tz0; V.tz1 = P.tz1; V.int_tz0 = P.int_tz0; V.int_tz1 = P.int_tz1;
  V.zlo = P.zlo; V.zhi = P.zhi; V.n_stored_tiles = P.n_stored_tiles;
  c->halo_layers = P.halo_layers;
  V.slot = nullptr; V.pool_tiles = 0;
  if (P.pool_tiles) {
    if ((rc = tryhip(hipMalloc(&V.slot, (size_t)V.n_stored_tiles * sizeof(uint32_t)), "hipMalloc(slot table)"))) return rc;
    if ((rc = tryhip(hipMemsetAsync(V.slot, 0xff, (size_t)V.n_stored_tiles * sizeof(uint32_t), c->stream), "hipMemset(slot table)"))) return rc;
    V.pool_tiles = P.pool_tiles;
  }
  c->tiles.n = P.tiles_n;
  // the set in use -- either index: a released context keeps the one it was on --; the other one is the first integrate()'s on the lane (ensure_other_set)
  tsdf_ctx::VolSet& s = set_in_use(c);
  if ((rc = tryhip(alloc_volume_set(c, s, c->stream), "hipMalloc(volume set)"))) return rc;
  bind_volume_set(s, V, c->tiles);
  return TSDF_OK;
}
int32_t setup_volume(tsdf_ctx* c, const VoxelGrid& G) {
  const SlabPlan P = plan_volume(c, G.res);
  if (int32_t rc = refuse_volume(c, P)) return rc;
  return build_volume(c, G, P);
}
// which form of the integrate kernels stream i can use (depends on the LUT and on the volume resolution): LutFit (grid_plan.hpp)
void fit_lut_to_volume(tsdf_ctx* c, uint32_t i) {
  const LutFit F = LutFit::of(c->res, c->luts.s[i].inv_res, integrate_box_cap(), integrate_row_cap());
  c->lut_dz[i] = F.dz;
  c->lds_ok[i] = F.cls;
}

}  // namespace rrhost
using namespace rrhost;

extern "C" {

const char* tsdf_last_error(const tsdf_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int32_t tsdf_create(const tsdf_config* cfg, tsdf_ctx** out) {
  if (!cfg || !out) { g_create_error = "null argument"; return TSDF_ERR_INVALID_ARGUMENT; }
  *out = nullptr;
  // struct_size lets the struct grow: a caller built against the layout that ended at slab_recompute_halo is still accepted
  tsdf_config grown{};
  if (cfg->struct_size == offsetof(tsdf_config, sparse_pool_tiles) || cfg->struct_size == offsetof(tsdf_config, proj_cache_mib) || cfg->struct_size == offsetof(tsdf_config, lane_flags)) {
    memcpy(&grown, cfg, cfg->struct_size); grown.struct_size = sizeof(tsdf_config); cfg = &grown;
  }
  if (cfg->struct_size != sizeof(tsdf_config)) { g_create_error = "tsdf_config.struct_size mismatch"; return TSDF_ERR_INVALID_ARGUMENT; }
  if (cfg->num_streams < 1 || cfg->num_streams > TSDF_MAX_STREAMS) { g_create_error = "num_streams out of range"; return TSDF_ERR_INVALID_ARGUMENT; }
  if (!(cfg->limit > 0.0f)) { g_create_error = "limit must be > 0"; return TSDF_ERR_INVALID_ARGUMENT; }
  for (int a = 0; a < 3; ++a)
    if (!(cfg->bbox_max[a] > cfg->bbox_min[a])) { g_create_error = "empty bounding box"; return TSDF_ERR_INVALID_ARGUMENT; }
  if (cfg->depth_w < 1 || cfg->depth_h < 1 || cfg->color_w < 1 || cfg->color_h < 1) { g_create_error = "image size must be >= 1"; return TSDF_ERR_INVALID_ARGUMENT; }
  if (cfg->depth_w > 65536 || cfg->depth_h > 65536 || cfg->color_w > 65536 || cfg->color_h > 65536) { g_create_error = "image sides above 65536 are not supported"; return TSDF_ERR_INVALID_ARGUMENT; }
  if ((uint64_t)cfg->depth_w * cfg->depth_h * cfg->num_streams >= (1ull << 24) * 16 || (uint64_t)cfg->depth_w * cfg->depth_h >= (1ull << 24) ||
      (uint64_t)cfg->color_w * cfg->color_h >= (1ull << 24)) { g_create_error = "images of 2^24 pixels or more are not supported (24-bit index arithmetic)"; return TSDF_ERR_INVALID_ARGUMENT; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { g_create_error = "no HIP device visible (the HIP path has no CPU fallback)"; return TSDF_ERR_NO_DEVICE; }
  if (cfg->device < 0 || cfg->device >= ndev) { g_create_error = "device ordinal out of range"; return TSDF_ERR_INVALID_ARGUMENT; }
  tsdf_ctx* c = new tsdf_ctx();
  c->cfg = *cfg;
  c->device = cfg->device;
  auto fail = [&](int32_t code) { g_create_error = c->err; tsdf_destroy(c); return code; };
  if (hipSetDevice(c->device) != hipSuccess) { c->err = "hipSetDevice failed"; return fail(TSDF_ERR_HIP); }
  // RR_LANE_PRIORITY (A/B hook): "pre,fill,integ,main" stream priorities: -1 = high, 0 = normal, 1 = low
  // All normal by default.  The lane ahead BELOW the others ("1,0,0,0") is worth 4 % at c2 with one context (115 against 120 us per frame: its re-layout and
  // brick marking otherwise take the machine from the march) -- but a low-priority stream changes how the runtime deals its hardware queues: three contexts
  // in flight fall from 7 120 to 4 210 frames/s, and beside RCCL's kernels the lane starves (1 010 against 3 470 frames/s in the one-rank exchange rehearsal)
  int lo = 0, hi = 0, ppre = cfg->lane_priority[0], pfill = cfg->lane_priority[1], pinteg = cfg->lane_priority[2], pmain = cfg->lane_priority[3];
  hipDeviceGetStreamPriorityRange(&lo, &hi);                             // (least, greatest): numerically greatest <= least
  if (const char* e = getenv("RR_LANE_PRIORITY")) sscanf(e, "%d,%d,%d,%d", &ppre, &pfill, &pinteg, &pmain);
  auto prio = [&](int rel) { return rel < 0 ? hi : (rel > 0 ? lo : (lo + hi) / 2); };
  // (the context's own stream: created WITHOUT a priority unless the hook asks for one -- streams created through the priority call are dealt
  //  their hardware queues differently: several contexts' streams then share one, 4 250 instead of 7 080 frames/s with three contexts in flight)
  // Space sharing of the lanes (round 4): RR_LANE_XCDS = "pre,fill,integ,main", each a hex mask of the XCDs (bit x = XCD x) the lane's stream may run on
  // (0 / absent = all), or RR_LANE_CUS = "a-b,a-b,a-b,a-b": the CU slots [a, b] of EVERY XCD (0 - 31).  Bit i of a HIP CU mask is CU slot i / 8 of XCD i % 8
  // on this part (tools/probes/cumask_probe.hip).
  uint32_t lane_mask[4][8]; bool lane_masked[4] = {false, false, false, false};
  {
    unsigned xm[4] = {0, 0, 0, 0}; int lo4[4] = {0, 0, 0, 0}, hi4[4] = {31, 31, 31, 31};
    const char* ex = getenv("RR_LANE_XCDS"); const char* ec = getenv("RR_LANE_CUS");
    if (ex) sscanf(ex, "%x,%x,%x,%x", &xm[0], &xm[1], &xm[2], &xm[3]);
    if (ec) sscanf(ec, "%d-%d,%d-%d,%d-%d,%d-%d", &lo4[0], &hi4[0], &lo4[1], &hi4[1], &lo4[2], &hi4[2], &lo4[3], &hi4[3]);
    for (int l = 0; l < 4; ++l) {
      lane_masked[l] = (ex && (xm[l] & 0xffu) != 0u && (xm[l] & 0xffu) != 0xffu) || (ec && (lo4[l] > 0 || hi4[l] < 31));
      for (int k = 0; k < 8; ++k) lane_mask[l][k] = 0u;
      for (int i = 0; i < 256; ++i) {
        const int xcd = i & 7, cu = i >> 3;
        const bool on = (!ex || (xm[l] & 0xffu) == 0u || ((xm[l] >> xcd) & 1u)) && cu >= lo4[l] && cu <= hi4[l];
        if (on) lane_mask[l][i >> 5] |= 1u << (i & 31);
      }
    }
  }
  auto make_stream = [&](hipStream_t* st, int lane, int rel, bool with_priority) -> hipError_t {
    if (lane_masked[lane]) return hipExtStreamCreateWithCUMask(st, 8, lane_mask[lane]);
    return with_priority ? hipStreamCreateWithPriority(st, hipStreamNonBlocking, prio(rel)) : hipStreamCreateWithFlags(st, hipStreamNonBlocking);
  };
  if (make_stream(&c->own_stream, 3, pmain, pmain != 0) != hipSuccess) { c->err = "hipStreamCreate failed"; return fail(TSDF_ERR_HIP); }
  c->stream = c->own_stream;
  // The three lanes of a context (stage overlap) are created together: the HIP runtime deals its hardware queues (4 by default,
  // GPU_MAX_HW_QUEUES) to streams in creation order, and two lanes that share a queue do not overlap at all
  // tsdf_config::lane_flags decides; the RR_* variables of the A/B tools override it when set
  c->overlap_fill = !(cfg->lane_flags & TSDF_LANES_ONE_STREAM); c->deep = !(cfg->lane_flags & TSDF_LANES_NO_INTEGRATE_LANE); c->fill_thread = !(cfg->lane_flags & TSDF_LANES_NO_FILL_THREAD);
  if (const char* e = getenv("RR_OVERLAP_FILL")) c->overlap_fill = atoi(e) != 0;
  if (c->overlap_fill) {
    const bool two_lanes = getenv("RR_LANES") ? atoi(getenv("RR_LANES")) == 2 : (cfg->lane_flags & TSDF_LANES_SHARED_FILL_LANE) != 0;   // the lane ahead and the fill lane share one stream
    if (make_stream(&c->pre_stream, 0, ppre, true) != hipSuccess ||
        (two_lanes ? (c->fill_stream = c->pre_stream, hipSuccess) : make_stream(&c->fill_stream, 1, pfill, true)) != hipSuccess ||
        hipEventCreateWithFlags(&c->pre_done, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->pre_gate[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->pre_gate[1], hipEventDisableTiming) != hipSuccess ||
        make_stream(&c->integ_stream, 2, pinteg, true) != hipSuccess ||
        hipEventCreateWithFlags(&c->draw_done[0], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->draw_done[1], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->integ_done, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&c->integ_gate, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->fill_done[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->fill_done[1], hipEventDisableTiming) != hipSuccess) { c->err = "hipStreamCreate failed"; return fail(TSDF_ERR_HIP); }
  }
  if (const char* e = getenv("RR_K1_RANGES")) c->use_ranges = atoi(e) != 0;
  if (const char* e = getenv("RR_FILL_THREAD")) c->fill_thread = atoi(e) != 0;
  if (const char* e = getenv("RR_PRE_ON_INTEG")) c->pre_on_integ = atoi(e) != 0;
  if (const char* e = getenv("RR_DEEP")) c->deep = atoi(e) != 0;          // A/B and test hook: integrate() on the context's stream, one volume
  {
    uint64_t mib = cfg->proj_cache_mib;                                   // 0: off (the default: measured slower than the LUT kernel)
    if (mib == 0) if (const char* e = getenv("RR_PROJ_CACHE_MB")) mib = (uint64_t)atoll(e);   // A/B and test hook
    c->proj_budget = (size_t)(mib << 20);
  }
  if (const char* e = getenv("RR_K1_CULLED_RANGES")) c->culled_ranges = atoi(e) != 0;
  if (const char* e = getenv("RR_K1_REC")) c->use_recs = atoi(e) != 0;    // A/B hook: 0 = the LDS form's own tile head
  const VoxelGrid G = VoxelGrid::of(cfg->bbox_min, cfg->bbox_max, cfg->voxel_size, cfg->res);
  if (G.error == VoxelGrid::kVoxelSize) { c->err = "voxel_size must be > 0 when res is not given"; return fail(TSDF_ERR_INVALID_ARGUMENT); }
  if (G.error) { c->err = "volume resolution out of range [1, 4096]"; return fail(TSDF_ERR_INVALID_ARGUMENT); }
  int32_t rc;
  if ((rc = setup_volume(c, G))) return fail(rc);
  auto tryhip = [&](hipError_t e, const char* what) -> int32_t {
    if (e == hipSuccess) return TSDF_OK;
    c->err = std::string(what) + ": " + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? TSDF_ERR_OUT_OF_MEMORY : TSDF_ERR_HIP;
  };
  if ((rc = tryhip(hipHostMalloc((void**)&c->h_num_occupied, sizeof(uint32_t), hipHostMallocDefault), "hipHostMalloc"))) return fail(rc);
  *c->h_num_occupied = 0;
  if ((rc = tryhip(hipMalloc((void**)&c->taps.d_words, (size_t)kTapStatBytes), "hipMalloc(texture tap counters)"))) return fail(rc);   // (so that tsdf_texture_taps_dev allocates nothing)
  if ((rc = setup_bricks(c, cfg->brick_size))) return fail(rc);
  // frame images
  FrameImages& F = c->frame;
  F.w = (int)cfg->depth_w; F.h = (int)cfg->depth_h; F.cw = (int)cfg->color_w; F.ch = (int)cfg->color_h;
  const size_t np = (size_t)cfg->num_streams * F.w * F.h, nc = (size_t)cfg->num_streams * F.cw * F.ch;
  if ((rc = alloc_frame_slot(c, 0))) return fail(rc);
  use_frame_slot(c, 0);
  if ((rc = tryhip(hipMalloc(&c->d_stage_depth, np * 8), "hipMalloc(stage)"))) return fail(rc);
  if ((rc = tryhip(hipMalloc(&c->d_stage_q, np * 4), "hipMalloc(stage)"))) return fail(rc);
  if ((rc = tryhip(hipMalloc(&c->d_stage_s, np * 4), "hipMalloc(stage)"))) return fail(rc);
  if ((rc = tryhip(hipMalloc(&c->d_stage_col, nc * 3), "hipMalloc(stage)"))) return fail(rc);
  c->luts.n = (int)cfg->num_streams;
  c->pre.filter_textures = 1; c->pre.refine = 1;                      // NetKinectArray.cpp:63-69
  if ((rc = setup_view(c, cfg->view_w, cfg->view_h))) return fail(rc);
  if ((rc = tryhip(sync_ctx(c), "hipStreamSynchronize"))) return fail(rc);
  *out = c;
  return TSDF_OK;
}

int32_t tsdf_destroy(tsdf_ctx* c) {
  CHECK_CTX(c);
  hipSetDevice(c->device);
  sync_ctx(c);          // (a null handle is the NULL stream: tsdf_adopt_null_stream)
  if (c->copy_stream) hipStreamSynchronize(c->copy_stream);   // an asynchronous upload may still be writing a frame slot, a presented frame or a streamed mesh still travelling to its host buffer
  release_present(c);
  tsdf_comm_destroy(c);
  release_view(c); release_bricks(c);
  release_volume(c);
  for (auto& sl : c->slots) { hipFree(sl.dqs); hipFree(sl.depth); hipFree(sl.color); hipFree(sl.ranges); if (sl.ready) hipEventDestroy(sl.ready); if (sl.released) hipEventDestroy(sl.released); }
  for (int k = 0; k < 2; ++k) { if (c->h_stage[k]) hipHostFree(c->h_stage[k]); if (c->stage_done[k]) hipEventDestroy(c->stage_done[k]); }
  hipFree(c->d_astage);
  if (c->copy_stream) hipStreamDestroy(c->copy_stream);
  hipFree(c->d_raw); hipFree(c->d_depth2); hipFree(c->d_depth_rg); hipFree(c->d_lab); hipFree(c->d_depth_b); hipFree(c->d_normal); hipFree(c->d_pre_blocks);
  hipFree(c->d_stage_depth); hipFree(c->d_stage_q); hipFree(c->d_stage_s); hipFree(c->d_stage_col);
  for (auto& per : c->lut_alloc) for (void* p : per) hipFree(p);
  if (c->h_num_occupied) hipHostFree(c->h_num_occupied);
  hipFree(c->d_occ_counts);
  for (int k = 0; k < 2; ++k) { if (c->h_wire[k]) hipHostFree(c->h_wire[k]); if (c->wire_done[k]) hipEventDestroy(c->wire_done[k]); }
  hipFree(c->d_wire);
  for (auto& kv : c->timers) for (auto& e : kv.second.ev) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
  if (c->pre_stream && c->pre_stream != c->fill_stream) hipStreamDestroy(c->pre_stream);
  if (c->pre_done) hipEventDestroy(c->pre_done);
  for (hipEvent_t g : c->pre_gate) if (g) hipEventDestroy(g);
  if (c->src_ready) hipEventDestroy(c->src_ready);
  for (hipEvent_t e : c->read_fence) if (e) hipEventDestroy(e);
  hipFree(c->d_mvt_vtx); hipFree(c->d_calibvis_skipped);
  hipFree(c->rays.d_rays); hipFree(c->rays.d_hits); hipFree(c->rays.d_surf); hipFree(c->rays.d_list); hipFree(c->rays.d_words);
  hipFree(c->taps.d_xyz); hipFree(c->taps.d_taps); hipFree(c->taps.d_sensor); hipFree(c->taps.mesh_taps); hipFree(c->taps.mesh_sensor); hipFree(c->taps.d_words);
  if (c->fill_worker) {
    c->fill_worker->stop.store(true);
    { std::lock_guard<std::mutex> lk(c->fill_worker->m); }
    c->fill_worker->cv.notify_one();
    if (c->fill_worker->th.joinable()) c->fill_worker->th.join();
    delete c->fill_worker; c->fill_worker = nullptr;
  }
  if (c->fill_stream) hipStreamDestroy(c->fill_stream);
  if (c->integ_stream) hipStreamDestroy(c->integ_stream);
  for (hipEvent_t e : {c->integ_done, c->integ_gate, c->draw_done[0], c->draw_done[1]}) if (e) hipEventDestroy(e);
  for (hipEvent_t e : c->fill_done) if (e) hipEventDestroy(e);
  if (c->own_stream) hipStreamDestroy(c->own_stream);
  delete c;
  return TSDF_OK;
}

int32_t tsdf_sparse_pool_stats(tsdf_ctx* c, uint32_t* need, uint32_t* cap) {
  CHECK_CTX(c);
  if (!c->vol.slot) FAIL(c, TSDF_ERR_STATE, "not a sparse context");
  HIP_TRY(c, hipSetDevice(c->device));
  uint32_t n = 0;
  HIP_TRY(c, hipMemcpyAsync(&n, c->tiles.count, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, sync_ctx(c));
  if (need) *need = n;
  if (cap) *cap = c->vol.pool_tiles;
  return TSDF_OK;
}
int32_t tsdf_fill_stats(tsdf_ctx* c, uint64_t out[2]) {
  CHECK_CTX(c);
  if (!out) return TSDF_ERR_INVALID_ARGUMENT;
  out[0] = c->n_fills; out[1] = c->n_fills_by_tiles;
  return TSDF_OK;
}
int32_t tsdf_integrate_stats(tsdf_ctx* c, uint32_t out[6]) {
  CHECK_CTX(c);
  if (!out) return TSDF_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < 6; ++k) out[k] = 0;
  if (!c->last_integrate_cached || !c->proj.data) return TSDF_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->d_item_stats) HIP_TRY(c, hipMalloc((void**)&c->d_item_stats, 4 * sizeof(uint32_t)));
  TileState S = c->tiles;
  if (c->use_bricks) { const tsdf_ctx::VolSet& s = set_in_use(c); const int p = s.history.last(); S.list = s.list[p]; S.count = s.counts + p; }
  launch_item_stats(c->stream, c->luts, S, c->use_bricks ? 1 : 0, c->d_pair_masks, c->proj, c->d_item_stats);
  HIP_TRY(c, hipMemcpyAsync(out, c->d_item_stats, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(out + 4, c->proj.alloc, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, sync_ctx(c));
  out[4] = std::min(out[4], c->proj.cap); out[5] = c->proj.cap;
  return TSDF_OK;
}
int32_t tsdf_set_stream(tsdf_ctx* c, void* s) {
  CHECK_CTX(c);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_ctx(c));
  c->stream = s ? (hipStream_t)s : c->own_stream;
  return TSDF_OK;
}
// The process's NULL ("legacy default") stream has the handle 0, which tsdf_set_stream reads as "back to the context's own
// stream": adopting it needs an entry point of its own.  torch.cuda.default_stream().cuda_stream IS 0, so a caller that wants
// the context's kernels ordered with torch ops / RCCL collectives issued on torch's default stream must call this one.
int32_t tsdf_adopt_null_stream(tsdf_ctx* c) {
  CHECK_CTX(c);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_ctx(c));
  c->stream = nullptr;                         // hipStream_t 0: every launch / copy / event record below goes to the NULL stream
  return TSDF_OK;
}
int32_t tsdf_sync(tsdf_ctx* c) { CHECK_CTX(c); HIP_TRY(c, sync_ctx(c)); return TSDF_OK; }

int32_t tsdf_set_calibration(tsdf_ctx* c, uint32_t i, const float* inv, const uint32_t ri[3], const float* uv, const uint32_t ru[3], const float* xyz, const uint32_t rx[3]) {
  CHECK_CTX(c);
  if (i >= c->cfg.num_streams) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "stream %u out of range", i);
  if (!inv || !ri) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "cv_xyz_inv is required");
  HIP_TRY(c, hipSetDevice(c->device));
  StreamLut& L = c->luts.s[i];
  auto vol_n = [](const uint32_t r[3]) { return (size_t)r[0] * r[1] * r[2]; };
  // every LUT is indexed with 24-bit multiplies per axis and a 32-bit texel index in the kernels: the same bounds for all three
  auto check_res = [&](const uint32_t r[3], const char* what) -> int32_t {
    for (int a = 0; a < 3; ++a) if (r[a] < 1 || r[a] > 2048) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "%s resolution out of range [1, 2048]", what);
    if ((uint64_t)r[0] * r[1] * r[2] > (1ull << 31)) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "%s larger than 2^31 texels (the kernels index it with 32 bits)", what);
    return TSDF_OK;
  };
  if (int32_t rc = check_res(ri, "cv_xyz_inv")) return rc;
  if (uv) { if (!ru) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "cv_uv resolution missing"); if (int32_t rc = check_res(ru, "cv_uv")) return rc; }
  if (xyz) { if (!rx) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "cv_xyz resolution missing"); if (int32_t rc = check_res(rx, "cv_xyz")) return rc; }
  // re-calibration of a stream: queued kernels may still read the old volumes; wait, then free what this call replaces
  if (c->have_calib[i]) HIP_TRY(c, sync_ctx(c));
  auto replace = [&](int slot, void* fresh) { if (c->lut_alloc[i][slot]) hipFree(c->lut_alloc[i][slot]); c->lut_alloc[i][slot] = fresh; };
  // allocate, copy, and only then swap: a failed copy must leave the stream's old volume (and L.*) in place, never a freed pointer
  auto upload = [&](void** fresh, const void* src, size_t bytes) -> int32_t {
    *fresh = nullptr;
    HIP_TRY(c, hipMalloc(fresh, bytes));
    const hipError_t e = hipMemcpy(*fresh, src, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { hipFree(*fresh); *fresh = nullptr; FAIL(c, TSDF_ERR_HIP, "hipMemcpy(calibration volume) failed: %s", hipGetErrorString(e)); }
    return TSDF_OK;
  };
  void* fresh = nullptr;
  if (int32_t rc = upload(&fresh, inv, vol_n(ri) * sizeof(float4))) return rc;
  replace(0, fresh);
  L.inv = (const float4*)fresh; for (int a = 0; a < 3; ++a) L.inv_res[a] = (int)ri[a];
  fit_lut_to_volume(c, i);
  c->tile_bounds_valid = false;                                          // the tiles' LUT-box bounds and cached projections belong to the old volume
  if (c->proj.data) {                                                    // (the stream is idle: synchronised above) the pool's slot size follows the LUTs: re-made by the next integrate()
    hipFree(c->proj.data); hipFree(c->proj.slot); hipFree(c->proj.items); hipFree(c->d_proj_words);
    c->proj = ProjCache{}; c->d_proj_words = nullptr; c->last_integrate_cached = false;
  }
  c->proj_failed = false;
  if (uv) {
    if (int32_t rc = upload(&fresh, uv, vol_n(ru) * sizeof(float2))) return rc;
    replace(1, fresh);
    L.uv = (const float2*)fresh; for (int a = 0; a < 3; ++a) L.uv_res[a] = (int)ru[a];
  }
  if (xyz) {
    const size_t n = vol_n(rx);
    std::vector<float> padded(n * 4);
    for (size_t k = 0; k < n; ++k) { padded[4 * k] = xyz[3 * k]; padded[4 * k + 1] = xyz[3 * k + 1]; padded[4 * k + 2] = xyz[3 * k + 2]; padded[4 * k + 3] = 0.0f; }
    if (int32_t rc = upload(&fresh, padded.data(), n * sizeof(float4))) return rc;
    replace(2, fresh);
    L.xyz = (const float4*)fresh; for (int a = 0; a < 3; ++a) L.xyz_res[a] = (int)rx[a];
    // CalibVolumes::addVolume builds the sensor's frustum from this volume (CalibVolumes.cpp:122) and getCameraPositions()
    // (:224-230) feeds the quality pass: default camera position, until tsdf_set_camera_position overrides it
    float cam[3];
    if (tsdf_frustum_from_volume(xyz, rx, nullptr, cam) == TSDF_OK) {
      if (std::isfinite(cam[0]) && std::isfinite(cam[1]) && std::isfinite(cam[2])) {
        for (int a = 0; a < 3; ++a) c->pre.cam[i][a] = cam[a];
        c->have_cam[i] = true;
      }
      // ... and draws it (CalibVolumes::drawFrustums, :214-218): the corner samples and the camera position of the frustum overlay
      frustum_corners(xyz, rx, c->frustum_corner[i]);
      for (int a = 0; a < 3; ++a) c->frustum_cam[i][a] = cam[a];
      c->have_frustum[i] = true;
    }
  }
  c->have_calib[i] = true;
  return TSDF_OK;
}

// ---- the frame intake (frame_intake.hpp)
static tsdf_ctx::FrameSlot& current_slot(tsdf_ctx* c) { return c->slots[c->intake.slots.current()]; }
static const float* raw_depth(const tsdf_ctx* c) { return c->intake.raw.read_from() == kRawOwn ? c->d_raw : c->raw_src; }
// a reader of a single-buffered image was queued on the context's stream: record fence f behind it
static int32_t record_read_fence(tsdf_ctx* c, int f) {
  c->intake.fences.reader_queued(f);
  if (!c->read_fence[f]) HIP_TRY(c, hipEventCreateWithFlags(&c->read_fence[f], hipEventDisableTiming));
  HIP_TRY(c, hipEventRecord(c->read_fence[f], c->stream));
  return TSDF_OK;
}
// ... and the lane that rewrites the image waits for it
static int32_t wait_read_fence(tsdf_ctx* c, int f, hipStream_t lane) {
  if (c->intake.fences.writer_takes(f, lane != c->stream)) HIP_TRY(c, hipStreamWaitEvent(lane, c->read_fence[f], 0));
  return TSDF_OK;
}
// the producer of a frame's device arrays may be work on the context's stream: the lane goes behind all of it
static int32_t wait_for_producer(tsdf_ctx* c, hipStream_t lane) {
  if (!c->src_ready) HIP_TRY(c, hipEventCreateWithFlags(&c->src_ready, hipEventDisableTiming));
  HIP_TRY(c, hipEventRecord(c->src_ready, c->stream));
  HIP_TRY(c, hipStreamWaitEvent(lane, c->src_ready, 0));
  return TSDF_OK;
}
// On the lane ahead the re-layout launch of a new frame also clears the brick counters the frame's clearOccupiedBricks() is going to use
// (it flips to them here instead): one launch and one dependent step less on the lane.
static uint32_t* counters_for_upload(tsdf_ctx* c, hipStream_t lane) {
  const int k = c->ahead.counters_for_upload(lane != c->stream && c->d_counters[0]);
  if (k < 0) return nullptr;
  return c->br.counters = c->d_counters[k];
}
// The frame slot a new frame is written to.  On the lane ahead: the OTHER slot (the context's stream may still read the current one for
// the previous frame), once per frame of the lane; c->frame then points at it, so everything queued from now on reads the new frame.
static int32_t begin_slot_write(tsdf_ctx* c, hipStream_t lane, bool keep_colour) {
  if (!c->ahead.slot_for_write(lane != c->stream)) return TSDF_OK;      // (nothing queued reads the current slot -- the first frame --: in place)
  const int old = c->intake.slots.current(), t = alt_of(old);
  if (int32_t rc = alloc_frame_slot(c, t)) return rc;
  if (keep_colour) {                                                     // "colour may be NULL (keeps the previous one)": the previous one lives in the other slot
    const size_t nc = (size_t)c->cfg.num_streams * c->frame.cw * c->frame.ch;
    HIP_TRY(c, hipMemcpyAsync(c->slots[t].color, c->slots[old].color, nc * sizeof(uchar4), hipMemcpyDeviceToDevice, lane));
  }
  use_frame_slot(c, t);
  return TSDF_OK;
}
int32_t tsdf_upload_frame(tsdf_ctx* c, const float* depth_rg, const float* quality, const float* silhouette, const uint8_t* colour) {
  CHECK_CTX(c);
  if (!depth_rg || !quality || !silhouette) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "depth, quality and silhouette are required");
  HIP_TRY(c, hipSetDevice(c->device));
  const hipStream_t lane = pre_enter(c);
  if (int32_t rc = begin_slot_write(c, lane, colour == nullptr)) return rc;
  const FrameImages& F = c->frame;
  const size_t np = (size_t)c->cfg.num_streams * F.w * F.h, nc = (size_t)c->cfg.num_streams * F.cw * F.ch;
  HIP_TRY(c, hipMemcpyAsync(c->d_stage_depth, depth_rg, np * 8, hipMemcpyHostToDevice, lane));
  HIP_TRY(c, hipMemcpyAsync(c->d_stage_q, quality, np * 4, hipMemcpyHostToDevice, lane));
  HIP_TRY(c, hipMemcpyAsync(c->d_stage_s, silhouette, np * 4, hipMemcpyHostToDevice, lane));
  if (colour) HIP_TRY(c, hipMemcpyAsync(c->d_stage_col, colour, nc * 3, hipMemcpyHostToDevice, lane));
  launch_pack_frame_fused(lane, c->d_stage_depth, c->d_stage_q, c->d_stage_s, (float4*)F.dqs, (float*)c->frame.depth, current_slot(c).ranges,
                          (int)c->cfg.num_streams, F.w, F.h, colour ? c->d_stage_col : nullptr, (uchar4*)F.color, nc, counters_for_upload(c, lane), (uint32_t)c->counter_words);
  HIP_TRY(c, hipGetLastError());
  c->intake.slots.preprocessed_written();
  pre_leave(c, lane);
  return TSDF_OK;
}
// The same with the four arrays already in device memory (a producer on the GPU: the pre-processing of another library, a decoder, a
// staging buffer the caller DMA'd himself): no copy, one re-layout launch into a frame slot.  This is what a NEW frame costs the path
// itself (NetKinectArray hands integrate() a new frame every time, kinect_client.cpp:586-599).
//   flags 0                      the arrays were (or are being) written by work queued on the context's stream: the re-layout is ordered behind it
//   TSDF_FRAME_ARRAYS_COMPLETE   the arrays are complete now: the re-layout starts at once on the lane ahead, beside the previous frame's kernels
// Either way the arrays must stay untouched until work queued on the context's stream AFTER the next tsdf_integrate() / draw call runs.
int32_t tsdf_upload_frame_dev(tsdf_ctx* c, const float* depth_rg, const float* quality, const float* silhouette, const uint8_t* colour, uint32_t flags) {
  CHECK_CTX(c);
  if (!depth_rg || !quality || !silhouette) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "depth, quality and silhouette are required");
  if (((uintptr_t)depth_rg & 7u) || ((uintptr_t)quality & 3u) || ((uintptr_t)silhouette & 3u) || ((uintptr_t)colour & 3u))
    FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "device arrays must be aligned to their element size (depth 8 bytes, the others 4)");
  HIP_TRY(c, hipSetDevice(c->device));
  const hipStream_t lane = pre_enter(c);
  if (lane != c->stream && !(flags & TSDF_FRAME_ARRAYS_COMPLETE)) { if (int32_t rc = wait_for_producer(c, lane)) return rc; }
  if (int32_t rc = begin_slot_write(c, lane, colour == nullptr)) return rc;
  const FrameImages& F = c->frame;
  const size_t nc = (size_t)c->cfg.num_streams * F.cw * F.ch;
  timer_begin_on(c, "0repack", lane);
  launch_pack_frame_fused(lane, depth_rg, quality, silhouette, (float4*)F.dqs, (float*)c->frame.depth, current_slot(c).ranges,
                          (int)c->cfg.num_streams, F.w, F.h, colour, (uchar4*)F.color, nc, counters_for_upload(c, lane), (uint32_t)c->counter_words);
  timer_end_on(c, "0repack", lane);
  HIP_TRY(c, hipGetLastError());
  c->intake.slots.preprocessed_written();
  pre_leave(c, lane);
  return TSDF_OK;
}

// ---- asynchronous frame upload: NetKinectArray's double PBO (framework/double_pixel_buffer.cpp:18-81; readLoop's memcpy into the
// mapped back buffer NetKinectArray.cpp:516-520; update() = swap + PBO -> texture DMA, :225-236) as two device frame slots, a pinned
// host staging ring and a copy stream.  While the path computes on the current slot the next frame travels into the other one.
static int32_t ensure_async_upload(tsdf_ctx* c) {
  if (c->async_upload_ready) return TSDF_OK;
  const size_t np = (size_t)c->cfg.num_streams * c->frame.w * c->frame.h, nc = (size_t)c->cfg.num_streams * c->frame.cw * c->frame.ch;
  const size_t bytes = np * 16 + nc * 3;
  for (int k = 0; k < 2; ++k) {                                            // (re-entered after a failed first attempt: keep what exists)
    if (!c->h_stage[k]) HIP_TRY(c, hipHostMalloc((void**)&c->h_stage[k], bytes, hipHostMallocDefault));
    if (!c->stage_done[k]) HIP_TRY(c, hipEventCreateWithFlags(&c->stage_done[k], hipEventDisableTiming));
  }
  if (!c->d_astage) HIP_TRY(c, hipMalloc((void**)&c->d_astage, bytes));
  if (int32_t rc = alloc_frame_slot(c, 0)) return rc;
  if (int32_t rc = alloc_frame_slot(c, 1)) return rc;
  HIP_TRY(c, sync_ctx(c));                             // the new slot's colour memset
  if (int32_t rc = ensure_copy_stream(c)) return rc;   // (the frame read-out may have made it already)
  c->async_upload_ready = true;
  return TSDF_OK;
}
int32_t tsdf_frame_staging(tsdf_ctx* c, float** depth_rg, float** quality, float** silhouette, uint8_t** colour) {
  CHECK_CTX(c);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, block_pipeline(c));                                          // the caller manages the two frame slots himself from here on
  if (int32_t rc = ensure_async_upload(c)) return rc;
  const FrameSlots::Staging G = c->intake.slots.staging();
  if (G.wait) HIP_TRY(c, hipEventSynchronize(c->stage_done[G.index]));   // its last upload has left the buffer
  const size_t np = (size_t)c->cfg.num_streams * c->frame.w * c->frame.h;
  uint8_t* b = c->h_stage[G.index];
  if (depth_rg) *depth_rg = (float*)b;
  if (quality) *quality = (float*)(b + np * 8);
  if (silhouette) *silhouette = (float*)(b + np * 12);
  if (colour) *colour = b + np * 16;
  return TSDF_OK;
}
int32_t tsdf_upload_frame_async(tsdf_ctx* c, const float* depth_rg, const float* quality, const float* silhouette, const uint8_t* colour, int32_t with_colour) {
  CHECK_CTX(c);
  HIP_TRY(c, hipSetDevice(c->device));
  float *sd, *sq, *ss; uint8_t* sc;
  if (int32_t rc = tsdf_frame_staging(c, &sd, &sq, &ss, &sc)) return rc;   // (waits for the staging buffer)
  const size_t np = (size_t)c->cfg.num_streams * c->frame.w * c->frame.h, nc = (size_t)c->cfg.num_streams * c->frame.cw * c->frame.ch;
  // NULL (or the staging pointer itself): the producer wrote the staging buffer in place, as readLoop() writes the mapped PBO
  if (depth_rg && depth_rg != sd) memcpy(sd, depth_rg, np * 8);
  if (quality && quality != sq) memcpy(sq, quality, np * 4);
  if (silhouette && silhouette != ss) memcpy(ss, silhouette, np * 4);
  if (colour && colour != sc) { memcpy(sc, colour, nc * 3); with_colour = 1; }
  const FrameSlots::Async A = c->intake.slots.async_queued();
  const int k = A.staging;
  tsdf_ctx::FrameSlot& S = c->slots[A.slot];
  if (A.wait_released) HIP_TRY(c, hipStreamWaitEvent(c->copy_stream, S.released, 0));   // the path's reads of the slot were all queued before `released`
  const size_t bytes = np * 16 + (with_colour ? nc * 3 : 0);
  HIP_TRY(c, hipMemcpyAsync(c->d_astage, c->h_stage[k], bytes, hipMemcpyHostToDevice, c->copy_stream));
  HIP_TRY(c, hipEventRecord(c->stage_done[k], c->copy_stream));
  launch_pack_frame_fused(c->copy_stream, (const float*)c->d_astage, (const float*)(c->d_astage + np * 8), (const float*)(c->d_astage + np * 12), S.dqs, S.depth, S.ranges,
                          (int)c->cfg.num_streams, c->frame.w, c->frame.h, with_colour ? c->d_astage + np * 16 : nullptr, S.color, nc);
  HIP_TRY(c, hipEventRecord(S.ready, c->copy_stream));
  HIP_TRY(c, hipGetLastError());
  return TSDF_OK;
}
int32_t tsdf_select_frame_slot(tsdf_ctx* c, uint32_t slot) {
  CHECK_CTX(c);
  if (slot > 1) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "frame slot must be 0 or 1");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, block_pipeline(c));                                          // the caller manages the two frame slots himself from here on
  if (int32_t rc = alloc_frame_slot(c, (int)slot)) return rc;
  tsdf_ctx::FrameSlot& O = current_slot(c);
  const FrameSlots::Select T = c->intake.slots.select((int)slot, O.released != nullptr);
  if (T.record_released) HIP_TRY(c, hipEventRecord(O.released, c->stream));
  if (T.wait_ready) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->slots[slot].ready, 0));   // the path waits on the GPU, not on the host
  use_frame_slot(c, (int)slot);
  return TSDF_OK;
}
int32_t tsdf_current_frame_slot(const tsdf_ctx* c, uint32_t* slot) { CHECK_CTX(c); if (!slot) return TSDF_ERR_INVALID_ARGUMENT; *slot = (uint32_t)c->intake.slots.current(); return TSDF_OK; }

// ---- image pre-processing (NetKinectArray::processTextures)
static int32_t ensure_pre_buffers(tsdf_ctx* c) {
  const FrameImages& F = c->frame;
  const size_t np = (size_t)c->cfg.num_streams * F.w * F.h;
  if (!c->d_raw) {
    HIP_TRY(c, hipMalloc(&c->d_raw, np * sizeof(float)));
    HIP_TRY(c, hipMalloc(&c->d_depth2, np * sizeof(float)));
    HIP_TRY(c, hipMalloc(&c->d_depth_rg, np * sizeof(float2)));
    HIP_TRY(c, hipMalloc(&c->d_lab, np * sizeof(float4)));
    HIP_TRY(c, hipMalloc(&c->d_depth_b, np * sizeof(float2)));
    HIP_TRY(c, hipMalloc(&c->d_normal, np * sizeof(float4)));
    const size_t blocks = (size_t)c->cfg.num_streams * ((F.w + 15) / 16) * ((F.h + 15) / 16);
    c->pre_cand_cap = (uint32_t)std::min<size_t>(blocks, 1024);
    if (const char* e = getenv("RR_TEST_PRE_CAND_CAP")) c->pre_cand_cap = (uint32_t)std::min<size_t>(blocks, (size_t)std::max(1, atoi(e)));   // test hook: a short list, so that candidate blocks overflow it
    HIP_TRY(c, hipMalloc(&c->d_pre_blocks, (1 + c->pre_cand_cap + blocks) * sizeof(uint32_t)));
    HIP_TRY(c, hipMemset(c->d_pre_blocks, 0, (1 + c->pre_cand_cap + blocks) * sizeof(uint32_t)));
  }
  return TSDF_OK;
}
// The raw frame (NetKinectArray::update(): depth + colour of every sensor) goes through the lane ahead like a pre-processed one does (round 4): its
// colour is re-laid out into the frame slot the lane writes, its depth is what tsdf_process_textures() -- on the same lane -- starts from.
int32_t tsdf_upload_raw_frame(tsdf_ctx* c, const float* depth_raw, const uint8_t* colour) {
  CHECK_CTX(c);
  if (!depth_raw || !colour) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "raw depth and colour are required");
  HIP_TRY(c, hipSetDevice(c->device));
  if (int32_t rc = ensure_pre_buffers(c)) return rc;
  const hipStream_t lane = pre_enter(c);
  if (int32_t rc = begin_slot_write(c, lane, false)) return rc;
  if (int32_t rc = wait_read_fence(c, kRawRead, lane)) return rc;   // an MVT draw (or a Lab window) still queued on the context's stream reads d_raw
  const FrameImages& F = c->frame;
  const size_t np = (size_t)c->cfg.num_streams * F.w * F.h, nc = (size_t)c->cfg.num_streams * F.cw * F.ch;
  HIP_TRY(c, hipMemcpyAsync(c->d_raw, depth_raw, np * sizeof(float), hipMemcpyHostToDevice, lane));
  HIP_TRY(c, hipMemcpyAsync(c->d_stage_col, colour, nc * 3, hipMemcpyHostToDevice, lane));
  c->pending_rgb = c->d_stage_col;                                       // its RGBA8 re-layout rides along in tsdf_process_textures' first launch
  c->intake.raw.uploaded(kRawOwn, true); c->intake.slots.raw_arrived();
  pre_leave(c, lane);
  return TSDF_OK;
}
// ... and with both arrays in device memory already (a decoder, a camera SDK's buffer): no copy -- the passes read depth_raw where it lies.  flags as
// for tsdf_upload_frame_dev; the arrays must stay untouched until work queued on the context's stream AFTER the next tsdf_integrate() / draw call runs.
static int32_t upload_raw_frame_dev_impl(tsdf_ctx* c, const float* depth_raw, const uint8_t* colour, uint32_t flags, bool defer_gate) {
  CHECK_CTX(c);
  if (!depth_raw || !colour) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "raw depth and colour are required");
  if (((uintptr_t)depth_raw & 3u) || ((uintptr_t)colour & 3u)) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "device arrays must be 4-byte aligned");
  HIP_TRY(c, hipSetDevice(c->device));
  if (int32_t rc = ensure_pre_buffers(c)) return rc;
  const hipStream_t lane = pre_enter(c, defer_gate);                      // (nothing below writes what the previous frames' draws read: flips of host pointers, a wait for the producer)
  if (lane != c->stream && !(flags & TSDF_FRAME_ARRAYS_COMPLETE)) { if (int32_t rc = wait_for_producer(c, lane)) return rc; }
  if (int32_t rc = begin_slot_write(c, lane, false)) return rc;
  c->pending_rgb = colour;                                               // its RGBA8 re-layout rides along in tsdf_process_textures' first launch
  c->raw_src = depth_raw; c->intake.raw.uploaded(kRawCaller, true); c->intake.slots.raw_arrived();
  pre_leave(c, lane);
  return TSDF_OK;
}
int32_t tsdf_upload_raw_frame_dev(tsdf_ctx* c, const float* depth_raw, const uint8_t* colour, uint32_t flags) { return upload_raw_frame_dev_impl(c, depth_raw, colour, flags, false); }
int32_t tsdf_set_depth_limits(tsdf_ctx* c, uint32_t i, float mn, float mx) {
  CHECK_CTX(c);
  if (i >= c->cfg.num_streams || !(mx > mn)) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "bad stream index or depth limits");
  c->pre.cv_min[i] = mn; c->pre.cv_max[i] = mx; c->have_limits[i] = true;
  return TSDF_OK;
}
int32_t tsdf_set_camera_position(tsdf_ctx* c, uint32_t i, const float xyz[3]) {
  CHECK_CTX(c);
  if (i >= c->cfg.num_streams || !xyz) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "bad stream index");
  for (int a = 0; a < 3; ++a) c->pre.cam[i][a] = xyz[a];
  c->have_cam[i] = true;
  return TSDF_OK;
}

// ---- frame ingest (NetKinectArray::init sizes :118-139, readLoop :482-529, update :225-236)
static void wire_sizes(const tsdf_ctx* c, uint32_t cf, uint32_t df, uint64_t* cs, uint64_t* ds) {
  const uint64_t cp = (uint64_t)c->frame.cw * c->frame.ch, dp = (uint64_t)c->frame.w * c->frame.h;
  *cs = cf == TSDF_COLOR_DXT1 ? cp * 4 / 8 : (cf == TSDF_COLOR_DXT5 ? cp : cp * 3);     // :118-130 (DXT5: the literal 307200 = 640*480)
  *ds = df == TSDF_DEPTH_U8 ? dp : dp * 4;                                               // :134-141
}
int32_t tsdf_set_wire_format(tsdf_ctx* c, uint32_t color_format, uint32_t depth_format) {
  CHECK_CTX(c);
  if (color_format != TSDF_COLOR_RGB8 && color_format != TSDF_COLOR_DXT1 && color_format != TSDF_COLOR_DXT5) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "colour format must be 0 (RGB8), 1 (DXT1) or 5 (DXT5)");
  if (depth_format != TSDF_DEPTH_F32 && depth_format != TSDF_DEPTH_U8) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "depth format must be 0 (float32) or 1 (8 bit)");
  uint64_t cs, ds;
  wire_sizes(c, color_format, depth_format, &cs, &ds);
  if ((cs & 15) || (ds & 15)) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "image sizes give records that are not 16-byte multiples (colour %llu, depth %llu bytes)", (unsigned long long)cs, (unsigned long long)ds);
  if (color_format != TSDF_COLOR_RGB8 && ((c->frame.cw | c->frame.ch) & 3)) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "DXT colour needs a resolution that is a multiple of 4 (the wire size w*h/2 assumes it)");
  c->color_format = color_format; c->depth_format = depth_format;
  return TSDF_OK;
}
int32_t tsdf_wire_sizes(tsdf_ctx* c, uint64_t* colorsize, uint64_t* depthsize, uint64_t* message_bytes) {
  CHECK_CTX(c);
  uint64_t cs, ds;
  wire_sizes(c, c->color_format, c->depth_format, &cs, &ds);
  if (colorsize) *colorsize = cs;
  if (depthsize) *depthsize = ds;
  if (message_bytes) *message_bytes = (cs + ds) * c->cfg.num_streams;
  return TSDF_OK;
}
int32_t tsdf_set_depth_compression(tsdf_ctx* c, uint32_t i, int32_t compressed, float near_, float far_) {
  CHECK_CTX(c);
  if (i >= c->cfg.num_streams) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "stream %u out of range", i);
  const float scale = far_ - near_;                                      // NetKinectArray.cpp:346-349
  c->pre.compress[i] = compressed != 0; c->pre.dc_near[i] = near_; c->pre.dc_scale[i] = scale; c->pre.dc_scaled_near[i] = scale / 255.0f;
  return TSDF_OK;
}
int32_t tsdf_upload_wire_frame(tsdf_ctx* c, const void* message, uint64_t bytes, double* timestamp) {
  CHECK_CTX(c);
  uint64_t cs, ds;
  wire_sizes(c, c->color_format, c->depth_format, &cs, &ds);
  const uint64_t want = (cs + ds) * c->cfg.num_streams;
  if (!message || bytes != want) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "wire message must be %llu bytes (%u x (colour %llu + depth %llu)), got %llu", (unsigned long long)want, c->cfg.num_streams, (unsigned long long)cs, (unsigned long long)ds, (unsigned long long)bytes);
  HIP_TRY(c, hipSetDevice(c->device));
  if (int32_t rc = ensure_pre_buffers(c)) return rc;
  if (c->wire_capacity < want) {
    HIP_TRY(c, sync_ctx(c));
    c->intake.raw.wire_reallocated();
    for (int k = 0; k < 2; ++k) {
      if (c->h_wire[k]) HIP_TRY(c, hipHostFree(c->h_wire[k]));
      c->h_wire[k] = nullptr;
      HIP_TRY(c, hipHostMalloc((void**)&c->h_wire[k], want, hipHostMallocDefault));
      if (!c->wire_done[k]) HIP_TRY(c, hipEventCreateWithFlags(&c->wire_done[k], hipEventDisableTiming));
    }
    HIP_TRY(c, hipFree(c->d_wire)); c->d_wire = nullptr;
    HIP_TRY(c, hipMalloc(&c->d_wire, want));
    c->wire_capacity = want;
  }
  // double buffer: the copy out of slot k may still be in flight from two frames ago
  const RawFrame::Wire W = c->intake.raw.wire_taken();
  const int k = W.index;
  if (W.wait) HIP_TRY(c, hipEventSynchronize(c->wire_done[k]));
  memcpy(c->h_wire[k], message, want);                                   // readLoop's memcpy into the mapped PBO, :516-520
  if (timestamp) memcpy(timestamp, c->h_wire[k], sizeof(double));        // the first 8 bytes of the message, :510
  const hipStream_t lane = pre_enter(c);                                 // (round 4) the lane ahead: copy, unpack / DXT decode and the passes that follow
  if (int32_t rc = begin_slot_write(c, lane, false)) return rc;
  if (int32_t rc = wait_read_fence(c, kRawRead, lane)) return rc;   // an MVT draw (or a Lab window) still queued on the context's stream reads d_raw
  HIP_TRY(c, hipMemcpyAsync(c->d_wire, c->h_wire[k], want, hipMemcpyHostToDevice, lane));
  HIP_TRY(c, hipEventRecord(c->wire_done[k], lane));
  WireLayout L{};
  L.msg = c->d_wire; L.rec = (uint32_t)(cs + ds); L.cs = (uint32_t)cs; L.n = (int)c->cfg.num_streams;
  L.cw = c->frame.cw; L.ch = c->frame.ch; L.w = c->frame.w; L.h = c->frame.h;
  L.cfmt = (int)c->color_format; L.dfmt = (int)c->depth_format;
  timer_begin_on(c, "0ingest", lane);
  launch_wire_unpack(lane, L, (uchar4*)c->frame.color, c->d_raw);
  timer_end_on(c, "0ingest", lane);
  HIP_TRY(c, hipGetLastError());
  c->intake.raw.uploaded(kRawOwn, false); c->intake.slots.raw_arrived();   // (the unpack wrote the colour into the slot)
  pre_leave(c, lane);
  return TSDF_OK;
}
// the raw frame's colour waits for tsdf_process_textures' first launch: whoever reads the frame slot's colour before that asks for it here
static int32_t flush_pending_colour(tsdf_ctx* c) {
  if (!c->intake.raw.take_colour()) return TSDF_OK;
  const hipStream_t lane = pre_enter(c);
  launch_pack_color(lane, c->pending_rgb, (uchar4*)c->frame.color, (size_t)c->cfg.num_streams * c->frame.cw * c->frame.ch);
  HIP_TRY(c, hipGetLastError());
  pre_leave(c, lane);
  return TSDF_OK;
}
int32_t tsdf_download_raw_frame(tsdf_ctx* c, float* depth_raw, uint8_t* colour_rgba) {
  CHECK_CTX(c);
  if (!c->intake.raw.resident()) FAIL(c, TSDF_ERR_STATE, "no raw frame uploaded");
  HIP_TRY(c, hipSetDevice(c->device));
  if (int32_t rc = flush_pending_colour(c)) return rc;
  HIP_TRY(c, sync_ctx(c));
  const size_t np = (size_t)c->cfg.num_streams * c->frame.w * c->frame.h, nc = (size_t)c->cfg.num_streams * c->frame.cw * c->frame.ch;
  if (depth_raw) HIP_TRY(c, hipMemcpy(depth_raw, raw_depth(c), np * 4, hipMemcpyDeviceToHost));
  if (colour_rgba) HIP_TRY(c, hipMemcpy(colour_rgba, c->frame.color, nc * 4, hipMemcpyDeviceToHost));
  return TSDF_OK;
}
int32_t tsdf_set_preprocess(tsdf_ctx* c, int32_t filter_textures, int32_t processed_depth, int32_t refine) {
  CHECK_CTX(c);
  c->pre.filter_textures = filter_textures != 0; c->intake.raw.set_processed_depth(processed_depth != 0); c->pre.refine = refine != 0;
  return TSDF_OK;
}
static PreBuffers pre_buffers(tsdf_ctx* c) {
  PreBuffers B{};
  B.raw = raw_depth(c); B.depth2 = c->d_depth2; B.fdepth = c->intake.raw.processed_depth() ? c->d_depth2 : B.raw;
  B.depth_rg = c->d_depth_rg; B.lab = c->d_lab; B.depth_b = c->d_depth_b; B.normal = c->d_normal;
  B.dqs = (float4*)c->frame.dqs; B.depth_plane = (float*)c->frame.depth;
  B.cand_count = c->d_pre_blocks; B.cand_list = c->d_pre_blocks + 1; B.cand_cap = c->pre_cand_cap; B.blk_flag = c->d_pre_blocks + 1 + c->pre_cand_cap;
  return B;
}
// phase 0: the five passes.  Phases 1 and 2 are tsdf_frame_raw_dev's split of the same work (round 4): the morph and the filter pass read the raw frame and write
// only intermediate images of the lane's own, so they are queued IN FRONT of the lane's wait for the draws of two frames back (the two-frame cycle end of draw(f) ->
// preparation of f + 2 -> integrate(f + 2) -> draw(f + 2) that bounds the frame from raw data loses their 36 us); phase 2 -- behind that wait -- re-lays the colour out
// into the frame slot and runs the three passes that write what draws read (depth plane, packed texel, range cells, brick counters).
static int32_t process_textures_impl(tsdf_ctx* c, int phase) {
  CHECK_CTX(c);
  if (!c->intake.raw.resident()) FAIL(c, TSDF_ERR_STATE, "no raw frame uploaded (tsdf_upload_raw_frame)");
  for (uint32_t i = 0; i < c->cfg.num_streams; ++i) {
    if (!c->have_calib[i] || !c->luts.s[i].xyz || !c->luts.s[i].uv) FAIL(c, TSDF_ERR_STATE, "stream %u needs cv_xyz and cv_uv (tsdf_set_calibration)", i);
    if (!c->have_limits[i] || !c->have_cam[i]) FAIL(c, TSDF_ERR_STATE, "stream %u needs tsdf_set_depth_limits and tsdf_set_camera_position", i);
  }
  HIP_TRY(c, hipSetDevice(c->device));
  // Round 4: on the lane ahead, like markBricks() -- the passes read the raw frame and write only what the lane owns (the frame slot it flipped to,
  // the brick counters clearOccupiedBricks() flipped to, its own intermediate images), so they run beside the previous frames' integrate and draw.
  const hipStream_t lane = pre_enter(c, phase == 1);
  if (int32_t rc = begin_slot_write(c, lane, true)) return rc;          // (already done by the raw upload of this frame; a re-run of an old raw frame takes the colour along)
  if (phase != 1) { if (int32_t rc = wait_read_fence(c, kNormalsRead, lane)) return rc; }   // the point back-end reads the normal image this call rewrites
  if (int32_t rc = wait_read_fence(c, kProductsRead, lane)) return rc;   // a sensor texture window read the products this call rewrites (phase 1: d_depth2 and the filter pass's images)
  PreParams& P = c->pre;
  P.W = c->frame.w; P.H = c->frame.h; P.N = (int)c->cfg.num_streams;
  for (int a = 0; a < 3; ++a) { P.bbox_min[a] = c->cfg.bbox_min[a]; P.bbox_max[a] = c->cfg.bbox_max[a]; }
  const PreBuffers B = pre_buffers(c);
  c->intake.raw.passes_started();
  const uint8_t* const rgb = phase != 1 && c->intake.raw.take_colour() ? c->pending_rgb : nullptr;   // the colour rides along in the first launch behind the gate
  if (phase != 2) timer_begin_on(c, "1preprocess", lane);
  const size_t ncol = (size_t)c->cfg.num_streams * c->frame.cw * c->frame.ch;
  float4* const ranges = current_slot(c).ranges;
  uchar4* const rgba = (uchar4*)c->frame.color;
  auto launch = [&](unsigned passes, const uint8_t* rgb) { launch_preprocess(lane, P, B, c->luts, c->frame, c->br, ranges, passes, rgb, rgba, ncol); };
  if (phase == 1) launch(kPreMorph | kPreFilter, nullptr);
  else if (phase == 2) launch(kPreRelayout | kPreBoundary | kPreNormal | kPreQuality, rgb);
  else if (c->timers_on && c->timer_filter.find(",k_pre_") != std::string::npos) {   // each pass between its own pair of events, when the timer filter NAMES them (a pair costs the lane ~7 us)
    static const struct { unsigned pass; const char* name; } each[5] = {
        {kPreMorph, "k_pre_morph"}, {kPreFilter, "k_pre_filter"}, {kPreBoundary, "k_pre_boundary"}, {kPreNormal, "k_pre_normal"}, {kPreQuality, "k_pre_quality"}};
    for (const auto& e : each) {
      timer_begin_on(c, e.name, lane);
      launch(e.pass, rgb);
      timer_end_on(c, e.name, lane);
    }
  } else launch(kPreAll, rgb);
  HIP_TRY(c, hipGetLastError());
  if (phase != 1) {
    timer_end_on(c, "1preprocess", lane);
    c->intake.raw.passes_completed(); c->intake.slots.passes_completed();
  }
  pre_leave(c, lane);
  return TSDF_OK;
}
int32_t tsdf_process_textures(tsdf_ctx* c) { return process_textures_impl(c, 0); }
// the Lab image of the filter pass: the passes evaluate it only where the boundary pass reads it (k_pre_boundary); the whole image is produced on request, on the
// context's stream, from the inputs of the frame that was processed -- which must still be the resident ones
static int32_t produce_lab(tsdf_ctx* c) {
  if (!c->intake.raw.lab_current())
    FAIL(c, TSDF_ERR_STATE, "the Lab image is produced on request from the processed frame's inputs, and a newer raw frame has replaced them (download before the next upload)");
  launch_pre_lab(c->stream, c->pre, pre_buffers(c), c->luts, c->frame);
  HIP_TRY(c, hipGetLastError());
  return TSDF_OK;
}
int32_t tsdf_download_preprocessed(tsdf_ctx* c, float* depth2, float* depth_rg, float* lab, float* depth_b, float* sil, float* normals, float* quality) {
  CHECK_CTX(c);
  if (!c->intake.raw.resident()) FAIL(c, TSDF_ERR_STATE, "nothing was pre-processed yet");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_ctx(c));
  const size_t np = (size_t)c->cfg.num_streams * c->frame.w * c->frame.h;
  if (depth2) HIP_TRY(c, hipMemcpy(depth2, c->d_depth2, np * 4, hipMemcpyDeviceToHost));
  if (depth_rg) HIP_TRY(c, hipMemcpy(depth_rg, c->d_depth_rg, np * 8, hipMemcpyDeviceToHost));
  if (depth_b) HIP_TRY(c, hipMemcpy(depth_b, c->d_depth_b, np * 8, hipMemcpyDeviceToHost));
  std::vector<float4> tmp;
  auto fetch4 = [&](const void* src) -> int32_t { tmp.resize(np); HIP_TRY(c, hipMemcpy(tmp.data(), src, np * 16, hipMemcpyDeviceToHost)); return TSDF_OK; };
  int32_t rc;
  if (lab) {
    if ((rc = produce_lab(c))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  if (lab) { if ((rc = fetch4(c->d_lab))) return rc; for (size_t i = 0; i < np; ++i) { lab[3 * i] = tmp[i].x; lab[3 * i + 1] = tmp[i].y; lab[3 * i + 2] = tmp[i].z; } }
  if (normals) { if ((rc = fetch4(c->d_normal))) return rc; for (size_t i = 0; i < np; ++i) { normals[3 * i] = tmp[i].x; normals[3 * i + 1] = tmp[i].y; normals[3 * i + 2] = tmp[i].z; } }
  if (sil || quality) { if ((rc = fetch4(c->frame.dqs))) return rc; for (size_t i = 0; i < np; ++i) { if (quality) quality[i] = tmp[i].y; if (sil) sil[i] = tmp[i].z; } }
  return TSDF_OK;
}

static int32_t require_inputs(tsdf_ctx* c, bool need_xyz, bool need_uv) {
  if (!c->intake.slots.have_frame()) FAIL(c, TSDF_ERR_STATE, "no frame uploaded (tsdf_upload_frame)");
  for (uint32_t i = 0; i < c->cfg.num_streams; ++i) {
    if (!c->have_calib[i]) FAIL(c, TSDF_ERR_STATE, "stream %u has no calibration (tsdf_set_calibration)", i);
    if (need_xyz && !c->luts.s[i].xyz) FAIL(c, TSDF_ERR_STATE, "stream %u has no cv_xyz volume", i);
    if (need_uv && !c->luts.s[i].uv) FAIL(c, TSDF_ERR_STATE, "stream %u has no cv_uv volume", i);
  }
  return TSDF_OK;
}

int32_t tsdf_clear_bricks(tsdf_ctx* c) {
  CHECK_CTX(c);
  HIP_TRY(c, hipSetDevice(c->device));
  const hipStream_t lane = pre_enter(c);
  timer_begin_on(c, "bricks", lane);
  // the lane ahead: the other counter buffer (the previous frame's draw may still read this one), cleared by the frame's re-layout launch already;
  // the context's stream: the buffer the last integrate() zeroed, if it did
  const LaneAhead::Clear C = c->ahead.clear_bricks(lane != c->stream);
  c->br.counters = c->d_counters[C.buffer];
  if (C.fill) HIP_TRY(c, hipMemsetAsync(c->br.counters, 0, c->counter_words * sizeof(uint32_t), lane));
  pre_leave(c, lane);
  return TSDF_OK;
}
int32_t tsdf_mark_bricks(tsdf_ctx* c) {
  CHECK_CTX(c);
  int32_t rc = require_inputs(c, true, false);
  if (rc) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  const hipStream_t lane = pre_enter(c);
  const int word = c->ahead.mark_bricks(lane != c->stream);              // the count of the occupancy set the coming update flips to (or stays on)
  uint32_t* const zero_word = word >= 0 ? c->d_occ_counts + word : nullptr;
  // the peel tiles the coming draw would reset first -- those the draw before the previous one touched, in the peel image that draw used (two alternate
  // while the lanes are on) --: reset here, on the lane ahead, beside the previous frame's kernels
  PeelClear pc{};
  if (const int m = c->tiles_img.peel_reset_ahead(lane != c->stream && c->use_bricks && c->skip_space && c->d_peels_alt); m >= 0) {
    pc.peels = (uint4*)c->d_peels_alt; pc.touched_prev = c->d_touched[m];
    pc.w = c->vw; pc.h = c->vh; pc.ntx = (c->vw + 7) / 8; pc.n_tiles = pc.ntx * ((c->vh + 7) / 8);
  }
  launch_mark_bricks(lane, c->luts, c->frame, c->br, zero_word, pc.peels ? &pc : nullptr);
  HIP_TRY(c, hipGetLastError());
  pre_leave(c, lane);
  return TSDF_OK;
}
int32_t tsdf_update_occupied(tsdf_ctx* c, float* ratio) {
  CHECK_CTX(c);
  HIP_TRY(c, hipSetDevice(c->device));
  const hipStream_t lane = pre_enter(c);
  // the lane ahead: the other occupancy set (flags, list, count) -- the previous frame's integrate / draw may still read this one --, its count
  // zeroed by the marking launch instead of by the previous update (which would zero the word the context's stream is reading)
  const LaneAhead::Update U = c->ahead.update_occupied(lane != c->stream);
  c->br.num_occupied = c->d_occ_counts + U.set; c->br.flags = c->d_flags[U.set]; c->br.occupied = c->d_occupied[U.set];
  if (U.fill) HIP_TRY(c, hipMemsetAsync(c->br.num_occupied, 0, sizeof(uint32_t), lane));
  launch_update_occupied(lane, c->br, c->min_voxels, c->d_occ_counts + U.rearm);
  HIP_TRY(c, hipGetLastError());
  timer_end_on(c, "bricks", lane);
  pre_leave(c, lane);
  if (ratio) return tsdf_occupied_ratio(c, ratio);                     // the reference reads the count back every frame (:432-440); here only on request
  return TSDF_OK;
}
int32_t tsdf_occupied_ratio(tsdf_ctx* c, float* ratio) {
  CHECK_CTX(c);
  if (!ratio) return TSDF_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, join_pre(c));
  HIP_TRY(c, hipMemcpyAsync(c->h_num_occupied, c->br.num_occupied, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, sync_ctx(c));
  *ratio = (float)*c->h_num_occupied / (float)c->br.n;                 // :440
  return TSDF_OK;
}

int32_t tsdf_integrate(tsdf_ctx* c) {
  CHECK_CTX(c);
  int32_t rc = require_inputs(c, false, false);
  if (rc) return rc;
  if (c->vol.slot && !c->use_bricks) FAIL(c, TSDF_ERR_STATE, "a sparse tile pool needs brick culling (setUseBricks(true)): without it every tile is active");
  HIP_TRY(c, hipSetDevice(c->device));
  // the lane: the fourth one and the volume set the previous draw is NOT reading (stage overlap), or the context's stream
  hipStream_t lane = c->stream;
  if (deep_ok(c) && ensure_other_set(c, c->integ_stream)) {
    lane = c->integ_stream;
    const DrawLanes::Integrate I = c->lanes.integrate();
    if (I.record_end) HIP_TRY(c, record_draw_end(c, I.end));             // a draw without hole filling behind it: mark its end now
    if (I.join) HIP_TRY(c, wait_integ(c));                               // (bookkeeping only: the lane is in order, and a draw has normally consumed it)
    bind_volume_set(set_in_use(c), c->vol, c->tiles);                    // (the other set a moment ago: DrawLanes::integrate)
    if (I.wait_draw >= 0) HIP_TRY(c, hipStreamWaitEvent(lane, c->draw_done[I.wait_draw], 0));   // the draw two frames back read this set
    // the frame's images and brick state: from the lane ahead (both this lane and the context's stream wait for it), or from work on the context's stream
    hipError_t e;
    const bool from_lane = consume_pre(c, lane, &e);
    HIP_TRY(c, e);
    if (!from_lane) {
      HIP_TRY(c, hipEventRecord(c->integ_gate, c->stream));
      HIP_TRY(c, hipStreamWaitEvent(lane, c->integ_gate, 0));
    }
  } else {
    HIP_TRY(c, join_integ(c));
    HIP_TRY(c, join_pre(c));
  }
  const bool deep = lane != c->stream;
  timer_begin_on(c, "2integrate", lane);
  int lds = 2;
  for (uint32_t i = 0; i < c->cfg.num_streams; ++i) lds = std::min(lds, c->lds_ok[i]);
  const bool want_cache = lds >= 2 && c->k1_form_cap >= 3 && c->proj_budget > 0 && !c->vol.slot && !c->proj_failed;
  lds = std::min(lds, c->k1_form_cap);
  tsdf_ctx::VolSet& set = set_in_use(c);
  const TileHistory::Begin T = set.history.begin(c->use_bricks);
  const bool full_walk = set.history.full_walk();
  if (c->use_bricks) {
    // this frame's list / count, the previous integrate()'s (trusted unless something else may have written the volume)
    TileState& S = c->tiles;
    S.list = set.list[T.list]; S.count = set.counts + T.list;
    S.prev_list = set.list[T.prev]; S.prev_count = S.next_count = set.counts + T.prev;
    if (T.wipe) HIP_TRY(c, hipMemsetAsync(S.stamp, 0, (size_t)S.n * sizeof(uint32_t), lane));
  }
  // the draw that follows would first reset the peel tiles its predecessor touched: let the classify launch do it
  PeelClear pc{};
  {
    const bool whole = whole_volume(c);
    // (with the lanes on the reset rides on the lane ahead: tsdf_mark_bricks)
    if (const int m = c->tiles_img.peel_reset_classify(!deep && !pipelined(c) && c->use_bricks && !full_walk && c->skip_space && whole && c->d_peels); m >= 0) {
      pc.peels = (uint4*)c->d_peels; pc.touched_prev = c->d_touched[m];                             // the previous draw's tiles
      pc.w = c->vw; pc.h = c->vh; pc.ntx = (c->vw + 7) / 8; pc.n_tiles = pc.ntx * ((c->vh + 7) / 8);
    }
  }
  if (const int k = c->ahead.counters_zero_spare(c->use_bricks && !full_walk && !pipelined(c)); k >= 0) {   // ... and zero the spare counter buffer for the next clearOccupiedBricks() (the lane ahead clears its own)
    pc.zero = c->d_counters[k]; pc.zero_words = (uint32_t)c->counter_words;
  }
  if (c->use_bricks) launch_classify_tiles(lane, c->vol, c->br, c->tiles, full_walk, T.stamp, pc);
  // dense launches: the static half of the uniform-pair shortcut (k_integrate.hip), built once per calibration
  const float4* bounds = nullptr;
  const bool culled_ranges = c->use_bricks && c->culled_ranges && !c->vol.slot && (size_t)c->vol.n_stored_tiles * c->cfg.num_streams * 32 <= ((size_t)512 << 20);
  if ((!c->use_bricks || culled_ranges) && lds >= 2 && c->frame.ranges) {
    if (!c->d_tile_bounds) HIP_TRY(c, hipMalloc((void**)&c->d_tile_bounds, (size_t)c->vol.n_stored_tiles * c->cfg.num_streams * 2 * sizeof(float4)));
    if (!c->d_pair_masks) HIP_TRY(c, hipMalloc((void**)&c->d_pair_masks, (size_t)c->tiles.n * sizeof(uint32_t)));
    if (c->use_recs && !c->d_work_recs) HIP_TRY(c, hipMalloc((void**)&c->d_work_recs, (size_t)c->tiles.n * (sizeof(uint4) + 8 * sizeof(unsigned long long))));   // per tile: the 16-byte record, then (after all records) its 8 x 64 per-voxel bits
    if (!c->tile_bounds_valid) { launch_tile_bounds(lane, c->luts, c->vol, c->d_tile_bounds); c->tile_bounds_valid = true; }
    bounds = c->d_tile_bounds;
  }
  const ProjCache* proj = nullptr;
  if (bounds && want_cache) { if ((rc = ensure_proj_cache(c, &proj))) return rc; }
  c->last_integrate_cached = proj != nullptr;
  // which kernels, with what grids: decided here, once (launch_plan.hpp); the two A/B hooks are read once per process
  static const int forced_grid = [] { const char* e = getenv("RR_K1_GRID"); return e ? atoi(e) : 0; }();
  static const int dense_cap = [] { const char* e = getenv("RR_K1_DENSE_GRID"); return e ? atoi(e) : 16384; }();
  const IntegratePlan plan = plan_integrate(c->use_bricks, lds, c->frame.ranges != nullptr, bounds != nullptr, c->use_recs, proj != nullptr, c->vol.slot != nullptr,
                                            c->tiles.uniform != 0, c->tiles.n, forced_grid, dense_cap);
  c->last_k1 = plan;
  if (plan.pair_pass) {                                                // this frame's (tile, stream) pair classes (+ which work items are cached)
    timer_begin_on(c, "k_pair_masks", lane);
    launch_pair_masks(lane, c->luts, c->frame, c->vol, c->br, c->tiles, plan, bounds, c->d_pair_masks, proj, c->d_work_recs);
    timer_end_on(c, "k_pair_masks", lane);
  }
  timer_begin_on(c, "k_integrate_tiles", lane);                                // the kernel(s) alone (bench.py's roofline)
  launch_integrate_tiles(lane, c->luts, c->frame, c->vol, c->br, c->tiles, plan, c->d_pair_masks, proj, c->d_work_recs);
  timer_end_on(c, "k_integrate_tiles", lane);
  set.history.end(c->use_bricks);
  timer_end_on(c, "2integrate", lane);
  c->have_volume = true;
  HIP_TRY(c, hipGetLastError());
  return TSDF_OK;
}

static int32_t raymarch_impl(tsdf_ctx* c, const float* mv, const float* pr, bool outer_timer) {
  if (!mv || !pr) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "null matrix");
  int32_t rc = require_inputs(c, false, c->shade_mode != 3);
  if (rc) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  ViewParams P;
  if (!make_view_params(c, mv, pr, &P)) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "singular modelview / projection matrix");
  HIP_TRY(c, join_pre(c));
  if (outer_timer) timer_begin(c, "3recon");
  const bool partial = !whole_volume(c);
  const bool shifted = P.vp_org[0] != 0 || P.vp_org[1] != 0 || P.vp_off[0] != 0.0f || P.vp_off[1] != 0.0f;
  if (shifted && partial) FAIL(c, TSDF_ERR_STATE, "a viewport origin / offset is not available on a slab context (the composite indexes pixels)");
  if (shifted) HIP_TRY(c, hipMemsetAsync(c->d_nsamples, 0, (size_t)c->vw * c->vh * sizeof(float), c->stream));   // clearImage of tex_num_samples, :207-208: the stores land at origin + pixel
  // what the tile history (image_tiles.hpp) makes of this draw: first the depth limits, ...
  // (slab contexts too: a tile without a brick under it holds clear values after the march AND after a composite into this target --
  // the brick tables are replicated, so no rank can hit there)
  ImageTiles& T = c->tiles_img;
  const ImageTiles::Limits L = T.draw_limits(P.skip != 0, shifted, masked_direct(c), pipelined(c) && c->d_peels_alt);
  if (P.skip) {
    timer_begin(c, "brickdraw");
    if (L.start_history) {
      const size_t n_img_tiles = (size_t)((c->vw + 7) / 8) * ((c->vh + 7) / 8);
      for (int k = 0; k < 3; ++k) HIP_TRY(c, hipMemsetAsync(c->d_touched[k], 0, n_img_tiles, c->stream));
      if (L.alt_peels) launch_clear_peels(c->stream, c->d_peels_alt, c->vw * c->vh);   // (the other image: all clear, like the one this draw resets in full)
    }
    if (L.swap_peels) std::swap(c->d_peels, c->d_peels_alt);
    launch_depth_limits(c->stream, P, c->br, c->d_peels, L.touched_cur >= 0 ? c->d_touched[L.touched_cur] : nullptr,
                        L.touched_prev >= 0 ? c->d_touched[L.touched_prev] : nullptr, L.already_cleared);
    timer_end(c, "brickdraw");
  }
  // two pyramids alternate while the hole filling runs beside the next frame (stage overlap): this draw takes the other one and only has
  // to wait for the hole filling of the draw BEFORE the previous one -- long finished -- instead of the previous draw's
  const bool two_pyramids = ImageTiles::two_pyramids(c->fill_holes, c->overlap_fill, masked_direct(c));
  const DrawLanes::Pyramid Y = c->lanes.take_pyramid(two_pyramids);
  if (two_pyramids) {
    const int p = Y.index;
    if (!c->atlas_color[p]) {
      const size_t na = (size_t)c->atlas.aw * c->atlas.h;
      HIP_TRY(c, hipMalloc(&c->atlas_color[p], na * sizeof(float4)));
      HIP_TRY(c, hipMalloc(&c->atlas_depth[p], na * sizeof(float)));
      launch_clear_image(c->stream, c->atlas_color[p], c->atlas_depth[p], na, make_float4(0.0f, 1.0f, 0.0f, 0.0f), 1.0f);   // ViewLod::enable's clear
      T.second_pyramid_allocated();
    }
    c->atlas.color = c->atlas_color[p]; c->atlas.depth = c->atlas_depth[p];
  }
  for (int p = 0; p < 2; ++p) HIP_TRY(c, wait_fill(c, p, Y.join[p]));    // (one pyramid: the previous draw's hole filling still reads level 0 / writes the framebuffer)
  // ... then the march
  const ImageTiles::March M = T.draw_march(L.use_tiles, two_pyramids, c->fill_holes, masked_direct(c), partial);
  RayTarget RT = ray_target(c);
  if (L.use_tiles) {
    RT.touched_cur = c->d_touched[M.touched_cur]; RT.touched_prev = c->d_touched[M.touched_prev];
    RT.touched_prev_target = c->d_touched[M.touched_prev_target];
    RT.touched_recycle = c->d_touched[M.touched_recycle];
    RT.rewrite_all = M.rewrite_all; RT.rewrite_target = M.rewrite_target;
    RT.fill_mask = M.fill_mask ? c->d_fill_mask[Y.index] : nullptr;
  }
  HIP_TRY(c, join_integ(c));                                             // the volume: from here on (the depth limits above needed the bricks only)
  const MarchPlan plan = plan_march(partial, P.skip != 0, c->vol.slot != nullptr, c->d_long != nullptr, c->march_cap ? c->march_cap : 0xffffffffu, c->march_box);
  timer_begin(c, "draw");
  timer_begin(c, "k_march");
  launch_march(c->stream, P, c->vol, RT, plan, c->d_hits, c->d_hit_counters, c->hit_parity, c->d_long);
  timer_end(c, "k_march");
  launch_shade(c->stream, P, c->luts, c->frame, c->vol, RT, plan, c->d_hits, c->d_hit_counters, c->hit_parity, c->d_long);
  c->hit_parity ^= 1;
  c->last_two_pass = plan.two_pass;
  c->own_miss_counts = true;
  if (masked_direct(c)) launch_resolve_masked(c->stream, c->atlas, c->vw, c->vh, c->d_fb_c, c->d_fb_d, (int)c->color_mask_mode, c->keep_color ? 1 : 0);
  timer_end(c, "draw");
  c->lanes.draw_marched(c->integ_stream != nullptr);
  HIP_TRY(c, hipGetLastError());
  return TSDF_OK;
}
// ---- the point back-end behind the same Reconstruction interface (kinect::ReconPoints, recon_points.cpp)
int32_t tsdf_upload_normals(tsdf_ctx* c, const float* normals_rgb) {
  CHECK_CTX(c);
  if (!normals_rgb) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "null normals");
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t np = (size_t)c->cfg.num_streams * c->frame.w * c->frame.h;
  if (!c->d_normal) HIP_TRY(c, hipMalloc(&c->d_normal, np * sizeof(float4)));
  std::vector<float4> padded(np);
  for (size_t i = 0; i < np; ++i) padded[i] = make_float4(normals_rgb[3 * i], normals_rgb[3 * i + 1], normals_rgb[3 * i + 2], 0.0f);
  HIP_TRY(c, sync_ctx(c));
  HIP_TRY(c, hipMemcpy(c->d_normal, padded.data(), np * sizeof(float4), hipMemcpyHostToDevice));
  c->intake.raw.normals_were_uploaded();
  return TSDF_OK;
}
int32_t tsdf_view_matrices(const float* mv, const float* pr, uint32_t vw, uint32_t vh, const float* bbox_min, const float* bbox_max, float* out) {
  if (!mv || !pr || !bbox_min || !bbox_max || !out || !vw || !vh) return TSDF_ERR_INVALID_ARGUMENT;
  ViewParams P;
  Mat4 v2w;
  if (!view_matrices(bbox_min, bbox_max, (int)vw, (int)vh, mv, pr, &P, &v2w)) return TSDF_ERR_INVALID_ARGUMENT;
  memcpy(out, v2w.m, 64); memcpy(out + 16, P.img_to_eye.m, 64); memcpy(out + 32, P.normal.m, 64);
  for (int a = 0; a < 3; ++a) out[48 + a] = P.cam_vol[a];
  return TSDF_OK;
}

// the per-pixel 64-bit keys of the depth-keyed draws (raster_dev.hpp) and of the compact composite, allocated on first use
static hipError_t comp_key(tsdf_ctx* c) {
  return c->d_comp_key ? hipSuccess : hipMalloc(&c->d_comp_key, (size_t)c->vw * c->vh * sizeof(unsigned long long));
}
int32_t tsdf_draw_points(tsdf_ctx* c, const float* mv, const float* pr) {
  CHECK_CTX(c);
  if (!mv || !pr) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "null matrix");
  int32_t rc = require_inputs(c, true, true);
  if (rc) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  ViewParams P;
  if (!make_view_params(c, mv, pr, &P)) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "singular modelview / projection matrix");
  PointParams Q{};
  double mvd[16], prd[16], pm[16];
  for (int i = 0; i < 16; ++i) { mvd[i] = mv[i]; prd[i] = pr[i]; }
  mat_mul_d(prd, mvd, pm);
  for (int i = 0; i < 16; ++i) Q.pmv.m[i] = (float)pm[i];
  for (int a = 0; a < 3; ++a) { Q.bbox_min[a] = c->cfg.bbox_min[a]; Q.bbox_max[a] = c->cfg.bbox_max[a]; }
  Q.normals = c->d_normal;
  HIP_TRY(c, comp_key(c));
  FrameImages F = c->frame;
  F.depth = (float*)c->frame.depth;
  HIP_TRY(c, join_pre(c));
  timer_begin(c, "points");
  HIP_TRY(c, begin_framebuffer_write(c));
  launch_draw_points(c->stream, P, Q, c->luts, F, c->d_comp_key, c->d_fb_c, c->d_fb_d);
  timer_end(c, "points");
  if (c->d_normal && pipelined(c)) { if ((rc = record_read_fence(c, kNormalsRead))) return rc; }   // the next tsdf_process_textures() on the lane ahead rewrites the normal image
  HIP_TRY(c, hipGetLastError());
  return TSDF_OK;
}
// kinect::ReconTrigrid (recon_trigrid.cpp)
int32_t tsdf_set_min_length(tsdf_ctx* c, float v) { CHECK_CTX(c); if (!(v > 0.0f)) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "min_length must be positive"); c->min_length = v; return TSDF_OK; }
int32_t tsdf_draw_trigrid(tsdf_ctx* c, const float* mv, const float* pr) {
  CHECK_CTX(c);
  if (!mv || !pr) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "null matrix");
  int32_t rc = require_inputs(c, true, true);
  if (rc) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  ViewParams P;
  if (!make_view_params(c, mv, pr, &P)) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "singular modelview / projection matrix");
  PointParams Q{};
  double mvd[16], prd[16], pm[16];
  for (int i = 0; i < 16; ++i) { mvd[i] = mv[i]; prd[i] = pr[i]; }
  mat_mul_d(prd, mvd, pm);
  for (int i = 0; i < 16; ++i) Q.pmv.m[i] = (float)pm[i];
  for (int a = 0; a < 3; ++a) { Q.bbox_min[a] = c->cfg.bbox_min[a]; Q.bbox_max[a] = c->cfg.bbox_max[a]; }
  const size_t nv = (size_t)c->vw * c->vh;
  if (!c->d_tri_z) { HIP_TRY(c, hipMalloc(&c->d_tri_z, nv * sizeof(uint32_t))); HIP_TRY(c, hipMalloc(&c->d_tri_acc, nv * sizeof(float4))); }
  HIP_TRY(c, join_pre(c));
  timer_begin(c, "trigrid");
  HIP_TRY(c, begin_framebuffer_write(c));
  launch_draw_trigrid(c->stream, P, Q, c->luts, c->frame, c->min_length, c->d_tri_z, c->d_tri_acc, c->d_fb_c, c->d_fb_d);
  timer_end(c, "trigrid");
  HIP_TRY(c, hipGetLastError());
  return TSDF_OK;
}
// kinect::ReconMVT (recon_mvt.cpp): Trigrid's draw() from the raw depth, bilateral-filtered per grid vertex
int32_t tsdf_draw_mvt(tsdf_ctx* c, const float* mv, const float* pr) {
  CHECK_CTX(c);
  if (!mv || !pr) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "null matrix");
  if (!c->intake.raw.resident()) FAIL(c, TSDF_ERR_STATE, "no raw frame uploaded (tsdf_upload_raw_frame / tsdf_upload_raw_frame_dev / tsdf_upload_wire_frame)");
  for (uint32_t i = 0; i < c->cfg.num_streams; ++i) {
    if (!c->have_calib[i] || !c->luts.s[i].xyz || !c->luts.s[i].uv) FAIL(c, TSDF_ERR_STATE, "stream %u needs cv_xyz and cv_uv (tsdf_set_calibration)", i);
  }
  HIP_TRY(c, hipSetDevice(c->device));
  ViewParams P;
  if (!make_view_params(c, mv, pr, &P)) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "singular modelview / projection matrix");
  PointParams Q{};
  double mvd[16], prd[16], pm[16];
  for (int i = 0; i < 16; ++i) { mvd[i] = mv[i]; prd[i] = pr[i]; }
  mat_mul_d(prd, mvd, pm);
  for (int i = 0; i < 16; ++i) Q.pmv.m[i] = (float)pm[i];
  for (int a = 0; a < 3; ++a) { Q.bbox_min[a] = c->cfg.bbox_min[a]; Q.bbox_max[a] = c->cfg.bbox_max[a]; }
  const size_t nv = (size_t)c->vw * c->vh;
  if (!c->d_tri_z) { HIP_TRY(c, hipMalloc(&c->d_tri_z, nv * sizeof(uint32_t))); HIP_TRY(c, hipMalloc(&c->d_tri_acc, nv * sizeof(float4))); }
  if (!c->d_mvt_vtx) HIP_TRY(c, hipMalloc(&c->d_mvt_vtx, (size_t)c->cfg.num_streams * (c->frame.w + 1) * (c->frame.h + 1) * sizeof(float2)));
  if (int32_t rc = flush_pending_colour(c)) return rc;                   // the slot colour of a raw frame nobody has processed yet
  HIP_TRY(c, join_pre(c));
  timer_begin(c, "mvt");
  HIP_TRY(c, begin_framebuffer_write(c));
  launch_draw_mvt(c->stream, P, Q, c->luts, c->frame, raw_depth(c), c->min_length, c->d_mvt_vtx, c->d_tri_z, c->d_tri_acc, c->d_fb_c, c->d_fb_d);
  timer_end(c, "mvt");
  HIP_TRY(c, hipGetLastError());
  c->have_mvt = true;
  if (pipelined(c)) { if (int32_t rc = record_read_fence(c, kRawRead)) return rc; }   // the next raw upload on the lane ahead rewrites d_raw
  return TSDF_OK;
}
int32_t tsdf_download_mvt_vertices(tsdf_ctx* c, float* out) {
  CHECK_CTX(c);
  if (!out) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "null output");
  if (!c->have_mvt) FAIL(c, TSDF_ERR_STATE, "no MVT draw yet (tsdf_draw_mvt)");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_ctx(c));
  HIP_TRY(c, hipMemcpy(out, c->d_mvt_vtx, (size_t)c->cfg.num_streams * (c->frame.w + 1) * (c->frame.h + 1) * sizeof(float2), hipMemcpyDeviceToHost));
  return TSDF_OK;
}
int32_t tsdf_raymarch(tsdf_ctx* c, const float* mv, const float* pr) {
  CHECK_CTX(c);
  int32_t rc = raymarch_impl(c, mv, pr, true);
  if (rc == TSDF_OK) timer_end(c, "3recon");
  return rc;
}
// fillColors(): with stage overlap on its own stream behind an event of the context's stream; *used = the stream it was queued on
static int32_t fill_colors_impl(tsdf_ctx* c, hipStream_t* used) {
  hipStream_t fs = c->stream;
  const int set = c->lanes.set(), pyramid = c->lanes.pyramid();
  if (c->overlap_fill) {
    if (!c->fill_stream) {                                                // (a context created with RR_OVERLAP_FILL=0 and switched on later)
      HIP_TRY(c, hipStreamCreateWithFlags(&c->fill_stream, hipStreamNonBlocking));
      for (hipEvent_t& e : c->fill_done) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    for (hipEvent_t& e : c->draw_done) if (!e) HIP_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_TRY(c, record_draw_end(c, c->lanes.draw_end()));                  // everything the caller queued so far: the march / composite into level 0
    fs = c->fill_stream;
  }
  const bool by_tiles = c->tiles_img.fill(c->color_mask_mode != 0, c->keep_color);
  const uint8_t* tile_mask = by_tiles ? c->d_fill_mask[pyramid] : nullptr;
  ++c->n_fills; c->n_fills_by_tiles += by_tiles ? 1 : 0;
  if (c->overlap_fill && c->fill_thread && !c->timers_on) {              // the helper thread issues the lane's calls (draw_lanes.hpp)
    if (!c->fill_worker) {
      c->fill_worker = new tsdf_ctx::FillWorker();
      c->fill_worker->device = c->device; c->fill_worker->stream = c->fill_stream;
      c->fill_worker->th = std::thread([w = c->fill_worker] { w->run(); });
    }
    tsdf_ctx::FillWorker::Job j{c->atlas, tile_mask, {c->d_lvl_mask[0], c->d_lvl_mask[1]}, c->vw, c->vh, c->d_fb_c, c->d_fb_d, (int)c->color_mask_mode, c->keep_color ? 1 : 0,
                                c->draw_done[set], c->fill_done[pyramid]};
    c->lanes.fill_queued(c->fill_worker->submit(j));
    if (used) *used = c->fill_stream;
    return TSDF_OK;
  }
  if (c->fill_worker) { c->fill_worker->drain(); HIP_TRY(c, fill_worker_error(c)); }   // (earlier jobs first: the lane is in order)
  if (c->overlap_fill) HIP_TRY(c, hipStreamWaitEvent(c->fill_stream, c->draw_done[set], 0));
  timer_begin_on(c, "holefill", fs);
  launch_inpaint_pyramid(fs, c->atlas, tile_mask, c->d_lvl_mask);
  launch_colorfill(fs, c->atlas, c->vw, c->vh, c->d_fb_c, c->d_fb_d, (int)c->color_mask_mode, c->keep_color ? 1 : 0, tile_mask);
  timer_end_on(c, "holefill", fs);
  if (c->overlap_fill) { HIP_TRY(c, hipEventRecord(c->fill_done[pyramid], fs)); c->lanes.fill_queued(); }
  HIP_TRY(c, hipGetLastError());
  if (used) *used = fs;
  return TSDF_OK;
}
int32_t tsdf_fill_colors(tsdf_ctx* c) {
  CHECK_CTX(c);
  if (!c->fill_holes) FAIL(c, TSDF_ERR_STATE, "colour filling is off: the raymarch did not render into the pyramid");
  HIP_TRY(c, hipSetDevice(c->device));
  return fill_colors_impl(c, nullptr);
}
static int32_t brickwire_precheck(tsdf_ctx* c);
static int32_t draw_bricks_impl(tsdf_ctx* c, const float* mv, const float* pr);
// the tail of drawF() behind the raymarch (recon_integration.cpp:160-173): fillColors(), drawOccupiedBricks() when setDrawBricks is on, end of "3recon"
static int32_t draw_f_tail(tsdf_ctx* c, const float* mv, const float* pr) {
  int32_t rc;
  hipStream_t last = c->stream;
  if (c->fill_holes && (rc = fill_colors_impl(c, &last))) return rc;
  if (c->draw_bricks) {
    if ((rc = draw_bricks_impl(c, mv, pr))) return rc;
    last = c->stream;                                                    // (the overlay joined the fill lane)
  }
  timer_end_on(c, "3recon", last);
  return TSDF_OK;
}
int32_t tsdf_draw_f(tsdf_ctx* c, const float* mv, const float* pr) {
  CHECK_CTX(c);
  int32_t rc;
  if (c->draw_bricks && (rc = brickwire_precheck(c))) return rc;         // (before anything is queued)
  if ((rc = raymarch_impl(c, mv, pr, true))) return rc;
  return draw_f_tail(c, mv, pr);
}
int32_t tsdf_frame_dev(tsdf_ctx* c, const float* depth_rg, const float* quality, const float* silhouette, const uint8_t* colour, uint32_t flags, const float* mv, const float* pr) {
  CHECK_CTX(c);
  int32_t rc;
  static const bool prof = getenv("RR_HOST_PROFILE") != nullptr;          // (measurement hook: host time of each step, printed every 1000 frames)
  if (prof) {
    using clk = std::chrono::steady_clock;
    static double acc[6] = {0, 0, 0, 0, 0, 0}; static int n = 0;
    auto t0 = clk::now();
    auto lap = [&](int k) { auto t1 = clk::now(); acc[k] += std::chrono::duration<double, std::micro>(t1 - t0).count(); t0 = t1; };
    if (depth_rg && (rc = tsdf_upload_frame_dev(c, depth_rg, quality, silhouette, colour, flags))) return rc;
    lap(0);
    if ((rc = tsdf_clear_bricks(c))) return rc;
    if ((rc = tsdf_mark_bricks(c))) return rc;
    lap(1);
    if ((rc = tsdf_update_occupied(c, nullptr))) return rc;
    lap(2);
    if ((rc = tsdf_integrate(c))) return rc;
    lap(3);
    if (c->draw_bricks && (rc = brickwire_precheck(c))) return rc;
    if ((rc = raymarch_impl(c, mv, pr, true))) return rc;
    lap(4);
    if ((rc = draw_f_tail(c, mv, pr))) return rc;
    lap(5);
    if (++n % 1000 == 0) { fprintf(stderr, "host us per frame: upload %.1f clear+mark %.1f update %.1f integrate %.1f draw %.1f fill %.1f\n", acc[0] / 1000, acc[1] / 1000, acc[2] / 1000, acc[3] / 1000, acc[4] / 1000, acc[5] / 1000); for (double& a : acc) a = 0; }
    return TSDF_OK;
  }
  if (depth_rg && (rc = tsdf_upload_frame_dev(c, depth_rg, quality, silhouette, colour, flags))) return rc;
  if ((rc = tsdf_clear_bricks(c)) || (rc = tsdf_mark_bricks(c)) || (rc = tsdf_update_occupied(c, nullptr)) || (rc = tsdf_integrate(c))) return rc;
  return tsdf_draw_f(c, mv, pr);
}
// The same from the RAW frame: NetKinectArray::update() + processTextures() in front of the path (kinect_client.cpp:569-577)
int32_t tsdf_frame_raw_dev(tsdf_ctx* c, const float* depth_raw, const uint8_t* colour, uint32_t flags, const float* mv, const float* pr) {
  CHECK_CTX(c);
  int32_t rc;
  const bool split = depth_raw && rrhost::pipelined(c) && !(c->timers_on && c->timer_filter.find(",k_pre_") != std::string::npos);   // (the per-pass timers keep the five passes in one piece)
  if (depth_raw && (rc = upload_raw_frame_dev_impl(c, depth_raw, colour, flags, split))) return rc;
  if (split) {                                                           // morph + filter in front of the lane's gate, the rest behind it (process_textures_impl)
    if ((rc = process_textures_impl(c, 1)) || (rc = tsdf_clear_bricks(c)) || (rc = process_textures_impl(c, 2))) return rc;
  } else if ((rc = tsdf_clear_bricks(c)) || (rc = tsdf_process_textures(c))) return rc;
  if ((rc = tsdf_update_occupied(c, nullptr)) || (rc = tsdf_integrate(c))) return rc;
  return tsdf_draw_f(c, mv, pr);
}
int32_t tsdf_set_stage_overlap(tsdf_ctx* c, int32_t on) {
  CHECK_CTX(c);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_ctx(c));
  c->overlap_fill = on != 0;
  c->tiles_img.drop_history();                                           // one pyramid or two alternating: what the march targets hold changes
  return TSDF_OK;
}

// ---- the overlays of the client's draw3d() in mono mode (kinect_client.cpp:672-683): "Draw TSDF" and "Draw frustums"
static OverlayView overlay_view(const tsdf_ctx* c, const float* mv, const float* pr) {
  OverlayView v;
  memcpy(v.mv.m, mv, 64); memcpy(v.proj.m, pr, 64);
  v.w = c->vw; v.h = c->vh;
  return v;
}
static int32_t overlay_mono(tsdf_ctx* c) {
  if (c->color_mask_mode != 0 || c->vp_org[0] != 0 || c->vp_org[1] != 0 || c->vp_off[0] != 0.0f || c->vp_off[1] != 0.0f)
    FAIL(c, TSDF_ERR_STATE, "the overlays are drawn in mono mode only (colour mask 0, no viewport origin / offset)");
  return TSDF_OK;
}
static int32_t overlay_checks(tsdf_ctx* c, const float* mv, const float* pr, ViewParams* P) {
  if (!mv || !pr) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "null matrix");
  if (!make_view_params(c, mv, pr, P)) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "singular modelview / projection matrix");
  return overlay_mono(c);
}
// fillColors() recorded draw_done[set] BEFORE an overlay, and the integrate() two frames later that overwrites the set waits for that event
// only: record it again behind the overlay
static int32_t overlay_rerecord_draw(tsdf_ctx* c) {
  if (c->integ_stream && c->draw_done[c->lanes.set()]) HIP_TRY(c, record_draw_end(c, c->lanes.draw_end(true)));
  return TSDF_OK;
}
int32_t tsdf_draw_calibvis(tsdf_ctx* c, const float* mv, const float* pr) {
  CHECK_CTX(c);
  ViewParams P;
  if (int32_t rc = overlay_checks(c, mv, pr, &P)) return rc;
  if (!c->have_calib[0] || !c->luts.s[0].inv) FAIL(c, TSDF_ERR_STATE, "stream 0 needs cv_xyz_inv (tsdf_set_calibration): its resolution is the point grid");
  if (!whole_volume(c)) FAIL(c, TSDF_ERR_STATE, "the TSDF overlay needs the whole volume (a Z-slab context holds part of it)");
  HIP_TRY(c, hipSetDevice(c->device));
  CalibVisParams Q{};
  for (int a = 0; a < 3; ++a) {                                          // vol_to_world = translate(bbox_min) * scale(extent), fp32 (recon_calibs.cpp:38-45)
    Q.v2w.m[a * 5] = c->cfg.bbox_max[a] - c->cfg.bbox_min[a];
    Q.v2w.m[12 + a] = c->cfg.bbox_min[a];
    Q.gres[a] = c->luts.s[0].inv_res[a];
    Q.step[a] = 1.0f / (float)Q.gres[a];
  }
  Q.v2w.m[15] = 1.0f;
  Q.view = overlay_view(c, mv, pr);
  // empty-space skip: a tile of class kTileMinus holds -limit (every change of the limit marks every class of both volume sets mixed,
  // tsdf_set_tsdf_limit, so the classes were computed under the current one); such samples are discarded iff -limit <= -0.01
  Q.skip = -c->vol.limit <= -kCalibVisLimit ? 1 : 0;
  HIP_TRY(c, comp_key(c));
  if (!c->d_calibvis_skipped) HIP_TRY(c, hipMalloc(&c->d_calibvis_skipped, sizeof(unsigned long long)));
  Q.skipped = c->d_calibvis_skipped;
  // a draw: the volume of the latest integrate() (the set a raymarch issued now would read), the framebuffer after the hole filling
  HIP_TRY(c, join_pre(c));
  HIP_TRY(c, join_integ(c));
  HIP_TRY(c, begin_framebuffer_write(c));
  timer_begin(c, "calibvis");
  HIP_TRY(c, hipMemsetAsync(c->d_calibvis_skipped, 0, sizeof(unsigned long long), c->stream));
  launch_draw_calibvis(c->stream, Q, c->vol, c->d_comp_key, c->d_fb_c, c->d_fb_d);
  timer_end(c, "calibvis");
  c->calibvis_points = (uint64_t)Q.gres[0] * Q.gres[1] * Q.gres[2];
  if (int32_t rc = overlay_rerecord_draw(c)) return rc;
  HIP_TRY(c, hipGetLastError());
  return TSDF_OK;
}
int32_t tsdf_set_active_kinect(tsdf_ctx* c, uint32_t stream) {
  CHECK_CTX(c);
  if (stream >= c->cfg.num_streams) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "stream %u out of range", stream);
  return TSDF_OK;                                                        // (the layer selects LUT lookups whose results calib_vis.{vs,fs} never use)
}
int32_t tsdf_draw_frustums(tsdf_ctx* c, const float* mv, const float* pr) {
  CHECK_CTX(c);
  ViewParams P;
  if (int32_t rc = overlay_checks(c, mv, pr, &P)) return rc;
  FrustumParams Q{};
  for (uint32_t i = 0; i < c->cfg.num_streams; ++i) {
    if (!c->have_frustum[i]) FAIL(c, TSDF_ERR_STATE, "stream %u needs cv_xyz (tsdf_set_calibration): its corner samples are the frustum", i);
    memcpy(Q.corner[i], c->frustum_corner[i], sizeof(Q.corner[i]));
    memcpy(Q.cam[i], c->frustum_cam[i], sizeof(Q.cam[i]));
  }
  HIP_TRY(c, hipSetDevice(c->device));
  Q.view = overlay_view(c, mv, pr);
  Q.n = (int)c->cfg.num_streams;
  HIP_TRY(c, comp_key(c));
  HIP_TRY(c, begin_framebuffer_write(c));                                // the hole filling writes the framebuffer from its own lane
  timer_begin(c, "frustums");
  launch_draw_frustums(c->stream, Q, c->d_comp_key, c->d_fb_c, c->d_fb_d);
  timer_end(c, "frustums");
  HIP_TRY(c, hipGetLastError());
  return TSDF_OK;
}
int32_t tsdf_draw_bbox(tsdf_ctx* c, const float* mv, const float* pr) {
  CHECK_CTX(c);
  ViewParams P;
  if (int32_t rc = overlay_checks(c, mv, pr, &P)) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  BBoxParams Q{};
  Q.view = overlay_view(c, mv, pr);
  for (int a = 0; a < 3; ++a) { Q.lo[a] = c->cfg.bbox_min[a]; Q.hi[a] = c->cfg.bbox_max[a]; }
  HIP_TRY(c, comp_key(c));
  HIP_TRY(c, begin_framebuffer_write(c));                                // the hole filling writes the framebuffer from its own lane
  timer_begin(c, "bbox");
  launch_draw_bbox(c->stream, Q, c->d_comp_key, c->d_fb_c, c->d_fb_d);
  timer_end(c, "bbox");
  if (int32_t rc = overlay_rerecord_draw(c)) return rc;
  HIP_TRY(c, hipGetLastError());
  return TSDF_OK;
}
// ---- "Draw occupied bricks" (ReconIntegration::drawOccupiedBricks, recon_integration.cpp:447-454)
static int32_t brickwire_precheck(tsdf_ctx* c) {
  if (int32_t rc = overlay_mono(c)) return rc;
  if (12ull * (unsigned long long)c->br.n >= 0xffffffffull) FAIL(c, TSDF_ERR_STATE, "the brick grid is too large for the wireframe's primitive index (12 * bricks + segment in 32 bits)");
  return TSDF_OK;
}
static int32_t draw_bricks_impl(tsdf_ctx* c, const float* mv, const float* pr) {
  const bool plain = getenv("RR_BRICKWIRE_PLAIN") != nullptr;             // (measurement hook: the one-wave-per-segment form)
  BrickWireParams Q{};
  Q.view = overlay_view(c, mv, pr);
  HIP_TRY(c, comp_key(c));
  HIP_TRY(c, begin_framebuffer_write(c));                                // the hole filling writes the framebuffer from its own lane
  // the list of the latest update, from whatever lane ran it.  The join marks the occupancy set as in use by the context's stream, so the
  // next update on the lane ahead takes the other set; the one after that returns to this set behind the lane's gate, which the
  // context's stream records at the next frame's first lane call -- behind this draw, wherever in the frame it was queued.
  HIP_TRY(c, join_pre(c));
  timer_begin(c, "brickwire");
  launch_draw_brickwire(c->stream, Q, c->br, c->d_comp_key, c->d_fb_c, c->d_fb_d, plain);
  timer_end(c, "brickwire");
  if (int32_t rc = overlay_rerecord_draw(c)) return rc;
  HIP_TRY(c, hipGetLastError());
  return TSDF_OK;
}
int32_t tsdf_draw_bricks(tsdf_ctx* c, const float* mv, const float* pr) {
  CHECK_CTX(c);
  ViewParams P;
  if (int32_t rc = overlay_checks(c, mv, pr, &P)) return rc;
  if (int32_t rc = brickwire_precheck(c)) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  return draw_bricks_impl(c, mv, pr);
}
int32_t tsdf_set_draw_bricks(tsdf_ctx* c, int32_t active) {
  CHECK_CTX(c);
  c->draw_bricks = active != 0;
  return TSDF_OK;
}
int32_t tsdf_draw_textures(tsdf_ctx* c, uint32_t which) {
  CHECK_CTX(c);
  if (which > 1) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "texture %u: 0 (unit 15, the hole-filling atlas) or 1 (unit 16, the depth-limit image)", which);
  if (int32_t rc = overlay_mono(c)) return rc;
  if (which == 0 && !c->tiles_img.atlas_complete()) FAIL(c, TSDF_ERR_STATE, "unit 15: no hole filling has completed the atlas since the context was created or resized (or a later march rewrote it)");
  if (which == 1 && !c->tiles_img.limits_complete()) FAIL(c, TSDF_ERR_STATE, "unit 16: no draw with space skipping has produced the depth-limit image since the context was created or resized (or an integrate() reset it for the coming draw)");
  HIP_TRY(c, hipSetDevice(c->device));
  BlitParams Q{};
  const float rf_x = (float)c->atlas.aw, rf_y = (float)c->vh;            // ViewLod::resolution_full, view_lod.cpp:29 (AtlasPlan, grid_plan.hpp)
  Q.vw = (int)(uint32_t)(rf_x / 2.0f); Q.vh = (int)(uint32_t)(rf_y / 2.0f);          // uvec2(fvec2(resolution_full) / 2), kinect_client.cpp:706
  Q.vw = std::min(Q.vw, c->vw); Q.vh = std::min(Q.vh, c->vh);            // (the viewport lies inside the framebuffer: 0.75 w x 0.5 h)
  Q.fw = c->vw;
  if (which == 0) { Q.src = c->atlas.color; Q.peels = 0; Q.sw = c->atlas.aw; Q.sh = c->atlas.h; }
  else { Q.src = c->d_peels; Q.peels = 1; Q.sw = c->vw; Q.sh = c->vh; }
  HIP_TRY(c, begin_framebuffer_write(c));                                // the hole filling completes the atlas and writes the framebuffer on its own lane
  timer_begin(c, "textures");
  launch_blit_texture(c->stream, Q, c->d_fb_c);
  timer_end(c, "textures");
  HIP_TRY(c, hipGetLastError());
  return TSDF_OK;
}
// ---- the GUI's "Show textures" windows (kinect_client.cpp:483-515): one layer of one of NetKinectArray's seven texture arrays as an ImGui::Image
int32_t tsdf_sensor_view_size(const tsdf_ctx* c, float width, float size[2]) {
  CHECK_CTX(c);
  if (!size) return TSDF_ERR_INVALID_ARGUMENT;
  const float aspect = float(c->frame.h) / (float)c->frame.w;             // float(res.y) / res.x of the depth resolution, :506
  size[0] = width; size[1] = width / aspect;                              // ImVec2(width, width / aspect), :509
  return TSDF_OK;
}
int32_t tsdf_draw_sensor_texture(tsdf_ctx* c, uint32_t type, uint32_t stream, const float rect[4], const float clip[4]) {
  CHECK_CTX(c);
  if (type > 6) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "texture type %u: 0 Color, 1 Depth, 2 Quality, 3 Normals, 4 Silhouette, 5 Orig Depth, 6 LAB colors", type);
  if (stream >= c->cfg.num_streams) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "stream %u out of range", stream);
  if (!rect) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "null rect");
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(rect[k]) || (clip && !std::isfinite(clip[k]))) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "rect and clip must be finite");
  if (!(rect[2] > rect[0]) || !(rect[3] > rect[1])) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "empty quad: p_max must be greater than p_min on both axes");
  if (c->vp_org[0] != 0 || c->vp_org[1] != 0 || c->vp_off[0] != 0.0f || c->vp_off[1] != 0.0f)
    FAIL(c, TSDF_ERR_STATE, "the GUI is not rendered side by side (viewport origin / offset must be 0)");
  const WindowVerdict verdict = c->intake.raw.window(type, c->intake.slots.kind());
  switch (verdict) {                                                     // (before anything is queued)
    case kWindowNoFrame: FAIL(c, TSDF_ERR_STATE, "no frame uploaded");
    case kWindowRawUnprocessed: FAIL(c, TSDF_ERR_STATE, "the raw frame uploaded last has not been processed yet (tsdf_process_textures)");
    case kWindowNoSuchImage: FAIL(c, TSDF_ERR_STATE, "a frame handed over already processed has no %s image", type == 5 ? "morphed raw depth" : "Lab");
    case kWindowNoNormals: FAIL(c, TSDF_ERR_STATE, "a frame handed over already processed has normals only after tsdf_upload_normals");
    case kWindowLabStale: FAIL(c, TSDF_ERR_STATE, "the Lab image is produced on request from the processed frame's inputs, and a newer raw frame has replaced them");
    default: break;
  }
  const bool raw = verdict == kWindowRaw;
  HIP_TRY(c, hipSetDevice(c->device));
  const FrameImages& F = c->frame;
  const size_t np = (size_t)F.w * F.h, layer = stream;
  SensorTexParams Q{};
  Q.layer = (int)stream; Q.sw = F.w; Q.sh = F.h;
  switch (type) {
    case 0: Q.mode = kSensorRgba8; Q.src = F.color + layer * (size_t)F.cw * F.ch; Q.sw = F.cw; Q.sh = F.ch; break;
    case 1: if (raw) { Q.mode = kSensorRgNearest; Q.src = c->d_depth_b + layer * np; } else Q.mode = kSensorSlotDepth; break;   // (the slot keeps depth.r alone)
    case 2: Q.mode = kSensorSlotQuality; break;
    case 3: Q.mode = kSensorRgb32f; Q.src = c->d_normal + layer * np; break;
    case 4: Q.mode = kSensorSlotSilhouette; break;
    case 5: Q.mode = kSensorLumNearest; Q.src = c->d_depth2 + layer * np; break;
    default: Q.mode = kSensorRgb32f; Q.src = c->d_lab + layer * np; break;
  }
  // the scissor box of imgui_impl_glfw_glb.cpp:123 cut to the view; NULL: the whole view.  (int) truncates; +-2^30 bounds what a float can ask for
  const int w = c->vw, h = c->vh;
  auto trunc = [](float v) { return (int)std::min(std::max(v, -1073741824.0f), 1073741824.0f); };
  long long bx = 0, by = 0, bw = w, bh = h;
  if (clip) { bx = trunc(clip[0]); by = trunc((float)h - clip[3]); bw = trunc(clip[2] - clip[0]); bh = trunc(clip[3] - clip[1]); }
  if (bw < 0) bw = 0;
  if (bh < 0) bh = 0;
  Q.sx0 = (int)std::max<long long>(bx, 0); Q.sx1 = (int)std::min<long long>(bx + bw, w);
  Q.sy0 = (int)std::max<long long>(by, 0); Q.sy1 = (int)std::min<long long>(by + bh, h);
  for (int a = 0; a < 2; ++a) { Q.pmin[a] = rect[a]; Q.pmax[a] = rect[2 + a]; }
  Q.fw = w; Q.fh = h;
  // the launch rectangle: the quad's pixels, one to spare on every side (the kernel decides each pixel with the definition's own fp32 tests), cut to the box
  const double ylo = (double)h - (double)rect[3], yhi = (double)h - (double)rect[1];
  auto within = [](double v, int n) { return (int)std::min(std::max(v, -1.0), (double)n); };   // (a finite float can be far outside an int)
  const int qx0 = within(std::floor((double)rect[0]) - 1.0, w), qx1 = within(std::ceil((double)rect[2]) + 1.0, w);
  const int qy0 = within(std::floor(ylo) - 1.0, h), qy1 = within(std::ceil(yhi) + 1.0, h);
  Q.x0 = std::max(qx0, Q.sx0); Q.y0 = std::max(qy0, Q.sy0);
  Q.nx = std::min(qx1, Q.sx1) - Q.x0; Q.ny = std::min(qy1, Q.sy1) - Q.y0;
  if (type == 0) { if (int32_t rc = flush_pending_colour(c)) return rc; }
  HIP_TRY(c, begin_framebuffer_write(c));                                // the hole filling writes the framebuffer from its own lane
  HIP_TRY(c, join_pre(c));                                               // the lane ahead wrote the products and the frame slot
  if (raw && type == 6) { if (int32_t rc = produce_lab(c)) return rc; }
  timer_begin(c, "sensortex");
  launch_sensor_texture(c->stream, Q, F, c->d_fb_c);
  timer_end(c, "sensortex");
  // d_depth_b, d_normal, d_depth2, d_lab exist once: the next tsdf_process_textures on the lane ahead waits for this draw (the frame slots alternate behind
  // the lane's gate, which the context's stream records after this call).  The Lab pass also read the raw depth: a raw upload that rewrites d_raw waits too
  if ((type == 3 || (raw && (type == 1 || type >= 5))) && pipelined(c)) {
    if (int32_t rc = record_read_fence(c, kProductsRead)) return rc;
    if (type == 6) { if (int32_t rc = record_read_fence(c, kRawRead)) return rc; }
  }
  HIP_TRY(c, hipGetLastError());
  return TSDF_OK;
}
int32_t tsdf_calibvis_stats(tsdf_ctx* c, uint64_t out[2]) {
  CHECK_CTX(c);
  if (!out) return TSDF_ERR_INVALID_ARGUMENT;
  out[0] = c->calibvis_points; out[1] = 0;
  if (!c->d_calibvis_skipped) return TSDF_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_ctx(c));
  unsigned long long n = 0;
  HIP_TRY(c, hipMemcpy(&n, c->d_calibvis_skipped, sizeof(n), hipMemcpyDeviceToHost));
  out[1] = n;
  return TSDF_OK;
}

// ---- setters
int32_t tsdf_set_tsdf_limit(tsdf_ctx* c, float limit) {
  CHECK_CTX(c);
  if (!(limit > 0.0f)) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "limit must be > 0");
  const bool whole = whole_volume(c);
  // (halo_layers_for, grid_plan.hpp: how far past its faces a limit makes a slab read)
  if (!whole && halo_layers_for(limit, c->res[2]) > c->halo_layers) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "limit needs a wider slab halo than this context allocated");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_ctx(c));
  c->vol.limit = limit;
  for (int k = 0; k < 2; ++k) {                  // the clear value changed: no tile is known to hold it, in either volume set (the one in use first)
    tsdf_ctx::VolSet& s = c->vset[c->lanes.set() ^ k];
    if (!s.data) continue;
    Volume V = c->vol; TileState S = c->tiles;
    bind_volume_set(s, V, S);
    launch_mark_all_mixed(c->stream, S);
    s.history.invalidate();
  }
  HIP_TRY(c, sync_ctx(c));
  return TSDF_OK;
}
// setVoxelSize(), recon_integration.cpp:340-353: res = ceil(bbox / size), a new volume, and the brick grid re-snapped to the new
// voxels from the CURRENT (already snapped) brick size -- the reference passes m_brick_size, not the originally requested value.
int32_t tsdf_set_voxel_size(tsdf_ctx* c, float size) {
  CHECK_CTX(c);
  if (!(size > 0.0f)) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "voxel size must be > 0");
  if (c->cfg.slab_z0 != 0 || c->cfg.slab_z1 != 0) FAIL(c, TSDF_ERR_STATE, "setVoxelSize on a slab context: the slab range is in voxel planes of the old grid (re-create the contexts)");
  const uint32_t by_size[3] = {0, 0, 0};
  const VoxelGrid G = VoxelGrid::of(c->cfg.bbox_min, c->cfg.bbox_max, size, by_size);
  if (G.error) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "volume resolution out of range [1, 4096]");
  if (!c->mstream.ring.idle()) FAIL(c, TSDF_ERR_STATE, "%u streamed mesh frame(s) are queued or held: acquire and release them before the grid changes", c->mstream.ring.count);
  // both plans before anything is touched: a grid that the volume or the bricks refuse leaves the context as it was
  const float brick[3] = {c->br.size[0], c->br.size[1], c->br.size[2]};
  const SlabPlan S = plan_volume(c, G.res);
  if (int32_t rc = refuse_volume(c, S)) return rc;
  const BrickPlan B = BrickPlan::of(c->cfg.bbox_min, c->cfg.bbox_max, G.res, G.vox, brick);
  if (int32_t rc = refuse_bricks(c, B, brick)) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_ctx(c));
  VoxelGrid old{};
  for (int a = 0; a < 3; ++a) { old.res[a] = c->res[a]; old.vox[a] = c->vox[a]; }
  int32_t rc = build_volume(c, G, S);
  if (rc == TSDF_OK) rc = build_bricks(c, B, brick);
  if (rc != TSDF_OK) {                                                   // an allocation failed.  Leave a usable context behind: back to the old grid
    const std::string why = c->err;
    if (setup_volume(c, old) == TSDF_OK) setup_bricks(c, brick);
    c->err = why;
    return rc;
  }
  for (uint32_t i = 0; i < c->cfg.num_streams; ++i) if (c->have_calib[i]) fit_lut_to_volume(c, i);
  HIP_TRY(c, sync_ctx(c));
  return TSDF_OK;
}
int32_t tsdf_set_use_bricks(tsdf_ctx* c, int32_t a) { CHECK_CTX(c); c->use_bricks = a != 0; return TSDF_OK; }
int32_t tsdf_set_space_skip(tsdf_ctx* c, int32_t a) { CHECK_CTX(c); c->skip_space = a != 0; return TSDF_OK; }
int32_t tsdf_set_color_filling(tsdf_ctx* c, int32_t a) { CHECK_CTX(c); c->fill_holes = a != 0; c->tiles_img.drop_history(); return TSDF_OK; }   // the march target changes
int32_t tsdf_set_min_voxels_per_brick(tsdf_ctx* c, uint32_t n) { CHECK_CTX(c); c->min_voxels = n; return TSDF_OK; }
int32_t tsdf_set_shade_mode(tsdf_ctx* c, int32_t m) {
  CHECK_CTX(c);
  if (m < 0 || m > 3) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "shade mode must be 0..3");
  c->shade_mode = m;
  return TSDF_OK;
}
// Reconstruction::setViewportOffset -> uniform viewport_offset (recon_integration.cpp:527); the GL viewport origin is GL state the
// reference reads implicitly through gl_FragCoord (glViewport(x, y, ..), kinect_client.cpp:650,658)
int32_t tsdf_set_viewport_offset(tsdf_ctx* c, float x, float y) { CHECK_CTX(c); c->vp_off[0] = x; c->vp_off[1] = y; c->tiles_img.drop_history(); return TSDF_OK; }
int32_t tsdf_set_viewport_origin(tsdf_ctx* c, int32_t x, int32_t y) {
  CHECK_CTX(c);
  if (x < -(1 << 20) || x > (1 << 20) || y < -(1 << 20) || y > (1 << 20)) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "viewport origin out of range");
  c->vp_org[0] = x; c->vp_org[1] = y; c->tiles_img.drop_history();
  return TSDF_OK;
}
// Reconstruction::setColorMaskMode (reconstruction.cpp:51-53; used recon_integration.cpp:212-216,321-333) and whether the client
// cleared the colour buffer before this draw (glClear(GL_COLOR_BUFFER_BIT | GL_DEPTH_BUFFER_BIT), kinect_client.cpp:609-610,620) or
// only the depth buffer (the anaglyph's second eye, :627)
int32_t tsdf_set_color_mask_mode(tsdf_ctx* c, uint32_t mode) {
  CHECK_CTX(c);
  if (mode > 2) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "colour mask mode must be 0 (all), 1 (red) or 2 (green + blue)");
  c->color_mask_mode = mode; c->tiles_img.drop_history();
  return TSDF_OK;
}
int32_t tsdf_set_framebuffer_clear(tsdf_ctx* c, int32_t clear_color) { CHECK_CTX(c); c->keep_color = clear_color == 0; c->tiles_img.drop_history(); return TSDF_OK; }
int32_t tsdf_set_brick_size(tsdf_ctx* c, const float size[3]) {
  CHECK_CTX(c);
  if (!size) return TSDF_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_ctx(c));
  return setup_bricks(c, size);
}
int32_t tsdf_resize(tsdf_ctx* c, uint32_t w, uint32_t h) {
  CHECK_CTX(c);
  if (!c->present.ring.idle()) FAIL(c, TSDF_ERR_STATE, "%u presented frame(s) are queued or held: acquire and release them before the view changes size", c->present.ring.count);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_ctx(c));
  int32_t rc = setup_view(c, w, h);
  if (rc) return rc;
  HIP_TRY(c, sync_ctx(c));
  return TSDF_OK;
}

// ---- getters
int32_t tsdf_get_resolution(const tsdf_ctx* c, uint32_t res[3], uint32_t rb[3], float bs[3]) {
  CHECK_CTX(c);
  for (int a = 0; a < 3; ++a) { if (res) res[a] = (uint32_t)c->res[a]; if (rb) rb[a] = (uint32_t)c->br.res[a]; if (bs) bs[a] = c->br.size[a]; }
  return TSDF_OK;
}
int32_t tsdf_num_bricks(const tsdf_ctx* c, uint32_t* n) { CHECK_CTX(c); if (!n) return TSDF_ERR_INVALID_ARGUMENT; *n = (uint32_t)c->br.n; return TSDF_OK; }
int32_t tsdf_num_lods(const tsdf_ctx* c, uint32_t* n) { CHECK_CTX(c); if (!n) return TSDF_ERR_INVALID_ARGUMENT; *n = (uint32_t)c->atlas.num_lods; return TSDF_OK; }

// ---- downloads / uploads
static int32_t need_linear(tsdf_ctx* c) {
  if (!c->d_linear) HIP_TRY(c, hipMalloc(&c->d_linear, (size_t)c->res[0] * c->res[1] * c->res[2] * sizeof(float)));
  return TSDF_OK;
}
int32_t tsdf_download_volume(tsdf_ctx* c, float* out) {
  CHECK_CTX(c);
  if (!out) return TSDF_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  int32_t rc = need_linear(c);
  if (rc) return rc;
  HIP_TRY(c, join_integ(c));
  launch_volume_to_linear(c->stream, c->vol, c->d_linear);
  HIP_TRY(c, hipMemcpyAsync(out, c->d_linear, (size_t)c->res[0] * c->res[1] * c->res[2] * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, sync_ctx(c));
  return TSDF_OK;
}
int32_t tsdf_upload_volume(tsdf_ctx* c, const float* in) {
  CHECK_CTX(c);
  if (!in) return TSDF_ERR_INVALID_ARGUMENT;
  if (c->vol.slot) FAIL(c, TSDF_ERR_STATE, "tsdf_upload_volume is not available with a sparse tile pool (tiles get storage from integrate())");
  HIP_TRY(c, hipSetDevice(c->device));
  int32_t rc = need_linear(c);
  if (rc) return rc;
  HIP_TRY(c, sync_ctx(c));
  HIP_TRY(c, hipMemcpyAsync(c->d_linear, in, (size_t)c->res[0] * c->res[1] * c->res[2] * sizeof(float), hipMemcpyHostToDevice, c->stream));
  launch_volume_from_linear(c->stream, c->vol, c->d_linear);
  launch_mark_all_mixed(c->stream, c->tiles);
  set_in_use(c).history.invalidate();
  c->have_volume = true;
  HIP_TRY(c, sync_ctx(c));
  return TSDF_OK;
}
// the storage tiles the last culled integrate() computed (its compacted work list): ids are x-fastest tile indices relative to
// the first integrated tile layer; grid = {tiles along x, tiles along y, first integrated tile layer, integrated tiles}
int32_t tsdf_download_active_tiles(tsdf_ctx* c, uint32_t* ids, uint32_t capacity, uint32_t* count, uint32_t grid[4]) {
  CHECK_CTX(c);
  if (!count) return TSDF_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_ctx(c));
  const tsdf_ctx::VolSet& s = set_in_use(c);
  const int p = s.history.last();
  uint32_t n = 0;
  HIP_TRY(c, hipMemcpy(&n, s.counts + p, sizeof(uint32_t), hipMemcpyDeviceToHost));
  *count = n;
  if (grid) { grid[0] = (uint32_t)c->vol.ntx; grid[1] = (uint32_t)c->vol.nty; grid[2] = (uint32_t)c->vol.int_tz0; grid[3] = (uint32_t)c->tiles.n; }
  if (ids && capacity) HIP_TRY(c, hipMemcpy(ids, s.list[p], (size_t)std::min(n, capacity) * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return TSDF_OK;
}
// which integrate kernel the last tsdf_integrate launched, its grid and its work items: host values of the launcher; the culled launch's
// item count lives on the device (the compacted tile list's length), read like tsdf_download_active_tiles reads it
int32_t tsdf_integrate_form(tsdf_ctx* c, uint32_t out[4]) {
  CHECK_CTX(c);
  if (!out) return TSDF_ERR_INVALID_ARGUMENT;
  if (c->last_k1.form < 0) FAIL(c, TSDF_ERR_STATE, "no integrate() since the volume was set up");
  uint32_t n = (uint32_t)c->tiles.n;
  if (c->last_k1.culled) {
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, sync_ctx(c));
    const tsdf_ctx::VolSet& s = set_in_use(c);
    HIP_TRY(c, hipMemcpy(&n, s.counts + s.history.last(), sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  out[0] = (uint32_t)c->last_k1.form; out[1] = c->last_k1.grid; out[2] = n; out[3] = c->last_k1.culled ? 1u : 0u;
  return TSDF_OK;
}
int32_t tsdf_download_bricks(tsdf_ctx* c, uint32_t* counters, uint8_t* flags) {
  CHECK_CTX(c);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_ctx(c));
  if (counters) HIP_TRY(c, hipMemcpy(counters, c->br.counters, (size_t)c->br.n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (flags) HIP_TRY(c, hipMemcpy(flags, c->br.flags, (size_t)c->br.n, hipMemcpyDeviceToHost));
  return TSDF_OK;
}
int32_t tsdf_upload_brick_counters(tsdf_ctx* c, const uint32_t* counters) {
  CHECK_CTX(c);
  if (!counters) return TSDF_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_ctx(c));
  HIP_TRY(c, hipMemcpy(c->br.counters, counters, (size_t)c->br.n * sizeof(uint32_t), hipMemcpyHostToDevice));
  return TSDF_OK;
}
int32_t tsdf_download_image(tsdf_ctx* c, float* rgba, float* depth, float* ns, float* peels) {
  CHECK_CTX(c);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_ctx(c));
  const RayTarget R = ray_target(c);
  const size_t w = (size_t)c->vw, h = (size_t)c->vh;
  if (rgba) HIP_TRY(c, hipMemcpy2D(rgba, w * 16, R.color, (size_t)R.stride * 16, w * 16, h, hipMemcpyDeviceToHost));
  if (depth) HIP_TRY(c, hipMemcpy2D(depth, w * 4, R.depth, (size_t)R.stride * 4, w * 4, h, hipMemcpyDeviceToHost));
  if (ns) HIP_TRY(c, hipMemcpy(ns, c->d_nsamples, w * h * 4, hipMemcpyDeviceToHost));
  if (peels) {
    HIP_TRY(c, hipMemcpy(peels, c->d_peels, w * h * 16, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < w * h; ++i) { peels[4 * i + 1] = -peels[4 * i + 1]; peels[4 * i + 3] = 0.0f; }   // device keeps max z; reference keeps min(-z)
  }
  return TSDF_OK;
}
int32_t tsdf_upload_image(tsdf_ctx* c, const float* rgba, const float* depth) {
  CHECK_CTX(c);
  if (!rgba || !depth) return TSDF_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_ctx(c));
  const RayTarget R = ray_target(c);
  const size_t w = (size_t)c->vw, h = (size_t)c->vh;
  HIP_TRY(c, hipMemcpy2D(R.color, (size_t)R.stride * 16, rgba, w * 16, w * 16, h, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy2D(R.depth, (size_t)R.stride * 4, depth, w * 4, w * 4, h, hipMemcpyHostToDevice));
  c->tiles_img.target_uploaded(c->fill_holes || masked_direct(c));      // the march target no longer holds what the last march left
  return TSDF_OK;
}
int32_t tsdf_download_framebuffer(tsdf_ctx* c, float* rgba, float* depth) {
  CHECK_CTX(c);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_ctx(c));
  const size_t n = (size_t)c->vw * c->vh;
  if (rgba) HIP_TRY(c, hipMemcpy(rgba, c->d_fb_c, n * 16, hipMemcpyDeviceToHost));
  if (depth) HIP_TRY(c, hipMemcpy(depth, c->d_fb_d, n * 4, hipMemcpyDeviceToHost));
  return TSDF_OK;
}
int32_t tsdf_upload_framebuffer(tsdf_ctx* c, const float* rgba, const float* depth) {
  CHECK_CTX(c);
  if (!rgba || !depth) return TSDF_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_ctx(c));
  const size_t n = (size_t)c->vw * c->vh;
  HIP_TRY(c, hipMemcpy(c->d_fb_c, rgba, n * 16, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(c->d_fb_d, depth, n * 4, hipMemcpyHostToDevice));
  c->tiles_img.framebuffer_written();                                    // (behind the synchronisation above: nothing to join)
  return TSDF_OK;
}
int32_t tsdf_download_atlas(tsdf_ctx* c, float* rgba, float* depth) {
  CHECK_CTX(c);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_ctx(c));
  const size_t n = (size_t)c->atlas.aw * c->atlas.h;
  if (rgba) HIP_TRY(c, hipMemcpy(rgba, c->atlas.color, n * 16, hipMemcpyDeviceToHost));
  if (depth) HIP_TRY(c, hipMemcpy(depth, c->atlas.depth, n * 4, hipMemcpyDeviceToHost));
  return TSDF_OK;
}

// ---- mesh extraction (k_mesh.hip; the definition is in the header).  The reference has no counterpart: it is built on the raymarch's hit test
// (tsdf_raymarch.fs:96), get_gradient (:140-149), blendColors (:295-330) and vol_to_world / NormalMatrix (recon_integration.cpp:66-72,199).
namespace {                                                               // what one extract allocates besides the mesh: freed when it returns
struct MeshTemp { MeshScratch s{}; uint32_t* records = nullptr; ~MeshTemp() { mesh_scratch_free(s, records); } };
}  // namespace
static MeshGeometry mesh_geometry(const tsdf_ctx* c) {
  const float* lo = c->cfg.bbox_min; const float* hi = c->cfg.bbox_max;
  return MeshGeometry{{lo[0], lo[1], lo[2]}, {hi[0], hi[1], hi[2]}};
}
// the attribute flags and the level of an extract or a ring.  report_flags false: the caller reports unknown flags itself, behind the level (the ring's
// configuration names them with its capacities)
static int32_t mesh_flags_level_check(tsdf_ctx* c, uint32_t flags, uint32_t level, bool report_flags = true) {
  if (report_flags && (flags & ~(TSDF_MESH_NORMALS | TSDF_MESH_COLOURS))) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "unknown mesh flag");
  if (level > (uint32_t)kMeshMaxLevel) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "mesh level %u (0 .. %d: every voxel, every 2nd, every 4th)", level, kMeshMaxLevel);
  return TSDF_OK;
}
// the lattice tile layers of this context's slab at a level (result_paths.hpp), or the refusal of a slab whose planes do not lie on the level's tiles
static int32_t mesh_part_layers(tsdf_ctx* c, uint32_t level, MeshPartLayers* layers) {
  const Volume& V = c->vol;
  *layers = MeshPartLayers::of(V.own_tz0, V.own_tz1, (c->res[2] + 7) / 8, (int)level, mesh_lattice(V.res, (int)level).ntz);
  if (!layers->aligned) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "slab planes [%d, %d) do not lie on level %u's lattice tiles (%d planes each)", V.own_tz0 * 8, V.own_tz1 * 8, level, 8 << level);
  return TSDF_OK;
}
// May a call read the fused volume (the extract, the mesh stream, a cast)?  The whole volume on this context, written at least once; with colours also
// calibration and a frame.  on_a_slab: what the call says on a Z-slab context
static int32_t readable_volume_check(tsdf_ctx* c, const char* on_a_slab, bool wants_colour) {
  if (!whole_volume(c)) FAIL(c, TSDF_ERR_STATE, "%s", on_a_slab);
  if (!c->have_volume) FAIL(c, TSDF_ERR_STATE, "no volume yet (tsdf_integrate or tsdf_upload_volume)");
  return wants_colour ? require_inputs(c, false, true) : TSDF_OK;
}
int32_t tsdf_mesh_extract(tsdf_ctx* c, uint32_t flags, uint64_t* n_vertices, uint64_t* n_triangles) { return tsdf_mesh_extract_lod(c, flags, 0u, n_vertices, n_triangles); }
// one extract at a level of detail: level 0 is the voxel lattice (what tsdf_mesh_extract runs), level L the lattice of every (1 << L)-th voxel.  Everything
// per tile -- scratch, scan, records, stats -- is per LATTICE tile of that level.
int32_t tsdf_mesh_extract_lod(tsdf_ctx* c, uint32_t flags, uint32_t level, uint64_t* n_vertices, uint64_t* n_triangles) {
  CHECK_CTX(c);
  if (int32_t rc = mesh_flags_level_check(c, flags, level)) return rc;
  if (int32_t rc = readable_volume_check(c, "tsdf_mesh_extract on a Z-slab context: a slab extracts its part with tsdf_mesh_slab_extract", (flags & TSDF_MESH_COLOURS) != 0)) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  release_mesh(c);                                                       // (nothing queued reads it: extract and download synchronise)
  tsdf_ctx::Mesh& M = c->mesh;
  const Volume& V = c->vol;
  const MeshLattice L = mesh_lattice(V.res, (int)level);                 // (level 0 on a whole-volume context: the storage tiles, n_tiles = V.n_stored_tiles)
  const int n_tiles = L.ntx * L.nty * L.ntz, nb = mesh_scan_blocks(n_tiles);
  M.flags = flags; M.stats[0] = (uint64_t)n_tiles;
  uint64_t totals[4] = {0, 0, 0, 0};
  MeshTemp tmp;
  if (L.cr[0] >= 2 && L.cr[1] >= 2 && L.cr[2] >= 2) {                   // (a lattice one point thick has no cell)
    MeshScratch& S = tmp.s;
    HIP_TRY(c, mesh_scratch_allocate(S, n_tiles, (int)level, nullptr));
    HIP_TRY(c, join_integ(c));                                           // the volume tsdf_download_volume would return now
    if (flags & TSDF_MESH_COLOURS) HIP_TRY(c, join_pre(c));              // ... and the current frame slot's images
    timer_begin(c, "mesh_count");
    launch_mesh_count(c->stream, V, S);
    timer_end(c, "mesh_count");
    timer_begin(c, "mesh_scan");
    launch_mesh_scan(c->stream, S);
    timer_end(c, "mesh_scan");
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(totals, (const char*)S.sums + (size_t)nb * sizeof(totals), sizeof(totals), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, sync_ctx(c));
    if (totals[0] > 0xffffffffull) FAIL(c, TSDF_ERR_OUT_OF_MEMORY, "%llu vertices do not fit 32-bit indices", (unsigned long long)totals[0]);
    if (totals[0]) {
      const size_t nv = (size_t)totals[0], nt = (size_t)totals[1];
      const bool ok = mesh_store_allocate(M, nv, nt, flags) && hipMalloc((void**)&tmp.records, (size_t)totals[2] * 512 * sizeof(uint32_t)) == hipSuccess;
      if (!ok) { (void)hipGetLastError(); release_mesh(c); FAIL(c, TSDF_ERR_OUT_OF_MEMORY, "no device memory for a mesh of %zu vertices and %zu triangles", nv, nt); }
      timer_begin(c, "mesh_emit");
      launch_mesh_emit(c->stream, V, c->luts, c->frame, mesh_geometry(c), S, tmp.records, M.pos, M.nrm, M.col, M.tri);
      timer_end(c, "mesh_emit");
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, sync_ctx(c));
    }
  }
  M.nv = totals[0]; M.nt = totals[1]; M.valid = true;
  M.stats[1] = totals[3]; M.stats[2] = totals[2];
  M.stats[3] = mesh_store_bytes(M);
  if (n_vertices) *n_vertices = M.nv;
  if (n_triangles) *n_triangles = M.nt;
  return TSDF_OK;
}
static int32_t mesh_attribute_check(tsdf_ctx* c, bool want_normals, bool want_colours) {
  if (!c->mesh.valid) FAIL(c, TSDF_ERR_STATE, "no mesh (tsdf_mesh_extract)");
  if (want_normals && !(c->mesh.flags & TSDF_MESH_NORMALS)) FAIL(c, TSDF_ERR_STATE, "the last tsdf_mesh_extract produced no normals");
  if (want_colours && !(c->mesh.flags & TSDF_MESH_COLOURS)) FAIL(c, TSDF_ERR_STATE, "the last tsdf_mesh_extract produced no colours");
  return TSDF_OK;
}
int32_t tsdf_mesh_download(tsdf_ctx* c, float* position_xyz, float* normal_xyz, float* colour_rgba, uint32_t* triangles) {
  CHECK_CTX(c);
  int32_t rc = mesh_attribute_check(c, normal_xyz != nullptr, colour_rgba != nullptr);
  if (rc) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, mesh_store_download(c->mesh, position_xyz, normal_xyz, colour_rgba, triangles));
  return TSDF_OK;
}
int32_t tsdf_mesh_write_ply(tsdf_ctx* c, const char* path) {
  CHECK_CTX(c);
  if (!path) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "null path");
  int32_t rc = mesh_attribute_check(c, false, false);
  if (rc) return rc;
  const tsdf_ctx::Mesh& M = c->mesh;
  const bool nrm = (M.flags & TSDF_MESH_NORMALS) != 0, col = (M.flags & TSDF_MESH_COLOURS) != 0;
  std::vector<float> p((size_t)M.nv * 3), n(nrm ? (size_t)M.nv * 3 : 0), k(col ? (size_t)M.nv * 4 : 0);
  std::vector<uint32_t> t((size_t)M.nt * 3);
  if ((rc = tsdf_mesh_download(c, p.data(), nrm ? n.data() : nullptr, col ? k.data() : nullptr, t.data()))) return rc;
  std::string why;
  rc = rr_write_mesh_ply(path, M.nv, M.nt, p.data(), nrm ? n.data() : nullptr, col ? k.data() : nullptr, t.data(), &why);
  if (rc) c->err = why;
  return rc;
}
int32_t tsdf_mesh_stats(tsdf_ctx* c, uint64_t out[4]) {
  CHECK_CTX(c);
  if (!out) return TSDF_ERR_INVALID_ARGUMENT;
  int32_t rc = mesh_attribute_check(c, false, false);
  if (rc) return rc;
  for (int k = 0; k < 4; ++k) out[k] = c->mesh.stats[k];
  return TSDF_OK;
}

// ---- a Z-slab's part of the mesh (k_mesh_slab.hip; the definition is in the header).  Extract: count, scan and vertices of the owned lattice tile layers
// and the records of the seam layer's plane 0; link: the triangles, once the caller knows where the part starts and what the slab above begins with.
int32_t tsdf_mesh_slab_extract(tsdf_ctx* c, uint32_t flags, uint32_t level, uint64_t* n_vertices, uint64_t* n_triangles) {
  CHECK_CTX(c);
  // The part of an earlier extract goes FIRST, before any argument is looked at: whatever this call answers, seam / link / download / stats never
  // serve a part whose sizes the caller no longer holds (nothing queued reads it: extract, link and download synchronise).
  HIP_TRY(c, hipSetDevice(c->device));
  release_mesh_slab(c);
  if (int32_t rc = mesh_flags_level_check(c, flags, level)) return rc;
  if (!c->have_volume) FAIL(c, TSDF_ERR_STATE, "no volume yet (tsdf_integrate or tsdf_upload_volume)");
  if (flags & TSDF_MESH_COLOURS) if (int32_t rc = require_inputs(c, false, true)) return rc;
  const Volume& V = c->vol;
  const MeshLattice L = mesh_lattice(V.res, (int)level);
  MeshPartLayers layers;
  if (int32_t rc = mesh_part_layers(c, level, &layers)) return rc;
  const bool top = layers.top;
  // The halo holds every plane a vertex of this slab reads (the header says why): voxel plane z1 + stride for the seam records, and the gradient taps'
  // footprint x + 1 planes past either face, x = limit / 2 * res_z, against 8 * halo_layers >= 2 x + 2.  Checked all the same, never clamped silently.
  if (!top && V.tz1 - V.own_tz1 < 1) FAIL(c, TSDF_ERR_STATE, "the slab stores no halo layer above its planes");
  tsdf_ctx::MeshSlabPart& P = c->mslab;
  P.slab = MeshSlab{layers.layer0, (layers.layer1 - layers.layer0) * L.ntx * L.nty, top ? 0 : L.ntx * L.nty};
  P.ntx = L.ntx; P.nty = L.nty; P.flags = flags;
  P.seam_cnt.assign((size_t)P.slab.n_seam, 0u);
  P.stats[0] = (uint64_t)P.slab.n_own;
  const int n_tiles = P.slab.n_own + P.slab.n_seam, nb = mesh_scan_blocks(n_tiles);
  uint64_t totals[4] = {0, 0, 0, 0}, seam_vertices = 0, seam_surface = 0;
  if (L.cr[0] >= 2 && L.cr[1] >= 2 && L.cr[2] >= 2 && P.slab.n_own > 0) {   // (a lattice one point thick has no cell)
    MeshScratch& S = P.scratch;
    auto fail = [&](hipError_t e) { (void)hipGetLastError(); release_mesh_slab(c); c->err = std::string("tsdf_mesh_slab_extract: ") + hipGetErrorString(e);
                                    return e == hipErrorOutOfMemory ? TSDF_ERR_OUT_OF_MEMORY : TSDF_ERR_HIP; };
    if (const hipError_t e = mesh_scratch_allocate(S, n_tiles, (int)level, nullptr)) return fail(e);
    HIP_TRY(c, join_integ(c));                                           // the volume tsdf_download_volume would return now
    if (flags & TSDF_MESH_COLOURS) HIP_TRY(c, join_pre(c));              // ... and the current frame slot's images
    timer_begin(c, "mesh_slab_count");
    launch_mesh_slab_count(c->stream, V, S, P.slab);
    timer_end(c, "mesh_slab_count");
    timer_begin(c, "mesh_slab_scan");
    launch_mesh_scan(c->stream, S);
    timer_end(c, "mesh_slab_scan");
    if (const hipError_t e = hipGetLastError()) return fail(e);
    std::vector<uint2> seam((size_t)P.slab.n_seam);
    if (const hipError_t e = hipMemcpyAsync(totals, (const char*)S.sums + (size_t)nb * sizeof(totals), sizeof(totals), hipMemcpyDeviceToHost, c->stream)) return fail(e);
    if (P.slab.n_seam)
      if (const hipError_t e = hipMemcpyAsync(seam.data(), S.tile_cnt + P.slab.n_own, seam.size() * sizeof(uint2), hipMemcpyDeviceToHost, c->stream)) return fail(e);
    if (const hipError_t e = sync_ctx(c)) return fail(e);
    if (totals[0] > 0xffffffffull) { release_mesh_slab(c); FAIL(c, TSDF_ERR_OUT_OF_MEMORY, "%llu vertices do not fit 32-bit indices", (unsigned long long)totals[0]); }
    for (size_t k = 0; k < seam.size(); ++k) { P.seam_cnt[k] = seam[k].x; seam_vertices += seam[k].x; seam_surface += seam[k].x ? 1u : 0u; }
    if (totals[2]) {                                                     // tiles with surface, seam tiles included: records for all of them
      const size_t nv = (size_t)(totals[0] - seam_vertices), nt = (size_t)totals[1];
      const bool ok = mesh_store_allocate(P, nv, nt, flags) && hipMalloc((void**)&P.records, (size_t)totals[2] * 512 * sizeof(uint32_t)) == hipSuccess;
      if (!ok) { (void)hipGetLastError(); release_mesh_slab(c); FAIL(c, TSDF_ERR_OUT_OF_MEMORY, "no device memory for a slab mesh of %zu vertices and %zu triangles", nv, nt); }
      timer_begin(c, "mesh_slab_emit");
      launch_mesh_slab_vertices(c->stream, V, c->luts, c->frame, mesh_geometry(c), S, P.slab, P.records, P.pos, P.nrm, P.col);
      timer_end(c, "mesh_slab_emit");
      if (const hipError_t e = hipGetLastError()) return fail(e);
      if (const hipError_t e = sync_ctx(c)) return fail(e);
    }
  }
  P.nv = totals[0] - seam_vertices; P.nt = totals[1]; P.valid = true; P.linked = false;
  P.stats[1] = totals[3]; P.stats[2] = totals[2] - seam_surface;
  P.stats[3] = mesh_store_bytes(P);
  if (n_vertices) *n_vertices = P.nv;
  if (n_triangles) *n_triangles = P.nt;
  return TSDF_OK;
}
int32_t tsdf_mesh_slab_seam(tsdf_ctx* c, uint32_t* out) {
  CHECK_CTX(c);
  if (!out) return TSDF_ERR_INVALID_ARGUMENT;
  const tsdf_ctx::MeshSlabPart& P = c->mslab;
  if (!P.valid) FAIL(c, TSDF_ERR_STATE, "no slab mesh (tsdf_mesh_slab_extract)");
  const size_t n = (size_t)P.ntx * P.nty;
  if (!P.scratch.tile_vbase) { std::fill(out, out + n, 0u); return TSDF_OK; }   // (a lattice without a cell: nothing was counted)
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpy(out, P.scratch.tile_vbase, n * sizeof(uint32_t), hipMemcpyDeviceToHost));   // the first owned layer's tiles come first
  return TSDF_OK;
}
int32_t tsdf_mesh_slab_link(tsdf_ctx* c, uint64_t vertex_base, const uint32_t* above_seam) {
  CHECK_CTX(c);
  tsdf_ctx::MeshSlabPart& P = c->mslab;
  if (!P.valid) FAIL(c, TSDF_ERR_STATE, "no slab mesh (tsdf_mesh_slab_extract)");
  const bool top = c->vol.own_tz1 == (c->res[2] + 7) / 8;
  if (!above_seam && !top) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "a slab below the volume's top needs the seam table of the slab above");
  // every index the triangles can hold, from what the host knows: the slab's own vertices, and per seam tile the plane-0 vertices behind its base
  uint64_t end = vertex_base + P.nv;
  if (above_seam)
    for (size_t k = 0; k < P.seam_cnt.size(); ++k)
      if (P.seam_cnt[k]) end = std::max(end, vertex_base + P.nv + above_seam[k] + P.seam_cnt[k]);
  if (end > 0xffffffffull || vertex_base > 0xffffffffull) FAIL(c, TSDF_ERR_OUT_OF_MEMORY, "indices up to %llu do not fit 32 bits", (unsigned long long)end);
  HIP_TRY(c, hipSetDevice(c->device));
  release_mesh_slab_components(c);                                       // (they hold the indices of the link that was)
  if (P.nt) {
    if (P.slab.n_seam) {
      if (!P.above) HIP_TRY(c, hipMalloc((void**)&P.above, (size_t)P.slab.n_seam * sizeof(uint32_t)));
      HIP_TRY(c, hipMemcpyAsync(P.above, above_seam, (size_t)P.slab.n_seam * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    }
    timer_begin(c, "mesh_slab_link");
    launch_mesh_slab_triangles(c->stream, c->vol, P.scratch, P.slab, P.records, (uint32_t)vertex_base, (uint32_t)P.nv, P.above, P.tri);
    timer_end(c, "mesh_slab_link");
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, sync_ctx(c));                                             // (above_seam is the caller's again)
  }
  P.linked = true; P.vertex_base = vertex_base; P.index_end = end;
  return TSDF_OK;
}
int32_t tsdf_mesh_slab_download(tsdf_ctx* c, float* position_xyz, float* normal_xyz, float* colour_rgba, uint32_t* triangles) {
  CHECK_CTX(c);
  const tsdf_ctx::MeshSlabPart& P = c->mslab;
  if (!P.valid) FAIL(c, TSDF_ERR_STATE, "no slab mesh (tsdf_mesh_slab_extract)");
  if (normal_xyz && !(P.flags & TSDF_MESH_NORMALS)) FAIL(c, TSDF_ERR_STATE, "the last tsdf_mesh_slab_extract produced no normals");
  if (colour_rgba && !(P.flags & TSDF_MESH_COLOURS)) FAIL(c, TSDF_ERR_STATE, "the last tsdf_mesh_slab_extract produced no colours");
  if (triangles && !P.linked) FAIL(c, TSDF_ERR_STATE, "the slab's triangles have no indices yet (tsdf_mesh_slab_link)");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, mesh_store_download(P, position_xyz, normal_xyz, colour_rgba, triangles));
  return TSDF_OK;
}
int32_t tsdf_mesh_slab_stats(tsdf_ctx* c, uint64_t out[4]) {
  CHECK_CTX(c);
  if (!out) return TSDF_ERR_INVALID_ARGUMENT;
  if (!c->mslab.valid) FAIL(c, TSDF_ERR_STATE, "no slab mesh (tsdf_mesh_slab_extract)");
  for (int k = 0; k < 4; ++k) out[k] = c->mslab.stats[k];
  return TSDF_OK;
}

// ---- the components of a slab's linked part (k_mesh_slab_components.hip, mesh_cc_seams.hpp; the definition is in the header).  Step 1 labels the part
// alone and exports what crosses its seams, the merge is a host function of all slabs' lists, step 3 turns the merged links into global numbers.
namespace {
struct DeviceTemp {                                                       // device memory of one call: freed when it returns unless handed on
  std::vector<void*> owned;
  ~DeviceTemp() { for (void* p : owned) hipFree(p); }
  bool get(void* out, size_t bytes) {                                    // out: the address of a pointer of any type (no template inside extern "C")
    void* p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) { (void)hipGetLastError(); return false; }
    owned.push_back(p); *(void**)out = p;
    return true;
  }
  void hand_on(const void* p) { owned.erase(std::remove(owned.begin(), owned.end(), p), owned.end()); }
};
}  // namespace
int32_t tsdf_mesh_slab_components(tsdf_ctx* c, uint64_t out[4]) {
  CHECK_CTX(c);
  if (!out) return TSDF_ERR_INVALID_ARGUMENT;
  const tsdf_ctx::MeshSlabPart& P = c->mslab;
  if (!P.valid || !P.linked) FAIL(c, TSDF_ERR_STATE, "no linked slab mesh (tsdf_mesh_slab_extract, then tsdf_mesh_slab_link)");
  if (P.nt > 0xffffffffull) FAIL(c, TSDF_ERR_OUT_OF_MEMORY, "%llu triangles do not fit a component's 32-bit count", (unsigned long long)P.nt);
  HIP_TRY(c, hipSetDevice(c->device));
  tsdf_ctx::MeshSlabComponents made;
  made.labelled = true;
  if (P.nv) {
    const uint32_t nv = (uint32_t)P.nv, n = (uint32_t)(P.index_end - P.vertex_base);   // (the link has checked: index_end <= 2^32)
    const int nb_own = mesh_sc_scan_blocks(nv), nb_up = mesh_sc_scan_blocks(n - nv);
    DeviceTemp tmp;
    MeshSlabLabelling W{P.tri, (size_t)P.nt, nv, n, (uint32_t)P.vertex_base, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    unsigned long long* sums = nullptr;
    bool ok = tmp.get(&W.parent, (size_t)n * 4) && tmp.get(&W.label, (size_t)n * 4) && tmp.get(&W.rank, (size_t)nv * 4) && tmp.get(&W.down_mark, (size_t)nv * 2) &&
              tmp.get(&sums, (size_t)(3 * (nb_own + 1) + nb_up + 1) * 8);
    if (!ok) FAIL(c, TSDF_ERR_OUT_OF_MEMORY, "no device memory for the components of a part of %u vertices", nv);
    W.seam_root = W.down_mark + nv;
    W.root_sums = sums; W.down_sums = sums + (nb_own + 1); W.seam_sums = sums + 2 * (nb_own + 1); W.up_sums = sums + 3 * (nb_own + 1);
    HIP_TRY(c, hipMemsetAsync(W.down_mark, 0, (size_t)nv * 2, c->stream));
    timer_begin(c, "mesh_slab_components");
    launch_mesh_sc_label(c->stream, W, P.scratch, P.records, P.slab.layer0 > 0 ? P.ntx * P.nty : 0);
    timer_end(c, "mesh_slab_components");
    HIP_TRY(c, hipGetLastError());
    unsigned long long n_local = 0, n_down = 0, n_up = 0, n_roots = 0;
    HIP_TRY(c, hipMemcpyAsync(&n_local, W.root_sums + nb_own, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&n_down, W.down_sums + nb_own, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&n_up, W.up_sums + nb_up, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, sync_ctx(c));                                             // (the lists are sized exactly: the host has to know the counts)
    tsdf_mesh_component* local = nullptr; tsdf_mesh_seam_vertex* down = nullptr; tsdf_mesh_seam_vertex* up = nullptr; tsdf_mesh_seam_root* roots = nullptr;
    ok = tmp.get(&local, (size_t)n_local * sizeof(*local)) && tmp.get(&down, (size_t)n_down * sizeof(*down)) && tmp.get(&up, (size_t)n_up * sizeof(*up)) &&
         tmp.get(&roots, (size_t)(n_down + n_up) * sizeof(*roots));      // (at most one root per seam record)
    if (!ok) FAIL(c, TSDF_ERR_OUT_OF_MEMORY, "no device memory for %llu local components and %llu seam records", n_local, n_down + n_up);
    timer_begin(c, "mesh_slab_components");                              // (a second sample of the same call: the host's allocation lies between the two)
    launch_mesh_sc_lists(c->stream, W, local, down, up, roots);
    timer_end(c, "mesh_slab_components");
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(&n_roots, W.seam_sums + nb_own, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, sync_ctx(c));
    made.host_roots.resize((size_t)n_roots);
    if (n_roots) HIP_TRY(c, hipMemcpy(made.host_roots.data(), roots, (size_t)n_roots * sizeof(*roots), hipMemcpyDeviceToHost));
    made.label = W.label; made.rank = W.rank; made.local = local; made.down = down; made.up = up; made.roots = roots;
    for (const void* p : {(const void*)W.label, (const void*)W.rank, (const void*)local, (const void*)down, (const void*)up, (const void*)roots}) tmp.hand_on(p);
    made.n_index = n; made.n_local = n_local; made.n_down = n_down; made.n_up = n_up;
  }
  release_mesh_slab_components(c);                                       // (an earlier labelling of the same link: the same words)
  c->mslabc = std::move(made);
  const tsdf_ctx::MeshSlabComponents& K = c->mslabc;
  out[0] = K.n_local; out[1] = K.n_down; out[2] = K.n_up; out[3] = K.host_roots.size();
  return TSDF_OK;
}
int32_t tsdf_mesh_slab_component_seam(tsdf_ctx* c, tsdf_mesh_seam_vertex* down, tsdf_mesh_seam_vertex* up, tsdf_mesh_seam_root* roots) {
  CHECK_CTX(c);
  const tsdf_ctx::MeshSlabComponents& K = c->mslabc;
  if (!K.labelled) FAIL(c, TSDF_ERR_STATE, "no components of the slab's part (tsdf_mesh_slab_components after the link)");
  HIP_TRY(c, hipSetDevice(c->device));
  if (down && K.n_down) HIP_TRY(c, hipMemcpy(down, K.down, (size_t)K.n_down * sizeof(*down), hipMemcpyDeviceToHost));
  if (up && K.n_up) HIP_TRY(c, hipMemcpy(up, K.up, (size_t)K.n_up * sizeof(*up), hipMemcpyDeviceToHost));
  if (roots && !K.host_roots.empty()) std::copy(K.host_roots.begin(), K.host_roots.end(), roots);
  return TSDF_OK;
}
int32_t tsdf_mesh_merge_component_seams(const tsdf_mesh_component_seams* slabs, uint32_t n_slabs, uint64_t* component_base, tsdf_mesh_component_link* links,
                                        uint64_t* n_components) {
  return merge_component_seams(slabs, n_slabs, component_base, links, n_components) ? TSDF_ERR_INVALID_ARGUMENT : TSDF_OK;
}
int32_t tsdf_mesh_slab_link_components(tsdf_ctx* c, uint64_t component_base, const tsdf_mesh_component_link* links, uint64_t n_links, uint64_t* n_owned) {
  CHECK_CTX(c);
  tsdf_ctx::MeshSlabComponents& K = c->mslabc;
  const tsdf_ctx::MeshSlabPart& P = c->mslab;
  if (!K.labelled) FAIL(c, TSDF_ERR_STATE, "no components of the slab's part (tsdf_mesh_slab_components after the link)");
  if (n_links && !links) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "null links");
  // before any launch: a link names its root and final root by index, and only indices this slab exported itself may reach the scatter
  if (const int why = component_links_check(K.host_roots.data(), K.host_roots.size(), P.vertex_base, links, n_links))
    FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "the links are not those of this slab's %zu root records (mesh_cc_seams.hpp: component_links_check = %d)", K.host_roots.size(), why);
  if (component_base + K.n_local > 0x100000000ull) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "component numbers from %llu on do not fit 32 bits", (unsigned long long)component_base);
  HIP_TRY(c, hipSetDevice(c->device));
  uint64_t removed = 0;
  for (uint64_t i = 0; i < n_links; ++i) removed += links[i].final_root != links[i].root ? 1u : 0u;
  unsigned long long owned = 0;
  uint32_t* vertex = nullptr; uint32_t* triangle = nullptr; tsdf_mesh_component* table = nullptr;
  DeviceTemp tmp;
  if (P.nv) {
    const uint32_t nv = (uint32_t)P.nv;
    const int nb = mesh_sc_scan_blocks(nv);
    tsdf_mesh_component_link* d_links = nullptr; uint32_t* link_of = nullptr; uint32_t* number = nullptr; unsigned long long* sums = nullptr;
    const bool ok = tmp.get(&d_links, (size_t)n_links * sizeof(*links)) && tmp.get(&link_of, (size_t)nv * 4) && tmp.get(&number, (size_t)nv * 4) &&
                    tmp.get(&sums, (size_t)(nb + 1) * 8) && tmp.get(&vertex, (size_t)nv * 4) && tmp.get(&triangle, (size_t)P.nt * 4) &&
                    tmp.get(&table, (size_t)K.n_local * sizeof(*table));
    if (!ok) FAIL(c, TSDF_ERR_OUT_OF_MEMORY, "no device memory to number the components of a part of %u vertices", nv);
    if (n_links) HIP_TRY(c, hipMemcpyAsync(d_links, links, (size_t)n_links * sizeof(*links), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(link_of, 0xff, (size_t)nv * 4, c->stream));
    const MeshSlabLabelling W{P.tri, (size_t)P.nt, nv, (uint32_t)K.n_index, (uint32_t)P.vertex_base, nullptr, K.label, K.rank, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    timer_begin(c, "mesh_slab_components_link");
    launch_mesh_sc_link(c->stream, W, K.local, d_links, (uint32_t)n_links, (uint32_t)component_base, link_of, number, sums, vertex, triangle, table);
    timer_end(c, "mesh_slab_components_link");
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(&owned, sums + nb, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, sync_ctx(c));                                             // (links is the caller's again)
  }
  hipFree(K.vertex); hipFree(K.triangle); hipFree(K.table);              // (an earlier link of the same labelling)
  K.vertex = vertex; K.triangle = triangle; K.table = table;
  for (const void* p : {(const void*)vertex, (const void*)triangle, (const void*)table}) tmp.hand_on(p);
  K.n_owned = owned; K.removed = removed; K.linked = true;
  if (n_owned) *n_owned = owned;
  return TSDF_OK;
}
int32_t tsdf_mesh_slab_download_components(tsdf_ctx* c, uint32_t* vertex_component, uint32_t* triangle_component, tsdf_mesh_component* table) {
  CHECK_CTX(c);
  const tsdf_ctx::MeshSlabComponents& K = c->mslabc;
  if (!K.labelled || !K.linked) FAIL(c, TSDF_ERR_STATE, "the part's components have no global numbers yet (tsdf_mesh_slab_components, tsdf_mesh_slab_link_components)");
  HIP_TRY(c, hipSetDevice(c->device));
  if (vertex_component && c->mslab.nv) HIP_TRY(c, hipMemcpy(vertex_component, K.vertex, (size_t)c->mslab.nv * 4, hipMemcpyDeviceToHost));
  if (triangle_component && c->mslab.nt) HIP_TRY(c, hipMemcpy(triangle_component, K.triangle, (size_t)c->mslab.nt * 4, hipMemcpyDeviceToHost));
  if (table && K.n_owned) HIP_TRY(c, hipMemcpy(table, K.table, (size_t)K.n_owned * sizeof(*table), hipMemcpyDeviceToHost));
  return TSDF_OK;
}
int32_t tsdf_mesh_slab_component_stats(tsdf_ctx* c, uint64_t out[4]) {
  CHECK_CTX(c);
  if (!out) return TSDF_ERR_INVALID_ARGUMENT;
  if (!c->mslab.valid) FAIL(c, TSDF_ERR_STATE, "no slab mesh (tsdf_mesh_slab_extract)");
  const tsdf_ctx::MeshSlabComponents& K = c->mslabc;
  out[0] = K.n_local; out[1] = K.n_owned; out[2] = K.n_down + K.n_up; out[3] = K.removed;
  return TSDF_OK;
}

// ---- mesh components (k_mesh_components.hip; the definition is in the header): labels and table of the current mesh, and the mesh without some of them
namespace {
struct ComponentTemp {                                                    // what one call allocates besides what it leaves in the context: freed when it returns
  uint32_t* words = nullptr; unsigned long long* vsums = nullptr; unsigned long long* tsums = nullptr; uint32_t* largest = nullptr; uint8_t* keep = nullptr;
  tsdf_ctx::MeshComponents made{}; MeshArrays mesh{};                     // arrays not handed to the context yet
  tsdf_mesh_component_measure* rows = nullptr; unsigned long long* packed = nullptr;   // ... and measures not handed over yet
  ~ComponentTemp() {
    hipFree(words); hipFree(vsums); hipFree(tsums); hipFree(largest); hipFree(keep); hipFree(rows); hipFree(packed);
    hipFree(made.vertex); hipFree(made.triangle); hipFree(made.table);
    mesh_store_free(mesh);
  }
};
bool device_alloc(void** p, size_t bytes) { return hipMalloc(p, std::max<size_t>(bytes, 4)) == hipSuccess; }
}  // namespace
int32_t tsdf_mesh_components(tsdf_ctx* c, uint64_t* n_components) {
  CHECK_CTX(c);
  if (!c->mesh.valid) FAIL(c, TSDF_ERR_STATE, "no mesh (tsdf_mesh_extract / tsdf_mesh_extract_lod)");
  HIP_TRY(c, hipSetDevice(c->device));
  const tsdf_ctx::Mesh& M = c->mesh;
  if (M.nt > 0xffffffffull) FAIL(c, TSDF_ERR_OUT_OF_MEMORY, "%llu triangles do not fit a component's 32-bit count", (unsigned long long)M.nt);
  const uint32_t nv = (uint32_t)M.nv;
  const size_t nt = (size_t)M.nt;
  const int nb = mesh_cc_scan_blocks(nv);
  ComponentTemp tmp;
  tsdf_ctx::MeshComponents& K = tmp.made;
  bool ok = device_alloc((void**)&tmp.words, (size_t)nv * 4) && device_alloc((void**)&tmp.vsums, (size_t)(nb + 1) * 8) && device_alloc((void**)&tmp.largest, 4) &&
            device_alloc((void**)&K.vertex, (size_t)nv * 4) && device_alloc((void**)&K.triangle, nt * 4);
  if (!ok) { (void)hipGetLastError(); FAIL(c, TSDF_ERR_OUT_OF_MEMORY, "no device memory for the components of %u vertices and %zu triangles", nv, nt); }
  unsigned long long n = 0;
  uint32_t largest = 0;
  timer_begin(c, "mesh_components");
  launch_mesh_cc_label(c->stream, M.tri, nv, nt, tmp.words, K.vertex, tmp.vsums);
  timer_end(c, "mesh_components");
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(&n, tmp.vsums + nb, sizeof(n), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, sync_ctx(c));                                               // (the table is sized exactly: the host has to know C)
  if (!device_alloc((void**)&K.table, (size_t)n * sizeof(tsdf_mesh_component))) {
    (void)hipGetLastError();
    FAIL(c, TSDF_ERR_OUT_OF_MEMORY, "no device memory for a table of %llu components", n);
  }
  HIP_TRY(c, hipMemsetAsync(tmp.largest, 0, 4, c->stream));
  timer_begin(c, "mesh_components");                                     // (a second sample of the same call: the host's allocation lies between the two)
  launch_mesh_cc_number(c->stream, M.tri, nv, nt, tmp.vsums, (uint32_t)n, tmp.words, K.vertex, K.triangle, K.table, tmp.largest);
  timer_end(c, "mesh_components");
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(&largest, tmp.largest, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, sync_ctx(c));
  release_mesh_components(c);                                            // (an earlier labelling of the same mesh: the same words)
  tsdf_ctx::MeshComponents& X = c->mcomp;
  X.vertex = K.vertex; X.triangle = K.triangle; X.table = K.table; X.n = n; X.largest = largest; X.valid = true;
  K = tsdf_ctx::MeshComponents{};
  if (n_components) *n_components = n;
  return TSDF_OK;
}
static int32_t mesh_components_check(tsdf_ctx* c) {
  if (!c->mesh.valid) FAIL(c, TSDF_ERR_STATE, "no mesh (tsdf_mesh_extract / tsdf_mesh_extract_lod)");
  if (!c->mcomp.valid) FAIL(c, TSDF_ERR_STATE, "no components of the current mesh (tsdf_mesh_components after the extract, and again after a keep / filter)");
  return TSDF_OK;
}
int32_t tsdf_mesh_download_components(tsdf_ctx* c, uint32_t* vertex_component, uint32_t* triangle_component, tsdf_mesh_component* table) {
  CHECK_CTX(c);
  int32_t rc = mesh_components_check(c);
  if (rc) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  const tsdf_ctx::MeshComponents& K = c->mcomp;
  if (vertex_component && c->mesh.nv) HIP_TRY(c, hipMemcpy(vertex_component, K.vertex, (size_t)c->mesh.nv * 4, hipMemcpyDeviceToHost));
  if (triangle_component && c->mesh.nt) HIP_TRY(c, hipMemcpy(triangle_component, K.triangle, (size_t)c->mesh.nt * 4, hipMemcpyDeviceToHost));
  if (table && K.n) HIP_TRY(c, hipMemcpy(table, K.table, (size_t)K.n * sizeof(tsdf_mesh_component), hipMemcpyDeviceToHost));
  return TSDF_OK;
}
// keep_host: C bytes, or null = derive the flags on the device: from the table (n_triangles >= min_triangles), with a rule from the measures
static int32_t mesh_keep(tsdf_ctx* c, const uint8_t* keep_host, uint32_t min_triangles, uint64_t* n_vertices, uint64_t* n_triangles,
                         const tsdf_mesh_measure_rule* rule = nullptr) {
  int32_t rc = mesh_components_check(c);
  if (rc) return rc;
  if (rule && !c->mcomp.measured) FAIL(c, TSDF_ERR_STATE, "no measures of the current mesh's components (tsdf_mesh_component_measures after tsdf_mesh_components)");
  HIP_TRY(c, hipSetDevice(c->device));
  tsdf_ctx::Mesh& M = c->mesh;
  tsdf_ctx::MeshComponents& K = c->mcomp;
  const uint32_t nv = (uint32_t)M.nv, nc = (uint32_t)K.n;
  const size_t nt = (size_t)M.nt;
  const int nbv = mesh_cc_scan_blocks(nv), nbt = mesh_cc_scan_blocks(nt);
  ComponentTemp tmp;
  bool ok = device_alloc((void**)&tmp.keep, nc) && device_alloc((void**)&tmp.vsums, (size_t)(nbv + 1) * 8) && device_alloc((void**)&tmp.tsums, (size_t)(nbt + 1) * 8) &&
            device_alloc((void**)&tmp.words, (size_t)nv * 4);
  if (!ok) { (void)hipGetLastError(); FAIL(c, TSDF_ERR_OUT_OF_MEMORY, "no device memory to filter a mesh of %u vertices and %zu triangles", nv, nt); }
  unsigned long long kept_v = 0, kept_t = 0;
  if (keep_host && nc) HIP_TRY(c, hipMemcpyAsync(tmp.keep, keep_host, nc, hipMemcpyHostToDevice, c->stream));
  timer_begin(c, "mesh_filter");
  if (rule) launch_mesh_measure_keep(c->stream, K.measure, K.table, nc, *rule, tmp.keep);
  else if (!keep_host) launch_mesh_cc_keep_from_table(c->stream, K.table, nc, min_triangles, tmp.keep);
  launch_mesh_cc_keep_count(c->stream, tmp.keep, K.vertex, K.triangle, nv, nt, tmp.vsums, tmp.tsums);
  timer_end(c, "mesh_filter");
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(&kept_v, tmp.vsums + nbv, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(&kept_t, tmp.tsums + nbt, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, sync_ctx(c));                                               // (the new arrays are sized exactly; keep_host has been read)
  if (kept_v != M.nv) {                                                  // (every vertex has a component: all vertices kept = every component kept = the mesh as it is)
    MeshArrays& N = tmp.mesh;                                            // everything new is allocated before anything is replaced
    ok = !kept_v || mesh_store_allocate(N, kept_v, kept_t, M.flags);
    if (!ok) { (void)hipGetLastError(); FAIL(c, TSDF_ERR_OUT_OF_MEMORY, "no device memory for a filtered mesh of %llu vertices and %llu triangles", kept_v, kept_t); }
    if (kept_v) {
      timer_begin(c, "mesh_filter");
      launch_mesh_cc_keep_scatter(c->stream, tmp.keep, K.vertex, K.triangle, nv, nt, tmp.vsums, tmp.tsums, M, N, tmp.words);
      timer_end(c, "mesh_filter");
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, sync_ctx(c));
    }
    std::swap<MeshArrays>(M, N);                                         // (tmp frees the old arrays)
  }
  K.removed_vertices = M.nv - kept_v; K.removed_triangles = M.nt - kept_t;
  M.nv = kept_v; M.nt = kept_t;
  M.stats[3] = mesh_store_bytes(M);
  release_mesh_components(c);                                            // (they labelled the mesh that was)
  release_mesh_texture_taps(c);
  if (n_vertices) *n_vertices = M.nv;
  if (n_triangles) *n_triangles = M.nt;
  return TSDF_OK;
}
int32_t tsdf_mesh_keep_components(tsdf_ctx* c, const uint8_t* keep, uint64_t* n_vertices, uint64_t* n_triangles) {
  CHECK_CTX(c);
  if (!keep) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "null keep");
  return mesh_keep(c, keep, 0u, n_vertices, n_triangles);
}
int32_t tsdf_mesh_filter_components(tsdf_ctx* c, uint32_t min_triangles, uint64_t* n_vertices, uint64_t* n_triangles) {
  CHECK_CTX(c);
  return mesh_keep(c, nullptr, min_triangles, n_vertices, n_triangles);
}
// ---- mesh component measures (k_mesh_component_measures.hip, mesh_measure.hpp; the definition is in the header)
static int32_t mesh_measure_grid(tsdf_ctx* c, MeasureScale* S, tsdf_mesh_measure_grid* grid) {
  if (!measure_scale(c->cfg.bbox_min, c->cfg.bbox_max, S)) FAIL(c, TSDF_ERR_STATE, "the box has no positive finite extent: no measure grid");
  if (grid) *grid = tsdf_mesh_measure_grid{S->unit, {S->bbox_min[0], S->bbox_min[1], S->bbox_min[2]}, kMeasureBits};
  return TSDF_OK;
}
int32_t tsdf_mesh_measure_grid_info(tsdf_ctx* c, tsdf_mesh_measure_grid* grid) {
  CHECK_CTX(c);
  if (!grid) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "null grid");
  MeasureScale S;
  return mesh_measure_grid(c, &S, grid);
}
int32_t tsdf_mesh_component_measures(tsdf_ctx* c, tsdf_mesh_measure_grid* grid) {
  CHECK_CTX(c);
  int32_t rc = mesh_components_check(c);
  if (rc) return rc;
  MeasureScale S;
  if ((rc = mesh_measure_grid(c, &S, nullptr))) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  const tsdf_ctx::Mesh& M = c->mesh;
  tsdf_ctx::MeshComponents& K = c->mcomp;
  const uint32_t nv = (uint32_t)M.nv, nc = (uint32_t)K.n;
  ComponentTemp tmp;                                                       // everything new is allocated before anything is replaced
  if (!device_alloc((void**)&tmp.rows, (size_t)nc * sizeof(tsdf_mesh_component_measure)) || !device_alloc((void**)&tmp.packed, (size_t)nv * 8)) {
    (void)hipGetLastError();
    FAIL(c, TSDF_ERR_OUT_OF_MEMORY, "no device memory for the measures of %u components and %u vertices", nc, nv);
  }
  if (nc) {                                                                // (the empty mesh has no component: nothing to launch)
    timer_begin(c, "mesh_component_measures");                             // (the fill is part of the scheme: zero is every field's identity)
    const hipError_t filled = hipMemsetAsync(tmp.rows, 0, (size_t)nc * sizeof(tsdf_mesh_component_measure), c->stream);
    if (filled != hipSuccess) { timer_end(c, "mesh_component_measures"); HIP_TRY(c, filled); }
    launch_mesh_measures(c->stream, MeshMeasureGeometry{{S.bbox_min[0], S.bbox_min[1], S.bbox_min[2]}, S.scale}, M.pos, M.tri, nv, (size_t)M.nt, K.vertex, K.triangle, nc,
                         tmp.packed, tmp.rows);
    timer_end(c, "mesh_component_measures");
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, sync_ctx(c));
  hipFree(K.measure); hipFree(K.packed);                                   // (an earlier call's: the same words)
  K.measure = tmp.rows; K.packed = tmp.packed; K.measured = true;
  tmp.rows = nullptr; tmp.packed = nullptr;
  return mesh_measure_grid(c, &S, grid);
}
int32_t tsdf_mesh_download_component_measures(tsdf_ctx* c, tsdf_mesh_component_measure* rows) {
  CHECK_CTX(c);
  if (!rows) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "null rows");
  int32_t rc = mesh_components_check(c);
  if (rc) return rc;
  const tsdf_ctx::MeshComponents& K = c->mcomp;
  if (!K.measured) FAIL(c, TSDF_ERR_STATE, "no measures of the current mesh's components (tsdf_mesh_component_measures after tsdf_mesh_components)");
  HIP_TRY(c, hipSetDevice(c->device));
  if (K.n) HIP_TRY(c, hipMemcpy(rows, K.measure, (size_t)K.n * sizeof(tsdf_mesh_component_measure), hipMemcpyDeviceToHost));
  return TSDF_OK;
}
int32_t tsdf_mesh_filter_components_measured(tsdf_ctx* c, const tsdf_mesh_measure_rule* rule, uint64_t* n_vertices, uint64_t* n_triangles) {
  CHECK_CTX(c);
  if (!rule) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "null rule");
  if (rule->reserved != 0u || (rule->flags & ~TSDF_MESH_RULE_POSITIVE_VOLUME))
    FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "rule.reserved = %u and flags = 0x%x: reserved has to be 0, the one flag is TSDF_MESH_RULE_POSITIVE_VOLUME", rule->reserved, rule->flags);
  return mesh_keep(c, nullptr, 0u, n_vertices, n_triangles, rule);
}
int32_t tsdf_mesh_component_stats(tsdf_ctx* c, uint64_t out[4]) {
  CHECK_CTX(c);
  if (!out) return TSDF_ERR_INVALID_ARGUMENT;
  if (!c->mesh.valid) FAIL(c, TSDF_ERR_STATE, "no mesh (tsdf_mesh_extract / tsdf_mesh_extract_lod)");
  const tsdf_ctx::MeshComponents& K = c->mcomp;
  out[0] = K.n; out[1] = K.largest; out[2] = K.removed_vertices; out[3] = K.removed_triangles;
  return TSDF_OK;
}

// ---- mesh streaming (the definition is in the header): the same mesh every frame, packed, without a host wait or an allocation after the first call
static size_t mesh_stream_payload_capacity(const tsdf_ctx::MeshStream& R) { return (size_t)R.layout().payload_capacity(R.max_vertices, R.max_triangles, R.max_tiles); }
static size_t mesh_stream_tap_offset(const tsdf_ctx::MeshStream& R) { return (size_t)R.layout().tap_offset(R.max_vertices, R.max_triangles, R.max_tiles); }
int32_t tsdf_mesh_stream_config(tsdf_ctx* c, uint32_t flags, uint32_t max_vertices, uint32_t max_triangles, uint32_t max_surface_tiles, uint32_t slots) {
  return tsdf_mesh_stream_config_lod(c, flags, 0u, max_vertices, max_triangles, max_surface_tiles, slots);
}
int32_t tsdf_mesh_stream_config_lod(tsdf_ctx* c, uint32_t flags, uint32_t level, uint32_t max_vertices, uint32_t max_triangles, uint32_t max_surface_tiles, uint32_t slots) {
  return tsdf_mesh_stream_config_filter(c, flags, level, 0u, max_vertices, max_triangles, max_surface_tiles, slots);
}
int32_t tsdf_mesh_stream_config_filter(tsdf_ctx* c, uint32_t flags, uint32_t level, uint32_t min_triangles, uint32_t max_vertices, uint32_t max_triangles,
                                       uint32_t max_surface_tiles, uint32_t slots) {
  return tsdf_mesh_stream_config_compact(c, flags, level, min_triangles, TSDF_MESH_INDEX_U32, max_vertices, max_triangles, max_surface_tiles, slots);
}
// every config entry ends here.  part: tsdf_mesh_stream_config_part (the frames are this context's part of the tile-local frame)
static int32_t mesh_stream_configure(tsdf_ctx* c, uint32_t flags, uint32_t level, uint32_t min_triangles, uint32_t index_format, uint32_t max_vertices,
                                     uint32_t max_triangles, uint32_t max_surface_tiles, uint32_t slots, bool part) {
  tsdf_ctx::MeshStream& R = c->mstream;
  if (index_format > TSDF_MESH_INDEX_TILE16) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "mesh index format %u (0: uint32 indices, 1: tile-local 16-bit codes)", index_format);
  if (int32_t rc = mesh_flags_level_check(c, flags, level, false)) return rc;
  if ((flags & ~(TSDF_MESH_NORMALS | TSDF_MESH_COLOURS)) || !max_vertices || !max_triangles || !max_surface_tiles || slots < 2 || slots > kMaxResultSlots)
    FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "mesh stream flags %u / capacities %u vertices, %u triangles, %u tiles / slots %u (flags 1 normals, 2 colours; capacities > 0; 2..%u slots)",
         flags, max_vertices, max_triangles, max_surface_tiles, slots, kMaxResultSlots);
  if (!MeshFrameLayout{index_format, flags ? 16u : 8u}.fits(max_vertices, max_triangles, max_surface_tiles)) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "a mesh stream slot of more than 4 GiB");
  MeshPartLayers layers;
  if (part) if (int32_t rc = mesh_part_layers(c, level, &layers)) return rc;   // the alignment rule of tsdf_mesh_slab_extract, here at config time
  if (!R.ring.idle()) FAIL(c, TSDF_ERR_STATE, "%u streamed mesh frame(s) are queued or held: acquire and release them first", R.ring.count);
  HIP_TRY(c, hipSetDevice(c->device));
  // The ring is idle for the copies only (each was waited for before its frame was released): a frame that overflowed or had no payload was handed out
  // behind its header copy alone, and its emit launches, which read the slot's device header and the scratch, may still be queued on the context's stream.
  if (R.allocated) HIP_TRY(c, hipStreamSynchronize(c->stream));
  release_mesh_stream(c);
  R.flags = flags; R.level = level; R.max_vertices = max_vertices; R.max_triangles = max_triangles; R.max_tiles = max_surface_tiles; R.min_triangles = min_triangles; R.index_format = index_format; R.part = part; R.ring.configure(slots); R.configured = true;
  R.tap_flags = 0;                                                       // (every config entry means what it meant: tsdf_mesh_stream_config_taps amends it)
  R.frames = R.overflowed = R.bytes_copied = 0;
  return TSDF_OK;
}
int32_t tsdf_mesh_stream_config_compact(tsdf_ctx* c, uint32_t flags, uint32_t level, uint32_t min_triangles, uint32_t index_format, uint32_t max_vertices,
                                        uint32_t max_triangles, uint32_t max_surface_tiles, uint32_t slots) {
  CHECK_CTX(c);
  return mesh_stream_configure(c, flags, level, min_triangles, index_format, max_vertices, max_triangles, max_surface_tiles, slots, false);
}
int32_t tsdf_mesh_stream_config_part(tsdf_ctx* c, uint32_t flags, uint32_t level, uint32_t max_vertices, uint32_t max_triangles, uint32_t max_surface_tiles, uint32_t slots) {
  CHECK_CTX(c);
  return mesh_stream_configure(c, flags, level, 0u, TSDF_MESH_INDEX_TILE16, max_vertices, max_triangles, max_surface_tiles, slots, true);
}
int32_t tsdf_mesh_stream_level(tsdf_ctx* c, uint32_t* level) {
  CHECK_CTX(c);
  if (!level) return TSDF_ERR_INVALID_ARGUMENT;
  if (!c->mstream.configured) FAIL(c, TSDF_ERR_STATE, "tsdf_mesh_stream_level before tsdf_mesh_stream_config");
  *level = c->mstream.level;
  return TSDF_OK;
}
int32_t tsdf_mesh_stream_min_triangles(tsdf_ctx* c, uint32_t* min_triangles) {
  CHECK_CTX(c);
  if (!min_triangles) return TSDF_ERR_INVALID_ARGUMENT;
  if (!c->mstream.configured) FAIL(c, TSDF_ERR_STATE, "tsdf_mesh_stream_min_triangles before tsdf_mesh_stream_config");
  *min_triangles = c->mstream.min_triangles;
  return TSDF_OK;
}
int32_t tsdf_mesh_stream_index_format(tsdf_ctx* c, uint32_t* index_format) {
  CHECK_CTX(c);
  if (!index_format) return TSDF_ERR_INVALID_ARGUMENT;
  if (!c->mstream.configured) FAIL(c, TSDF_ERR_STATE, "tsdf_mesh_stream_index_format before tsdf_mesh_stream_config");
  *index_format = c->mstream.index_format;
  return TSDF_OK;
}
// "mesh streaming: texture taps in the frame": amends the current configuration; a change drops the slots as a config does (they are sized with the block)
int32_t tsdf_mesh_stream_config_taps(tsdf_ctx* c, uint32_t tap_flags) {
  CHECK_CTX(c);
  tsdf_ctx::MeshStream& R = c->mstream;
  if (!R.configured) FAIL(c, TSDF_ERR_STATE, "tsdf_mesh_stream_config_taps before tsdf_mesh_stream_config");
  if (tap_flags & ~kMeshStreamTaps) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "mesh stream tap flags %u (1: packed texture taps behind every frame)", tap_flags);
  if (!R.ring.idle()) FAIL(c, TSDF_ERR_STATE, "%u streamed mesh frame(s) are queued or held: acquire and release them first", R.ring.count);
  if (tap_flags && !R.layout().fits_taps(R.max_vertices, R.max_triangles, R.max_tiles, c->cfg.num_streams))
    FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "a mesh stream slot of more than 4 GiB with the taps of %u vertices and %u streams", R.max_vertices, c->cfg.num_streams);
  if (tap_flags == R.tap_flags) return TSDF_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  if (R.allocated) HIP_TRY(c, hipStreamSynchronize(c->stream));         // (as a config: launches of frames without payload may still be queued)
  release_mesh_stream(c);
  R.tap_flags = tap_flags;
  return TSDF_OK;
}
int32_t tsdf_mesh_stream_tap_flags(tsdf_ctx* c, uint32_t* tap_flags) {
  CHECK_CTX(c);
  if (!tap_flags) return TSDF_ERR_INVALID_ARGUMENT;
  if (!c->mstream.configured) FAIL(c, TSDF_ERR_STATE, "tsdf_mesh_stream_tap_flags before tsdf_mesh_stream_config");
  *tap_flags = c->mstream.tap_flags;
  return TSDF_OK;
}
// the filter's raw buffer and scratch (min_triangles >= 1): sized by the capacities, like everything the filter launches
static bool mesh_stream_filter_allocate(tsdf_ctx::MeshStream& R, const int c_res[3], uint64_t* bytes) {
  MeshStreamFilter& F = R.filter;
  F.max_vertices = R.max_vertices; F.max_triangles = R.max_triangles; F.min_triangles = R.min_triangles; F.stride = R.flags ? 16u : 8u;
  const size_t nv = R.max_vertices;
  // the raw frame is the uint32 one in either format; the tile-local format keeps the raw tile table behind it, at a multiple of 16 bytes
  const bool compact = R.index_format == kMeshIndexTile16;
  const size_t raw_payload = (size_t)MeshFrameLayout{kMeshIndexU32, F.stride}.payload_capacity(R.max_vertices, R.max_triangles, R.max_tiles);
  const size_t raw_frame = sizeof(MeshStreamHeader) + (compact ? (size_t)MeshFrameLayout::align16(raw_payload) : raw_payload);
  if (compact) {
    const MeshLattice L = mesh_lattice(c_res, (int)R.level);
    F.ntx = L.ntx; F.nty = L.nty;
    const size_t local_bytes = ((size_t)R.max_triangles + 3) / 4 * sizeof(uint16_t);
    if (hipMalloc((void**)&F.tri_local, local_bytes) != hipSuccess) return false;
    *bytes += local_bytes;
  }
  const struct { void** p; size_t bytes; } arrays[8] = {
    {(void**)&F.raw, raw_frame + (compact ? (size_t)R.max_tiles * sizeof(MeshTileRow) : 0)}, {(void**)&F.parent, nv * sizeof(uint32_t)}, {(void**)&F.label, nv * sizeof(uint32_t)},
    {(void**)&F.count, nv * sizeof(uint32_t)}, {(void**)&F.keep, (nv + 3) / 4 * 4}, {(void**)&F.vertex_sums, mesh_stream_filter_scan_words(R.max_vertices) * sizeof(uint64_t)},
    {(void**)&F.triangle_sums, mesh_stream_filter_scan_words(R.max_triangles) * sizeof(uint64_t)}, {(void**)&F.words, 3 * sizeof(uint32_t)}};
  for (const auto& A : arrays) { if (hipMalloc(A.p, A.bytes) != hipSuccess) return false; *bytes += A.bytes; }
  if (compact) F.raw_table = (MeshTileRow*)((uint8_t*)F.raw + raw_frame);
  return true;
}
// slots and scratch, once per configuration and grid
static int32_t mesh_stream_allocate(tsdf_ctx* c) {
  tsdf_ctx::MeshStream& R = c->mstream;
  const MeshLattice L = mesh_lattice(c->vol.res, (int)R.level);
  size_t n_tiles = (size_t)L.ntx * L.nty * L.ntz, record_slots = R.max_tiles;
  if (R.part) {                                                          // the scratch over owned + seam tiles, records for the seam tiles beyond the capacity
    MeshPartLayers P;
    if (int32_t rc = mesh_part_layers(c, R.level, &P)) return rc;
    const size_t per_layer = (size_t)L.ntx * L.nty;
    R.slab = MeshSlab{P.layer0, (int)((size_t)(P.layer1 - P.layer0) * per_layer), (int)P.seam_tiles(per_layer)};
    n_tiles = (size_t)R.slab.n_own + (size_t)R.slab.n_seam;
    record_slots = (size_t)P.record_slots(R.max_tiles, per_layer);
  }
  const size_t lead = R.min_triangles ? sizeof(MeshStreamFilterRecord) : R.part ? sizeof(MeshStreamPartRecord) : 0,
               // with taps a slot ends with their block (the filter's raw buffer needs none: taps are taken from the slot, after the scatter)
               slot_bytes = lead + (R.tap_flags ? (size_t)R.layout().slot_bytes_taps(R.max_vertices, R.max_triangles, R.max_tiles, c->cfg.num_streams)
                                                : sizeof(MeshStreamHeader) + mesh_stream_payload_capacity(R)),
               record_bytes = record_slots * 512 * sizeof(uint32_t);
  uint64_t bytes = (uint64_t)R.ring.slots * slot_bytes + record_bytes;
  bool ok = mesh_scratch_allocate(R.scratch, (int)n_tiles, (int)R.level, &bytes) == hipSuccess && hipMalloc((void**)&R.records, record_bytes) == hipSuccess;
  if (ok && R.min_triangles) ok = mesh_stream_filter_allocate(R, c->vol.res, &bytes);
  for (uint32_t k = 0; ok && k < R.ring.slots; ++k) {
    tsdf_ctx::MeshStreamSlot& S = R.slot[k];
    ok = hipMalloc((void**)&S.dev, slot_bytes) == hipSuccess;
    if (ok) { S.dev += lead; S.lead = lead; }                          // (release_mesh_stream frees dev - lead: a failed host allocation below must find it so)
    ok = ok && hipHostMalloc((void**)&S.host, slot_bytes, hipHostMallocDefault) == hipSuccess;
    if (ok) S.host += lead;
    for (hipEvent_t* e : {&S.header_written, &S.emitted, &S.header_ready, &S.ready}) ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    if (R.tap_flags) ok = ok && hipEventCreateWithFlags(&S.taps_written, hipEventDisableTiming) == hipSuccess;
  }
  if (ok) ok = ensure_copy_stream(c) == TSDF_OK;
  if (!ok) { (void)hipGetLastError(); release_mesh_stream(c); FAIL(c, TSDF_ERR_OUT_OF_MEMORY, "no memory for %u mesh stream slots of %zu bytes and the scratch of %zu tiles", R.ring.slots, slot_bytes, n_tiles); }
  R.device_bytes = bytes;
  R.allocated = true;
  return TSDF_OK;
}
// Queue the payload copy of every queued frame whose header has arrived on the host, oldest first (the copy stream is in order: behind a header still
// travelling nothing has arrived either).  Host side this is event queries only.
static int32_t mesh_stream_pump(tsdf_ctx* c) {
  tsdf_ctx::MeshStream& R = c->mstream;
  for (uint32_t k = 0; k < R.ring.count; ++k) {
    tsdf_ctx::MeshStreamSlot& S = R.slot[R.ring.queued(k)];
    if (S.payload_issued) continue;
    bool arrived;
    if (int32_t rc = event_reached(c, S.header_ready, false, &arrived)) return rc;
    if (!arrived) break;                                                 // (behind a header still travelling nothing has arrived either)
    const MeshStreamHeader* H = (const MeshStreamHeader*)S.host;
    S.table_rows = 0;
    if (R.index_format == kMeshIndexTile16 && H->n_vertices)               // (an overflowed or emptied frame has no row)
      S.table_rows = R.min_triangles ? ((const MeshStreamFilterRecord*)(S.host - S.lead))->table_rows : H->needed_tiles;
    S.payload_bytes = (size_t)R.layout().payload_bytes(H->n_vertices, H->n_triangles, S.table_rows);
    S.tap_bytes = R.tap_flags ? (size_t)MeshFrameLayout::tap_bytes(H->n_vertices, c->cfg.num_streams) : 0;   // (no vertex: no payload and no tap)
    if (S.payload_bytes) {
      HIP_TRY(c, hipStreamWaitEvent(c->copy_stream, S.emitted, 0));
      HIP_TRY(c, hipMemcpyAsync(S.host + sizeof(MeshStreamHeader), S.dev + sizeof(MeshStreamHeader), S.payload_bytes, hipMemcpyDeviceToHost, c->copy_stream));
      if (S.tap_bytes) {                                                 // the tap block: a copy of its own, of exactly the frame's bytes, from its fixed place
        const size_t at = sizeof(MeshStreamHeader) + mesh_stream_tap_offset(R);
        HIP_TRY(c, hipStreamWaitEvent(c->copy_stream, S.taps_written, 0));
        HIP_TRY(c, hipMemcpyAsync(S.host + at, S.dev + at, S.tap_bytes, hipMemcpyDeviceToHost, c->copy_stream));
      }
      HIP_TRY(c, hipEventRecord(S.ready, c->copy_stream));
    }
    S.payload_issued = true;                                             // (the counters move with it: a call that failed above repeats the slot without counting it twice)
    if (H->overflow) ++R.overflowed;
    R.bytes_copied += S.payload_bytes + S.tap_bytes;
  }
  return TSDF_OK;
}
// The packed taps of the frame in slot S ("mesh streaming: texture taps in the frame"): one launch behind the last launch that writes the slot's packed
// vertices and behind the header that holds the final n_vertices, which the kernel reads on the device.  It reads LUTs and the current frame slot's
// images (join_pre was taken with the frame's first launch), no volume.  The upload that overwrites that frame slot two frames later waits for the lane
// ahead's gate, which the context's stream records behind this launch; draw_done[set] is recorded again behind it, as tsdf_texture_taps_dev does.
static int32_t mesh_stream_queue_taps(tsdf_ctx* c, tsdf_ctx::MeshStreamSlot& S) {
  const tsdf_ctx::MeshStream& R = c->mstream;
  timer_begin(c, "mesh_stream_taps");
  launch_mesh_stream_taps(c->stream, c->luts, c->frame, c->vol.limit, (const MeshStreamHeader*)S.dev, S.dev + sizeof(MeshStreamHeader), R.flags ? 16u : 8u, R.max_vertices,
                          S.dev + sizeof(MeshStreamHeader) + mesh_stream_tap_offset(R));
  timer_end(c, "mesh_stream_taps");
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipEventRecord(S.taps_written, c->stream));
  return overlay_rerecord_draw(c);
}
// A filtered frame behind its raw header: emit into the raw buffer, the filter into the slot, the slot's final header, and only then the header's copy.
// draw_done is recorded again right behind the emit: the filter reads no volume, a later integrate() does not wait for it.
static int32_t mesh_stream_filtered_tail(tsdf_ctx* c, tsdf_ctx::MeshStreamSlot& S) {
  tsdf_ctx::MeshStream& R = c->mstream;
  const MeshStreamFilter& F = R.filter;
  timer_begin(c, "mesh_stream_emit");
  if (F.raw_table) launch_mesh_stream_emit_compact(c->stream, c->vol, c->luts, c->frame, mesh_geometry(c), R.scratch, R.flags, F.raw, R.records, F.raw + 1, F.raw_table);
  else launch_mesh_stream_emit(c->stream, c->vol, c->luts, c->frame, mesh_geometry(c), R.scratch, R.flags, F.raw, R.records, F.raw + 1);
  timer_end(c, "mesh_stream_emit");
  HIP_TRY(c, hipGetLastError());
  if (int32_t rc = overlay_rerecord_draw(c)) return rc;
  timer_begin(c, "mesh_stream_filter");
  launch_mesh_stream_filter(c->stream, F, S.dev + sizeof(MeshStreamHeader));
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipEventRecord(S.emitted, c->stream));
  launch_mesh_stream_filter_header(c->stream, F, (MeshStreamHeader*)S.dev, (MeshStreamFilterRecord*)(S.dev - S.lead));
  timer_end(c, "mesh_stream_filter");
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipEventRecord(S.header_written, c->stream));
  HIP_TRY(c, hipStreamWaitEvent(c->copy_stream, S.header_written, 0));
  HIP_TRY(c, hipMemcpyAsync(S.host - S.lead, S.dev - S.lead, S.lead + sizeof(MeshStreamHeader), hipMemcpyDeviceToHost, c->copy_stream));
  HIP_TRY(c, hipEventRecord(S.header_ready, c->copy_stream));
  if (R.tap_flags) if (int32_t rc = mesh_stream_queue_taps(c, S)) return rc;   // behind the final header; the header's copy does not wait for it
  ++R.frames;
  return TSDF_OK;
}
int32_t tsdf_mesh_stream(tsdf_ctx* c, uint64_t tag) {
  CHECK_CTX(c);
  tsdf_ctx::MeshStream& R = c->mstream;
  if (!R.configured) FAIL(c, TSDF_ERR_STATE, "tsdf_mesh_stream before tsdf_mesh_stream_config");
  int32_t rc;
  if (!R.part) {
    if ((rc = readable_volume_check(c, "tsdf_mesh_stream on a Z-slab context: slab parts (tsdf_mesh_slab_extract) are not streamed", (R.flags & TSDF_MESH_COLOURS) != 0))) return rc;
  } else {                                                               // a part ring: any context; the halo is the caller's to keep current, that it exists is checked
    if (!c->have_volume) FAIL(c, TSDF_ERR_STATE, "no volume yet (tsdf_integrate or tsdf_upload_volume)");
    if ((R.flags & TSDF_MESH_COLOURS) && (rc = require_inputs(c, false, true))) return rc;
    if (c->vol.own_tz1 != (c->res[2] + 7) / 8 && c->vol.tz1 - c->vol.own_tz1 < 1) FAIL(c, TSDF_ERR_STATE, "the slab stores no halo layer above its planes");
  }
  if (R.tap_flags && (rc = require_inputs(c, false, true))) return rc;   // taps: calibration (cv_xyz_inv, cv_uv) and a frame, whatever the vertex flags
  if (R.ring.full()) FAIL(c, TSDF_ERR_STATE, "all %u mesh stream slots are queued or held (tsdf_mesh_stream_acquire / tsdf_mesh_stream_release)", R.ring.slots);
  HIP_TRY(c, hipSetDevice(c->device));
  if (!R.allocated && (rc = mesh_stream_allocate(c))) return rc;
  if ((rc = mesh_stream_pump(c))) return rc;
  tsdf_ctx::MeshStreamSlot& S = R.slot[R.ring.push()];                   // (queued before its calls are: result_paths.hpp's transitions precede what acts on them)
  S.tag = tag; S.payload_issued = false; S.payload_bytes = 0; S.table_rows = 0; S.tap_bytes = 0;
  for (int a = 0; a < 3; ++a) S.res[a] = c->res[a];
  const bool filtered = R.min_triangles != 0;
  MeshStreamHeader* H = filtered ? R.filter.raw : (MeshStreamHeader*)S.dev;   // with a filter: count, scan, header and emit write the raw buffer, not the slot
  const Volume& V = c->vol;
  const MeshLattice L = mesh_lattice(V.res, (int)R.level);
  const bool cells = L.cr[0] >= 2 && L.cr[1] >= 2 && L.cr[2] >= 2;       // (a lattice one point thick has no cell)
  if (cells) {
    HIP_TRY(c, join_integ(c));                                           // the volume tsdf_download_volume would return now
    if ((R.flags & TSDF_MESH_COLOURS) || R.tap_flags) HIP_TRY(c, join_pre(c));   // ... and the current frame slot's images
    timer_begin(c, "mesh_stream_count");
    if (R.part) launch_mesh_slab_count(c->stream, V, R.scratch, R.slab); else launch_mesh_count(c->stream, V, R.scratch);
    timer_end(c, "mesh_stream_count");
    timer_begin(c, "mesh_stream_scan");
    launch_mesh_scan(c->stream, R.scratch);
    if (R.part) launch_mesh_part_header(c->stream, R.scratch, R.slab, (MeshStreamPartRecord*)(S.dev - S.lead), H, R.max_vertices, R.max_triangles, R.max_tiles);
    else launch_mesh_stream_header(c->stream, R.scratch, H, R.max_vertices, R.max_triangles, R.max_tiles);
    timer_end(c, "mesh_stream_scan");
  } else HIP_TRY(c, hipMemsetAsync(S.dev - S.lead, 0, S.lead + sizeof(MeshStreamHeader), c->stream));
  HIP_TRY(c, hipGetLastError());
  if (filtered && cells) return mesh_stream_filtered_tail(c, S);
  HIP_TRY(c, hipEventRecord(S.header_written, c->stream));
  HIP_TRY(c, hipStreamWaitEvent(c->copy_stream, S.header_written, 0));
  HIP_TRY(c, hipMemcpyAsync(S.host - S.lead, S.dev - S.lead, S.lead + sizeof(MeshStreamHeader), hipMemcpyDeviceToHost, c->copy_stream));
  HIP_TRY(c, hipEventRecord(S.header_ready, c->copy_stream));
  if (cells) {
    timer_begin(c, "mesh_stream_emit");
    if (R.part) launch_mesh_part_emit(c->stream, V, c->luts, c->frame, mesh_geometry(c), R.scratch, R.slab, R.flags, H, R.records, S.dev + sizeof(MeshStreamHeader));
    else if (R.index_format == kMeshIndexTile16) launch_mesh_stream_emit_compact(c->stream, V, c->luts, c->frame, mesh_geometry(c), R.scratch, R.flags, H, R.records, S.dev + sizeof(MeshStreamHeader), nullptr);
    else launch_mesh_stream_emit(c->stream, V, c->luts, c->frame, mesh_geometry(c), R.scratch, R.flags, H, R.records, S.dev + sizeof(MeshStreamHeader));
    timer_end(c, "mesh_stream_emit");
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(S.emitted, c->stream));
    // With the volume sets alternating, the integrate() two frames later overwrites the set these launches read, and it waits for draw_done[set] only:
    // record that event again behind them (as an overlay does).
    if ((rc = overlay_rerecord_draw(c))) return rc;
    if (R.tap_flags && (rc = mesh_stream_queue_taps(c, S))) return rc;   // behind the emit (the header was written and its copy queued before it)
  }
  ++R.frames;
  return TSDF_OK;
}
int32_t tsdf_mesh_stream_acquire(tsdf_ctx* c, int32_t wait, tsdf_mesh_frame* out, int32_t* ready) {
  CHECK_CTX(c);
  if (!out || (!ready && !wait)) return TSDF_ERR_INVALID_ARGUMENT;
  if (ready) *ready = 0;
  tsdf_ctx::MeshStream& R = c->mstream;
  if (R.ring.acquire() == kResultNoneQueued) FAIL(c, TSDF_ERR_STATE, "no streamed mesh frame is queued");
  if (R.ring.acquire() == kResultAlreadyHeld) FAIL(c, TSDF_ERR_STATE, "a streamed mesh frame is held already: tsdf_mesh_stream_release first");
  HIP_TRY(c, hipSetDevice(c->device));
  tsdf_ctx::MeshStreamSlot& S = R.slot[R.ring.oldest()];
  if (wait && !S.payload_issued) HIP_TRY(c, hipEventSynchronize(S.header_ready));
  int32_t rc;
  if ((rc = mesh_stream_pump(c))) return rc;
  if (!S.payload_issued) return TSDF_OK;                                  // (wait == 0: the header is still travelling)
  if (S.payload_bytes) {
    bool arrived;
    if ((rc = event_reached(c, S.ready, wait != 0, &arrived))) return rc;
    if (!arrived) return TSDF_OK;
  }
  const MeshStreamHeader* H = (const MeshStreamHeader*)S.host;
  const uint32_t stride = R.flags ? 16u : 8u;
  *out = tsdf_mesh_frame{};
  out->vertices = S.host + sizeof(MeshStreamHeader);
  // (tile-local format: the triangles are 16-bit codes, tsdf_mesh_stream_frame_compact hands them out)
  out->triangles = R.index_format == kMeshIndexTile16 ? nullptr : (const uint32_t*)(S.host + sizeof(MeshStreamHeader) + (size_t)H->n_vertices * stride);
  out->n_vertices = H->n_vertices; out->n_triangles = H->n_triangles;
  out->needed_vertices = H->needed_vertices; out->needed_triangles = H->needed_triangles; out->needed_tiles = H->needed_tiles;
  out->tag = S.tag; out->flags = R.flags; out->vertex_stride = stride; out->overflow = H->overflow;
  for (int a = 0; a < 3; ++a) { out->res[a] = (uint32_t)S.res[a]; out->bbox_min[a] = c->cfg.bbox_min[a]; out->bbox_max[a] = c->cfg.bbox_max[a]; }
  R.ring.hold();
  if (ready) *ready = 1;
  return TSDF_OK;
}
int32_t tsdf_mesh_stream_release(tsdf_ctx* c) {
  CHECK_CTX(c);
  tsdf_ctx::MeshStream& R = c->mstream;
  if (!R.ring.release()) FAIL(c, TSDF_ERR_STATE, "no streamed mesh frame is held");
  HIP_TRY(c, hipSetDevice(c->device));
  return mesh_stream_pump(c);
}
int32_t tsdf_mesh_stream_frame_filter(tsdf_ctx* c, uint64_t out[4]) {
  CHECK_CTX(c);
  if (!out) return TSDF_ERR_INVALID_ARGUMENT;
  const tsdf_ctx::MeshStream& R = c->mstream;
  if (!R.configured || !R.min_triangles) FAIL(c, TSDF_ERR_STATE, "the mesh ring is configured without a filter (tsdf_mesh_stream_config_filter, min_triangles >= 1)");
  if (!R.ring.held) FAIL(c, TSDF_ERR_STATE, "no streamed mesh frame is held (tsdf_mesh_stream_acquire)");
  const tsdf_ctx::MeshStreamSlot& S = R.slot[R.ring.oldest()];
  const MeshStreamFilterRecord* r = (const MeshStreamFilterRecord*)(S.host - S.lead);
  out[0] = r->components; out[1] = r->kept; out[2] = r->vertices_removed; out[3] = r->triangles_removed;
  return TSDF_OK;
}
int32_t tsdf_mesh_stream_frame_compact(tsdf_ctx* c, tsdf_mesh_compact* out) {
  CHECK_CTX(c);
  if (!out) return TSDF_ERR_INVALID_ARGUMENT;
  const tsdf_ctx::MeshStream& R = c->mstream;
  if (!R.configured || R.index_format != kMeshIndexTile16) FAIL(c, TSDF_ERR_STATE, "the mesh ring is configured with uint32 indices (tsdf_mesh_stream_config_compact, TSDF_MESH_INDEX_TILE16)");
  if (!R.ring.held) FAIL(c, TSDF_ERR_STATE, "no streamed mesh frame is held (tsdf_mesh_stream_acquire)");
  const tsdf_ctx::MeshStreamSlot& S = R.slot[R.ring.oldest()];
  const MeshStreamHeader* H = (const MeshStreamHeader*)S.host;
  const MeshFrameLayout layout = R.layout();
  const uint8_t* payload = S.host + sizeof(MeshStreamHeader);
  const MeshLattice L = mesh_lattice(S.res, (int)R.level);
  *out = tsdf_mesh_compact{};
  out->table = (const tsdf_mesh_tile_row*)(payload + layout.table_offset(H->n_vertices));
  out->triangles = (const uint16_t*)(payload + layout.triangle_offset(H->n_vertices, S.table_rows));
  out->n_tile_rows = S.table_rows;
  out->tiles[0] = (uint32_t)L.ntx; out->tiles[1] = (uint32_t)L.nty; out->tiles[2] = (uint32_t)L.ntz; out->level = R.level;
  return TSDF_OK;
}
int32_t tsdf_mesh_stream_frame_part(tsdf_ctx* c, tsdf_mesh_part* out) {
  CHECK_CTX(c);
  if (!out) return TSDF_ERR_INVALID_ARGUMENT;
  const tsdf_ctx::MeshStream& R = c->mstream;
  if (!R.configured || !R.part) FAIL(c, TSDF_ERR_STATE, "the mesh ring does not stream parts (tsdf_mesh_stream_config_part)");
  if (!R.ring.held) FAIL(c, TSDF_ERR_STATE, "no streamed mesh frame is held (tsdf_mesh_stream_acquire)");
  const tsdf_ctx::MeshStreamSlot& S = R.slot[R.ring.oldest()];
  const MeshPartLayers P = MeshPartLayers::of(c->vol.own_tz0, c->vol.own_tz1, (S.res[2] + 7) / 8, (int)R.level, mesh_lattice(S.res, (int)R.level).ntz);
  *out = tsdf_mesh_part{};
  out->layers[0] = (uint32_t)P.layer0; out->layers[1] = (uint32_t)P.layer1; out->level = R.level; out->top = P.top ? 1u : 0u;
  out->seam_tiles = (uint32_t)((const MeshStreamPartRecord*)(S.host - S.lead))->seam_tiles;
  return TSDF_OK;
}
int32_t tsdf_mesh_stream_frame_taps(tsdf_ctx* c, tsdf_mesh_taps* out) {
  CHECK_CTX(c);
  if (!out) return TSDF_ERR_INVALID_ARGUMENT;
  const tsdf_ctx::MeshStream& R = c->mstream;
  if (!R.configured || !R.tap_flags) FAIL(c, TSDF_ERR_STATE, "the mesh ring carries no texture taps (tsdf_mesh_stream_config_taps, TSDF_MESH_STREAM_TAPS)");
  if (!R.ring.held) FAIL(c, TSDF_ERR_STATE, "no streamed mesh frame is held (tsdf_mesh_stream_acquire)");
  const tsdf_ctx::MeshStreamSlot& S = R.slot[R.ring.oldest()];
  *out = tsdf_mesh_taps{};
  out->taps = (const tsdf_packed_tap*)(S.host + sizeof(MeshStreamHeader) + mesh_stream_tap_offset(R));
  out->n_vertices = ((const MeshStreamHeader*)S.host)->n_vertices; out->n_streams = c->cfg.num_streams; out->tap_bytes = (uint32_t)kMeshTapBytes;
  return TSDF_OK;
}
int32_t tsdf_mesh_stream_stats(tsdf_ctx* c, uint64_t out[4]) {
  CHECK_CTX(c);
  if (!out) return TSDF_ERR_INVALID_ARGUMENT;
  const tsdf_ctx::MeshStream& R = c->mstream;
  out[0] = R.frames; out[1] = R.overflowed; out[2] = R.bytes_copied; out[3] = R.device_bytes;
  return TSDF_OK;
}

// ---- ray queries (k_rays.hip; the definition is in the header, the host bookkeeping in ray_staging.hpp).  The reference has no counterpart.
// part: the part cast (tsdf_cast_rays_part / _dev), which any context answers -- a slab its owned samples, a whole-volume context the one-slab case
static int32_t ray_cast_checks(tsdf_ctx* c, const void* rays, uint64_t n, uint32_t flags, const void* hits, const void* surface, bool part = false) {
  switch (ray_cast_arguments(n, flags, rays != nullptr, hits != nullptr, surface != nullptr)) {
    case 0: break;
    case 1: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "unknown ray flag (1 unit cube, 2 normals, 4 colours)");
    case 2: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "null ray / hit array");
    case 3: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "the surface array goes with TSDF_RAY_NORMALS / TSDF_RAY_COLOURS: given exactly when one is set");
    default: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "%llu rays in one cast (at most 2^40)", (unsigned long long)n);
  }
  if (part) {
    if (!c->have_volume) FAIL(c, TSDF_ERR_STATE, "no volume yet (tsdf_integrate or tsdf_upload_volume)");
    return (flags & TSDF_RAY_COLOURS) ? require_inputs(c, false, true) : TSDF_OK;
  }
  return readable_volume_check(c, "ray queries on a Z-slab context: a ray crosses slabs; a slab casts its part with tsdf_cast_rays_part and tsdf_merge_ray_parts_dev merges the parts", (flags & TSDF_RAY_COLOURS) != 0);
}
// the launches of one cast on the context's stream, device arrays in and out; no host wait
static int32_t ray_cast_queue(tsdf_ctx* c, const tsdf_ray* rays, uint64_t n, uint32_t flags, tsdf_ray_hit* hits, tsdf_ray_surface* surface, bool part = false) {
  tsdf_ctx::Rays& R = c->rays;
  if (!R.d_list) {                                                       // the context's first cast
    HIP_TRY(c, hipMalloc((void**)&R.d_list, (size_t)kRayChunk * sizeof(RayHitRec)));
    HIP_TRY(c, hipMalloc((void**)&R.d_words, 64));
  }
  uint32_t* count = (uint32_t*)((char*)R.d_words + 32);
  HIP_TRY(c, join_integ(c));                                             // the volume tsdf_download_volume would return now
  if (flags & TSDF_RAY_COLOURS) HIP_TRY(c, join_pre(c));                 // ... and the current frame slot's images
  HIP_TRY(c, hipMemsetAsync(R.d_words, 0, 64, c->stream));
  RayCast Q{};
  box_origin_extent(c, Q.bbox_min, Q.ext);
  Q.flags = flags; Q.run = ray_run_length(c->vol.limit, c->vol.res); Q.n_cap = ray_sample_cap(c->vol.limit);
  const CallChunks K{n, kRayChunk};
  for (uint64_t k = 0; k < K.launches(); ++k) {
    const uint64_t first = K.first(k);
    Q.n = K.count(k);
    if (k && surface) HIP_TRY(c, hipMemsetAsync(count, 0, sizeof(uint32_t), c->stream));
    timer_begin(c, part ? "rays_part_march" : "rays_march");
    (part ? launch_rays_march_part : launch_rays_march)(c->stream, c->vol, Q, rays + first, hits + first, surface ? surface + first : nullptr, R.d_list, count, R.d_words);
    timer_end(c, part ? "rays_part_march" : "rays_march");
    if (surface) {                                                       // (serves a part unchanged: the halo covers the taps, a slab holds whole LUTs and frames)
      timer_begin(c, part ? "rays_part_surface" : "rays_surface");
      launch_rays_surface(c->stream, c->vol, c->luts, c->frame, Q, R.d_list, count, surface + first);
      timer_end(c, part ? "rays_part_surface" : "rays_surface");
    }
  }
  HIP_TRY(c, hipGetLastError());
  R.last_n = n; R.cast = true;
  // With the volume sets alternating, the integrate() two frames later overwrites the set these launches read, and it waits for draw_done[set] only:
  // record that event again behind them (as tsdf_mesh_stream does).
  return overlay_rerecord_draw(c);
}
static int32_t ray_staging_reserve(tsdf_ctx* c, uint64_t n, bool surface) {
  tsdf_ctx::Rays& R = c->rays;
  return staging_reserve(c, R.staging, n, surface, (void**)&R.d_rays, kRayBytes, (void**)&R.d_hits, kRayBytes, (void**)&R.d_surf, kRayBytes);
}
int32_t tsdf_cast_rays(tsdf_ctx* c, const tsdf_ray* rays, uint64_t n, uint32_t flags, tsdf_ray_hit* hits, tsdf_ray_surface* surface) {
  CHECK_CTX(c);
  int32_t rc = ray_cast_checks(c, rays, n, flags, hits, surface);
  if (rc) return rc;
  if (n == 0) { c->rays.last_n = 0; c->rays.cast = true; return TSDF_OK; }
  HIP_TRY(c, hipSetDevice(c->device));
  if ((rc = ray_staging_reserve(c, n, surface != nullptr))) return rc;
  tsdf_ctx::Rays& R = c->rays;
  HIP_TRY(c, hipMemcpyAsync(R.d_rays, rays, (size_t)(n * kRayBytes), hipMemcpyHostToDevice, c->stream));
  if ((rc = ray_cast_queue(c, R.d_rays, n, flags, R.d_hits, surface ? R.d_surf : nullptr))) return rc;
  HIP_TRY(c, hipMemcpyAsync(hits, R.d_hits, (size_t)(n * kRayBytes), hipMemcpyDeviceToHost, c->stream));
  if (surface) HIP_TRY(c, hipMemcpyAsync(surface, R.d_surf, (size_t)(n * kRayBytes), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, sync_ctx(c));
  return TSDF_OK;
}
int32_t tsdf_cast_rays_dev(tsdf_ctx* c, const tsdf_ray* rays_dev, uint64_t n, uint32_t flags, tsdf_ray_hit* hits_dev, tsdf_ray_surface* surface_dev) {
  CHECK_CTX(c);
  int32_t rc = ray_cast_checks(c, rays_dev, n, flags, hits_dev, surface_dev);
  if (rc) return rc;
  if (n == 0) { c->rays.last_n = 0; c->rays.cast = true; return TSDF_OK; }
  HIP_TRY(c, hipSetDevice(c->device));
  return ray_cast_queue(c, rays_dev, n, flags, hits_dev, surface_dev);
}
// A slab's part of a cast: the same calls with the part form of the march (the checks, staging, chunking, stream order and the re-recorded draw event
// are tsdf_cast_rays' and tsdf_cast_rays_dev's)
int32_t tsdf_cast_rays_part(tsdf_ctx* c, const tsdf_ray* rays, uint64_t n, uint32_t flags, tsdf_ray_hit* hits, tsdf_ray_surface* surface) {
  CHECK_CTX(c);
  int32_t rc = ray_cast_checks(c, rays, n, flags, hits, surface, true);
  if (rc) return rc;
  if (n == 0) { c->rays.last_n = 0; c->rays.cast = true; return TSDF_OK; }
  HIP_TRY(c, hipSetDevice(c->device));
  if ((rc = ray_staging_reserve(c, n, surface != nullptr))) return rc;
  tsdf_ctx::Rays& R = c->rays;
  HIP_TRY(c, hipMemcpyAsync(R.d_rays, rays, (size_t)(n * kRayBytes), hipMemcpyHostToDevice, c->stream));
  if ((rc = ray_cast_queue(c, R.d_rays, n, flags, R.d_hits, surface ? R.d_surf : nullptr, true))) return rc;
  HIP_TRY(c, hipMemcpyAsync(hits, R.d_hits, (size_t)(n * kRayBytes), hipMemcpyDeviceToHost, c->stream));
  if (surface) HIP_TRY(c, hipMemcpyAsync(surface, R.d_surf, (size_t)(n * kRayBytes), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, sync_ctx(c));
  return TSDF_OK;
}
int32_t tsdf_cast_rays_part_dev(tsdf_ctx* c, const tsdf_ray* rays_dev, uint64_t n, uint32_t flags, tsdf_ray_hit* hits_dev, tsdf_ray_surface* surface_dev) {
  CHECK_CTX(c);
  int32_t rc = ray_cast_checks(c, rays_dev, n, flags, hits_dev, surface_dev, true);
  if (rc) return rc;
  if (n == 0) { c->rays.last_n = 0; c->rays.cast = true; return TSDF_OK; }
  HIP_TRY(c, hipSetDevice(c->device));
  return ray_cast_queue(c, rays_dev, n, flags, hits_dev, surface_dev, true);
}
// the merge of `parts` parts on the context's stream: needs no volume, allocates nothing
int32_t tsdf_merge_ray_parts_dev(tsdf_ctx* c, const tsdf_ray_hit* hit_parts_dev, const tsdf_ray_surface* surface_parts_dev, uint32_t parts, uint64_t n, uint64_t stride_records,
                                 tsdf_ray_hit* hits_dev, tsdf_ray_surface* surface_dev) {
  CHECK_CTX(c);
  switch (ray_merge_arguments(parts, n, stride_records, hit_parts_dev != nullptr, hits_dev != nullptr, surface_parts_dev != nullptr, surface_dev != nullptr)) {
    case 0: break;
    case 1: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "no part to merge (parts == 0)");
    case 2: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "null hit part / hit array");
    case 3: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "the surface parts and the merged surface array go together: both or neither");
    case 4: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "parts lie %llu records apart and hold %llu each", (unsigned long long)stride_records, (unsigned long long)n);
    default: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "%llu rays x %u parts in one merge (at most 2^40 rays, their parts within 2^48 records)", (unsigned long long)n, parts);
  }
  if (n == 0) return TSDF_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const CallChunks K{n, kRayChunk};
  for (uint64_t k = 0; k < K.launches(); ++k) {
    const uint64_t first = K.first(k);
    launch_rays_merge(c->stream, hit_parts_dev + first, surface_parts_dev ? surface_parts_dev + first : nullptr, parts, K.count(k), stride_records, hits_dev + first,
                      surface_dev ? surface_dev + first : nullptr);
  }
  HIP_TRY(c, hipGetLastError());
  return TSDF_OK;
}
int32_t tsdf_view_rays(tsdf_ctx* c, const float* mv, const float* pr, int32_t x0, int32_t y0, int32_t w, int32_t h, tsdf_ray* rays) {
  CHECK_CTX(c);
  if (!mv || !pr || !rays) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "null matrix / ray array");
  if (ray_view_rect(x0, y0, w, h, c->vw, c->vh)) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "pixel rectangle (%d, %d) + %d x %d outside the %d x %d view", x0, y0, w, h, c->vw, c->vh);
  ViewParams P;
  if (!make_view_params(c, mv, pr, &P)) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "singular modelview / projection matrix");
  HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t n = (uint64_t)w * (uint64_t)h;
  int32_t rc = ray_staging_reserve(c, n, false);
  if (rc) return rc;
  launch_view_rays(c->stream, P, x0, y0, w, h, c->rays.d_rays);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(rays, c->rays.d_rays, (size_t)(n * kRayBytes), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return TSDF_OK;
}
int32_t tsdf_ray_stats(tsdf_ctx* c, uint64_t out[4]) {
  CHECK_CTX(c);
  if (!out) return TSDF_ERR_INVALID_ARGUMENT;
  const tsdf_ctx::Rays& R = c->rays;
  if (!R.cast) FAIL(c, TSDF_ERR_STATE, "no cast yet (tsdf_cast_rays / tsdf_cast_rays_dev / tsdf_cast_rays_part)");
  out[0] = R.last_n; out[1] = out[2] = out[3] = 0;
  if (!R.last_n) return TSDF_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  unsigned long long w[3] = {0, 0, 0};
  HIP_TRY(c, hipMemcpyAsync(w, R.d_words, sizeof(w), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  out[1] = w[0]; out[2] = w[1]; out[3] = w[2];
  return TSDF_OK;
}

// ---- texture taps (k_texture_taps.hip; the definition is in the header, the host bookkeeping in texture_taps.hpp).  The reference has no counterpart.
static int32_t texture_taps_checks(tsdf_ctx* c, const void* xyz, uint64_t n, uint32_t flags, const void* taps, const void* sensor) {
  switch (texture_taps_arguments(n, flags, xyz != nullptr, taps != nullptr, sensor != nullptr)) {
    case 0: break;
    case 1: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "unknown texture tap flag (1 unit cube, 2 sensor records)");
    case 2: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "null point / tap array");
    case 3: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "the sensor array goes with TSDF_TAPS_SENSOR: given exactly when it is set");
    default: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "%llu points in one call (at most 2^40)", (unsigned long long)n);
  }
  return require_inputs(c, false, true);                                 // calibration (cv_xyz_inv, cv_uv) and a frame; no volume is read
}
// the launches of one call on the context's stream, device arrays in and out; no host wait, no allocation
static int32_t texture_taps_queue(tsdf_ctx* c, const float* xyz, uint64_t n, uint32_t flags, tsdf_texture_tap* taps, tsdf_sensor_tap* sensor) {
  tsdf_ctx::TextureTaps& X = c->taps;
  const uint32_t N = c->cfg.num_streams;
  X.last_n = n; X.called = true;
  if (n == 0) return TSDF_OK;                                            // (tsdf_texture_tap_stats answers zeros without reading the counters)
  HIP_TRY(c, hipMemsetAsync(X.d_words, 0, (size_t)kTapStatBytes, c->stream));
  HIP_TRY(c, join_pre(c));                                              // the current frame slot's images, as the coloured ray cast takes them
  TapsLaunch Q{};
  box_origin_extent(c, Q.bbox_min, Q.ext);
  Q.flags = flags;
  const CallChunks K{n, kTapsChunk};
  for (uint64_t k = 0; k < K.launches(); ++k) {
    const uint64_t first = K.first(k);
    Q.n_points = K.count(k);
    timer_begin(c, "texture_taps");
    launch_texture_taps(c->stream, c->luts, c->frame, c->vol.limit, Q, xyz + 3 * first, taps + first * N, sensor ? sensor + first * N : nullptr, X.d_words);
    timer_end(c, "texture_taps");
  }
  HIP_TRY(c, hipGetLastError());
  // the upload two frames later overwrites the slot these launches read: it waits for what the context's stream held when the frame between was opened
  // (the lane ahead's gate), and with the volume sets alternating draw_done[set] is recorded again behind them, as the coloured cast and tsdf_mesh_stream do
  return overlay_rerecord_draw(c);
}
int32_t tsdf_texture_taps(tsdf_ctx* c, const float* xyz, uint64_t n, uint32_t flags, tsdf_texture_tap* taps, tsdf_sensor_tap* sensor) {
  CHECK_CTX(c);
  int32_t rc = texture_taps_checks(c, xyz, n, flags, taps, sensor);
  if (rc) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  tsdf_ctx::TextureTaps& X = c->taps;
  const uint32_t N = c->cfg.num_streams;
  if (n == 0) return texture_taps_queue(c, nullptr, 0, flags, nullptr, nullptr);
  if ((rc = staging_reserve(c, X.staging, n, sensor != nullptr, (void**)&X.d_xyz, kTapPointBytes, (void**)&X.d_taps, N * kTapBytes, (void**)&X.d_sensor, N * kTapBytes))) return rc;
  HIP_TRY(c, hipMemcpyAsync(X.d_xyz, xyz, (size_t)tap_point_bytes(n), hipMemcpyHostToDevice, c->stream));
  if ((rc = texture_taps_queue(c, X.d_xyz, n, flags, X.d_taps, sensor ? X.d_sensor : nullptr))) return rc;
  HIP_TRY(c, hipMemcpyAsync(taps, X.d_taps, (size_t)tap_record_bytes(n, N), hipMemcpyDeviceToHost, c->stream));
  if (sensor) HIP_TRY(c, hipMemcpyAsync(sensor, X.d_sensor, (size_t)tap_record_bytes(n, N), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, sync_ctx(c));
  return TSDF_OK;
}
int32_t tsdf_texture_taps_dev(tsdf_ctx* c, const float* xyz_dev, uint64_t n, uint32_t flags, tsdf_texture_tap* taps_dev, tsdf_sensor_tap* sensor_dev) {
  CHECK_CTX(c);
  int32_t rc = texture_taps_checks(c, xyz_dev, n, flags, taps_dev, sensor_dev);
  if (rc) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  return texture_taps_queue(c, xyz_dev, n, flags, taps_dev, sensor_dev);
}
int32_t tsdf_mesh_texture_taps(tsdf_ctx* c, uint32_t flags, uint64_t* n_vertices, uint32_t* n_streams) {
  CHECK_CTX(c);
  switch (mesh_texture_taps_arguments(flags)) {
    case 0: break;
    case 1: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "unknown texture tap flag (2 sensor records)");
    default: FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "TSDF_TAPS_UNIT_CUBE on the mesh form: a mesh's positions are world coordinates");
  }
  if (!c->mesh.valid) FAIL(c, TSDF_ERR_STATE, "no mesh (tsdf_mesh_extract / tsdf_mesh_extract_lod)");
  int32_t rc = require_inputs(c, false, true);
  if (rc) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  release_mesh_texture_taps(c);
  tsdf_ctx::TextureTaps& X = c->taps;
  const uint32_t N = c->cfg.num_streams;
  const uint64_t nv = c->mesh.nv;
  const bool want_sensor = (flags & TSDF_TAPS_SENSOR) != 0;
  if (nv) {
    bool ok = hipMalloc((void**)&X.mesh_taps, (size_t)tap_record_bytes(nv, N)) == hipSuccess;
    if (ok && want_sensor) ok = hipMalloc((void**)&X.mesh_sensor, (size_t)tap_record_bytes(nv, N)) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); release_mesh_texture_taps(c); FAIL(c, TSDF_ERR_OUT_OF_MEMORY, "no device memory for the texture taps of %llu vertices", (unsigned long long)nv); }
  }
  if ((rc = texture_taps_queue(c, c->mesh.pos, nv, flags, X.mesh_taps, X.mesh_sensor))) { release_mesh_texture_taps(c); return rc; }
  HIP_TRY(c, sync_ctx(c));
  X.mesh_nv = nv; X.mesh_valid = true; X.mesh_has_sensor = want_sensor;
  if (n_vertices) *n_vertices = nv;
  if (n_streams) *n_streams = N;
  return TSDF_OK;
}
int32_t tsdf_mesh_download_texture_taps(tsdf_ctx* c, tsdf_texture_tap* taps, tsdf_sensor_tap* sensor) {
  CHECK_CTX(c);
  const tsdf_ctx::TextureTaps& X = c->taps;
  if (!c->mesh.valid || !X.mesh_valid) FAIL(c, TSDF_ERR_STATE, "no texture taps for the current mesh (tsdf_mesh_texture_taps after the extract)");
  if (sensor && !X.mesh_has_sensor) FAIL(c, TSDF_ERR_STATE, "the last tsdf_mesh_texture_taps produced no sensor records (TSDF_TAPS_SENSOR)");
  if (!X.mesh_nv) return TSDF_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t bytes = (size_t)tap_record_bytes(X.mesh_nv, c->cfg.num_streams);
  if (taps) HIP_TRY(c, hipMemcpy(taps, X.mesh_taps, bytes, hipMemcpyDeviceToHost));
  if (sensor) HIP_TRY(c, hipMemcpy(sensor, X.mesh_sensor, bytes, hipMemcpyDeviceToHost));
  return TSDF_OK;
}
int32_t tsdf_texture_tap_stats(tsdf_ctx* c, uint64_t out[4]) {
  CHECK_CTX(c);
  if (!out) return TSDF_ERR_INVALID_ARGUMENT;
  const tsdf_ctx::TextureTaps& X = c->taps;
  if (!X.called) FAIL(c, TSDF_ERR_STATE, "no texture tap call yet (tsdf_texture_taps / tsdf_texture_taps_dev / tsdf_mesh_texture_taps)");
  out[0] = X.last_n; out[1] = c->cfg.num_streams; out[2] = out[3] = 0;
  if (!X.last_n) return TSDF_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  unsigned long long w[kTapStatSlots * kTapStatStride] = {};             // the counters are kTapStatSlots pairs (texture_taps.hpp): summed here
  HIP_TRY(c, hipMemcpyAsync(w, X.d_words, sizeof(w), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  tap_stat_sum(w, out + 2);
  return TSDF_OK;
}

// ---- frame read-out: what the client's window holds after glfwSwapBuffers (source/kinect_client.cpp:533), converted on the device and copied to a pinned
// host ring (include/rgbd_recon_hip.h, "frame read-out").  The mirror image of the asynchronous upload: a ring, the copy stream, the wire's DXT1.
static size_t present_frame_bytes(const tsdf_ctx* c) {
  return c->present.format == TSDF_PRESENT_DXT1 ? (size_t)((c->vw + 3) / 4) * ((c->vh + 3) / 4) * 8 : (size_t)c->vw * c->vh * 4;
}
int32_t tsdf_present_config(tsdf_ctx* c, uint32_t format, uint32_t flags, uint32_t slots) {
  CHECK_CTX(c);
  if (format > TSDF_PRESENT_DXT1 || (flags & ~TSDF_PRESENT_TOP_DOWN) || slots < 2 || slots > kMaxResultSlots)
    FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "present format %u / flags %u / slots %u (formats 0 RGBA8, 1 DXT1; flag 1 top-down; 2..%u slots)", format, flags, slots, kMaxResultSlots);
  if (!c->present.ring.idle()) FAIL(c, TSDF_ERR_STATE, "%u presented frame(s) are queued or held: acquire and release them first", c->present.ring.count);
  HIP_TRY(c, hipSetDevice(c->device));
  release_present(c);                                                    // (the ring is idle: every copy was waited for before its frame was released)
  c->present.format = format; c->present.flags = flags; c->present.ring.configure(slots);
  return TSDF_OK;
}
int32_t tsdf_present_size(tsdf_ctx* c, uint64_t* bytes) {
  CHECK_CTX(c);
  if (!bytes) return TSDF_ERR_INVALID_ARGUMENT;
  *bytes = (uint64_t)present_frame_bytes(c);
  return TSDF_OK;
}
int32_t tsdf_present(tsdf_ctx* c, uint64_t tag) {
  CHECK_CTX(c);
  tsdf_ctx::Present& R = c->present;
  if (R.ring.full()) FAIL(c, TSDF_ERR_STATE, "all %u present slots are queued or held (tsdf_present_acquire / tsdf_present_release)", R.ring.slots);
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t bytes = present_frame_bytes(c);
  if (R.bytes != bytes) {                                                // first use at this view size and format (tsdf_resize and tsdf_present_config drop the ring)
    release_present(c);
    for (uint32_t k = 0; k < R.ring.slots; ++k) {
      tsdf_ctx::PresentSlot& S = R.slot[k];
      HIP_TRY(c, hipMalloc(&S.dev, bytes));
      HIP_TRY(c, hipHostMalloc(&S.host, bytes, hipHostMallocDefault));
      HIP_TRY(c, hipEventCreateWithFlags(&S.converted, hipEventDisableTiming));
      HIP_TRY(c, hipEventCreateWithFlags(&S.ready, hipEventDisableTiming));
    }
    R.bytes = bytes;
  }
  if (int32_t rc = ensure_copy_stream(c)) return rc;
  tsdf_ctx::PresentSlot& S = R.slot[R.ring.push()];                      // (queued before its calls are: result_paths.hpp's transitions precede what acts on them)
  S.tag = tag;
  // The finished frame: the hole filling writes the framebuffer from its own lane, overlays from the context's stream.  The kernel's output is the slot's
  // device buffer, so the framebuffer is free again when the KERNEL has run, and nobody has to wait for the copy: every later writer of the framebuffer
  // is ordered behind the context's stream already -- the next hole filling waits for draw_done, which fill_colors_impl records on this stream behind the
  // next march (and so behind this kernel); a direct march (colour filling off) and the overlays run on this stream themselves.
  HIP_TRY(c, join_fill(c));
  timer_begin(c, "present");
  launch_present(c->stream, c->d_fb_c, S.dev, c->vw, c->vh, R.format, (R.flags & TSDF_PRESENT_TOP_DOWN) ? 1 : 0);
  timer_end(c, "present");
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipEventRecord(S.converted, c->stream));
  HIP_TRY(c, hipStreamWaitEvent(c->copy_stream, S.converted, 0));
  HIP_TRY(c, hipMemcpyAsync(S.host, S.dev, bytes, hipMemcpyDeviceToHost, c->copy_stream));
  HIP_TRY(c, hipEventRecord(S.ready, c->copy_stream));
  return TSDF_OK;
}
int32_t tsdf_present_acquire(tsdf_ctx* c, int32_t wait, const void** data, uint64_t* bytes, uint64_t* tag, uint32_t size[2]) {
  CHECK_CTX(c);
  if (!data) return TSDF_ERR_INVALID_ARGUMENT;
  *data = nullptr;
  tsdf_ctx::Present& R = c->present;
  if (R.ring.acquire() == kResultNoneQueued) FAIL(c, TSDF_ERR_STATE, "no presented frame is queued");
  if (R.ring.acquire() == kResultAlreadyHeld) FAIL(c, TSDF_ERR_STATE, "a presented frame is held already: tsdf_present_release first");
  HIP_TRY(c, hipSetDevice(c->device));
  const tsdf_ctx::PresentSlot& S = R.slot[R.ring.oldest()];
  bool arrived;
  if (int32_t rc = event_reached(c, S.ready, wait != 0, &arrived)) return rc;
  if (!arrived) return TSDF_OK;                                          // still travelling: *data stays NULL
  R.ring.hold();
  *data = S.host;
  if (bytes) *bytes = (uint64_t)R.bytes;
  if (tag) *tag = S.tag;
  if (size) { size[0] = (uint32_t)c->vw; size[1] = (uint32_t)c->vh; }
  return TSDF_OK;
}
int32_t tsdf_present_release(tsdf_ctx* c) {
  CHECK_CTX(c);
  if (!c->present.ring.release()) FAIL(c, TSDF_ERR_STATE, "no presented frame is held");
  return TSDF_OK;
}

// ---- multi-GPU hooks
int32_t tsdf_halo_info(const tsdf_ctx* c, uint32_t* layers, uint64_t* bytes) {
  CHECK_CTX(c);
  if (layers) *layers = (uint32_t)c->halo_layers;
  if (bytes) *bytes = (uint64_t)c->halo_layers * c->vol.nty * c->vol.ntx * TILE_VOX * sizeof(float);
  return TSDF_OK;
}
int32_t tsdf_halo_pack_dev(tsdf_ctx* c, void* lo, void* hi) {
  CHECK_CTX(c);
  if (c->vol.slot) FAIL(c, TSDF_ERR_STATE, "halo exchange is not available with a sparse tile pool (use slab_recompute_halo)");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, join_integ(c));                                             // (the volume: behind an integrate() in flight on the integrate lane)
  const Volume& V = c->vol;
  const size_t layer = (size_t)V.nty * V.ntx * TILE_VOX, n = (size_t)c->halo_layers * layer * sizeof(float);
  if (lo) HIP_TRY(c, hipMemcpyAsync(lo, V.data + (size_t)(V.own_tz0 - V.tz0) * layer, n, hipMemcpyDeviceToDevice, c->stream));
  if (hi) HIP_TRY(c, hipMemcpyAsync(hi, V.data + (size_t)(V.own_tz1 - c->halo_layers - V.tz0) * layer, n, hipMemcpyDeviceToDevice, c->stream));
  return TSDF_OK;
}
int32_t tsdf_halo_unpack_dev(tsdf_ctx* c, const void* below, const void* above) {
  CHECK_CTX(c);
  if (c->vol.slot) FAIL(c, TSDF_ERR_STATE, "halo exchange is not available with a sparse tile pool (use slab_recompute_halo)");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, join_integ(c));
  const Volume& V = c->vol;
  const size_t layer = (size_t)V.nty * V.ntx * TILE_VOX;
  if (below && V.tz0 < V.own_tz0) {
    const int have = V.own_tz0 - V.tz0;        // < halo_layers only at the volume boundary: take the top `have` layers
    HIP_TRY(c, hipMemcpyAsync(V.data, (const float*)below + (size_t)(c->halo_layers - have) * layer, (size_t)have * layer * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  }
  if (above && V.tz1 > V.own_tz1) {
    const int have = V.tz1 - V.own_tz1;
    HIP_TRY(c, hipMemcpyAsync(V.data + (size_t)(V.own_tz1 - V.tz0) * layer, above, (size_t)have * layer * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  }
  return TSDF_OK;
}
int32_t tsdf_export_partial_dev(tsdf_ctx* c, void* dst) {
  CHECK_CTX(c);
  if (!dst) return TSDF_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, join_fill(c));
  launch_export_partial(c->stream, ray_target(c), c->vw, c->vh, dst);
  HIP_TRY(c, hipGetLastError());
  return TSDF_OK;
}
int32_t tsdf_composite_dev(tsdf_ctx* c, const void* gathered, uint32_t n) {
  CHECK_CTX(c);
  if (!gathered || n < 1) return TSDF_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, join_fill(c));
  c->tiles_img.target_composited(c->fill_holes || masked_direct(c));    // the composite writes every pixel of the march target
  launch_composite(c->stream, gathered, (int)n, ray_target(c), c->vw, c->vh);
  HIP_TRY(c, hipGetLastError());
  return TSDF_OK;
}

int32_t tsdf_export_hits_dev(tsdf_ctx* c, void* dst, uint32_t capacity) {
  CHECK_CTX(c);
  if (!dst || capacity < 1) return TSDF_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  // the raymarch that just ran used counter (hit_parity ^ 1): raymarch_impl flips the parity after its launch
  const int p = c->hit_parity ^ 1;
  HIP_TRY(c, join_fill(c));
  launch_export_hits(c->stream, ray_target(c), c->vw, c->d_hits, c->d_hit_counters + p, c->last_two_pass ? c->d_long : nullptr, c->d_hit_counters + 2 + p, dst, capacity);
  HIP_TRY(c, hipGetLastError());
  return TSDF_OK;
}
int32_t tsdf_composite_hits_dev(tsdf_ctx* c, const void* gathered, uint32_t n, uint64_t stride_bytes) {
  CHECK_CTX(c);
  if (!gathered || n < 1 || n > 32 || stride_bytes < 32) return TSDF_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, comp_key(c));
  // a compositing context that did not march this frame (dedicated compositor, multigpu.py) has no miss counts of its own: 0 then
  HIP_TRY(c, join_fill(c));
  c->tiles_img.target_composited(c->fill_holes || masked_direct(c));    // the composite writes every pixel of the march target
  launch_composite_hits(c->stream, gathered, (size_t)stride_bytes, (int)n, ray_target(c), c->vw, c->vh, c->d_comp_key, c->own_miss_counts ? 1 : 0);
  HIP_TRY(c, hipGetLastError());
  return TSDF_OK;
}

int32_t tsdf_set_march_cap(tsdf_ctx* c, uint32_t samples) { CHECK_CTX(c); c->march_cap = samples; c->tiles_img.drop_history(); return TSDF_OK; }

// ---- timers
int32_t tsdf_enable_timers(tsdf_ctx* c, int32_t a) { CHECK_CTX(c); c->timers_on = a != 0; return TSDF_OK; }
int32_t tsdf_set_timer_filter(tsdf_ctx* c, const char* names) {
  CHECK_CTX(c);
  c->timer_filter = (names && *names) ? "," + std::string(names) + "," : std::string();
  return TSDF_OK;
}
int32_t tsdf_timer_ms(tsdf_ctx* c, const char* name, float* ms) {
  CHECK_CTX(c);
  if (!name || !ms) return TSDF_ERR_INVALID_ARGUMENT;
  auto it = c->timers.find(name);
  if (it == c->timers.end() || it->second.used == 0) FAIL(c, TSDF_ERR_STATE, "timer '%s' has not run", name);
  auto& e = it->second.ev[it->second.used - 1];
  HIP_TRY(c, hipEventSynchronize(e.second));
  HIP_TRY(c, hipEventElapsedTime(ms, e.first, e.second));
  return TSDF_OK;
}
// event pairs are created on first use; creating them inside a measured loop costs host time per frame: make n available up front
int32_t tsdf_timer_reserve(tsdf_ctx* c, const char* name, uint32_t n) {
  CHECK_CTX(c);
  if (!name) return TSDF_ERR_INVALID_ARGUMENT;
  HIP_TRY(c, hipSetDevice(c->device));
  Timer& t = c->timers[name];
  while (t.ev.size() < std::min<size_t>(n, kMaxTimerPairs)) {
    hipEvent_t a, b;
    HIP_TRY(c, hipEventCreate(&a)); HIP_TRY(c, hipEventCreate(&b));
    t.ev.emplace_back(a, b);
  }
  return TSDF_OK;
}
// caller-defined intervals on the context's stream (bench.py brackets whole frames with them)
int32_t tsdf_timer_begin(tsdf_ctx* c, const char* name) { CHECK_CTX(c); if (!name) return TSDF_ERR_INVALID_ARGUMENT; HIP_TRY(c, hipSetDevice(c->device)); timer_begin(c, name); return TSDF_OK; }
int32_t tsdf_timer_end(tsdf_ctx* c, const char* name) { CHECK_CTX(c); if (!name) return TSDF_ERR_INVALID_ARGUMENT; timer_end(c, name); return TSDF_OK; }
// the end event behind the hole filling that is still in flight on its own stream (stage overlap): begin ... end_after_fill spans a whole
// frame from its first kernel to its framebuffer -- the frame's latency, where tsdf_timer_end would stop at the march
int32_t tsdf_timer_end_after_fill(tsdf_ctx* c, const char* name) {
  CHECK_CTX(c);
  if (!name) return TSDF_ERR_INVALID_ARGUMENT;
  if (c->fill_worker) c->fill_worker->drain();
  timer_end_on(c, name, c->lanes.any_fill_pending() ? c->fill_stream : c->stream);
  return TSDF_OK;
}
// the individual samples recorded since the last tsdf_timer_stats / tsdf_timer_samples of this timer (and resets it)
int32_t tsdf_timer_samples(tsdf_ctx* c, const char* name, float* out_ms, uint32_t capacity, uint32_t* count) {
  CHECK_CTX(c);
  if (!name || !count || (!out_ms && capacity)) return TSDF_ERR_INVALID_ARGUMENT;
  *count = 0;
  auto it = c->timers.find(name);
  if (it == c->timers.end()) return TSDF_OK;
  Timer& t = it->second;
  const size_t n = std::min<size_t>(t.used, capacity);
  for (size_t i = 0; i < n; ++i) {
    HIP_TRY(c, hipEventSynchronize(t.ev[i].second));
    HIP_TRY(c, hipEventElapsedTime(&out_ms[i], t.ev[i].first, t.ev[i].second));
  }
  *count = (uint32_t)n;
  t.used = 0;
  return TSDF_OK;
}
int32_t tsdf_timer_spans(tsdf_ctx* c, const char* name, const char* origin, float* begin_ms, float* end_ms, uint32_t capacity, uint32_t* count) {
  CHECK_CTX(c);
  if (!name || !origin || !count || ((!begin_ms || !end_ms) && capacity)) return TSDF_ERR_INVALID_ARGUMENT;
  *count = 0;
  auto it = c->timers.find(name), io = c->timers.find(origin);
  if (it == c->timers.end() || io == c->timers.end() || io->second.used == 0) return TSDF_OK;
  Timer& t = it->second;
  const hipEvent_t zero = io->second.ev[0].first;
  const size_t n = std::min<size_t>(t.used, capacity);
  for (size_t i = 0; i < n; ++i) {
    HIP_TRY(c, hipEventSynchronize(t.ev[i].second));
    HIP_TRY(c, hipEventElapsedTime(&begin_ms[i], zero, t.ev[i].first));
    HIP_TRY(c, hipEventElapsedTime(&end_ms[i], zero, t.ev[i].second));
  }
  *count = (uint32_t)n;
  return TSDF_OK;
}
int32_t tsdf_timer_stats(tsdf_ctx* c, const char* name, uint32_t* count, float* total_ms) {
  CHECK_CTX(c);
  if (!name || !count || !total_ms) return TSDF_ERR_INVALID_ARGUMENT;
  *count = 0; *total_ms = 0.0f;
  auto it = c->timers.find(name);
  if (it == c->timers.end()) return TSDF_OK;
  Timer& t = it->second;
  double sum = 0.0;
  for (size_t i = 0; i < t.used; ++i) {
    float ms = 0.0f;
    HIP_TRY(c, hipEventSynchronize(t.ev[i].second));
    HIP_TRY(c, hipEventElapsedTime(&ms, t.ev[i].first, t.ev[i].second));
    sum += ms;
  }
  *count = (uint32_t)t.used; *total_ms = (float)sum;
  t.used = 0;
  return TSDF_OK;
}

}  // extern "C"
