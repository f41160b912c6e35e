// Native multi-GPU exchange behind the C ABI (SURVEY.md section 8b "tsdf_halo_exchange(ctx) / tsdf_composite(ctx) ... one context per rank
// sharing an RCCL communicator", section 8e).  The reference's caller is C++ (source/kinect_client.cpp:569-614): with these entry
// points it drives N GPUs itself -- one process (or thread) per GPU, one context each, RCCL over xGMI on the context's own stream:
//   tsdf_comm_unique_id / tsdf_comm_init / tsdf_comm_destroy   communicator life time (the caller carries the 128-byte id to the ranks)
//   tsdf_broadcast_frame    the frame arrives in ONE process (NetKinectArray's reader, NetKinectArray.cpp:482-529): broadcast of the four
//                           arrays as delivered, then every rank re-lays its copy out (tsdf_upload_frame_dev's launch)
//   tsdf_halo_exchange      all-gather of every slab's two boundary tile layers, before the raymarch
//   tsdf_composite_gather   hit records of every slab -> rank 0, nearest hit per pixel, hole filling; sizes without a host sync per frame
//   tsdf_composite_finish   before the result is read: repairs a gather that turned out too small
// RCCL is bound at run time (dlopen): a process that never calls tsdf_comm_* needs no librccl, and inside a torch process the copy torch
// has already loaded is the one used (two RCCLs in one process would each bring their own device state).
#include <dlfcn.h>

#include <algorithm>
#include <cstdio>
#include <cstring>

#include <rccl/rccl.h>

#include "ctx.hpp"

using namespace rrhost;

namespace {
struct Rccl {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  std::string why;
};
// Thread-safe (C++11 magic static: the object is complete before any caller sees it; "one process (or thread) per GPU" makes concurrent first
// calls the normal case).  RR_TEST_NO_RCCL (test hook): behave as if the library could not be loaded.
static Rccl load_rccl() {
  Rccl R;
  if (getenv("RR_TEST_NO_RCCL")) { R.why = "librccl.so not loaded (RR_TEST_NO_RCCL is set)"; return R; }
  const char* names[] = {"librccl.so.1", "librccl.so"};
  for (int pass = 0; pass < 2 && !R.lib; ++pass)                        // first a copy that is already in the process (torch's), then the system's
    for (const char* n : names)
      if (!R.lib) R.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL | (pass == 0 ? RTLD_NOLOAD : 0));
  if (!R.lib) { const char* e = dlerror(); R.why = std::string("librccl.so not found: ") + (e ? e : "no loader message"); return R; }   // (dlerror() clears itself: one call)
  bool ok = true;
  auto sym = [&](const char* n) { void* p = dlsym(R.lib, n); if (!p) { ok = false; R.why = std::string("librccl lacks ") + n; } return p; };
  R.GetUniqueId = (decltype(R.GetUniqueId))sym("ncclGetUniqueId");
  R.CommInitRank = (decltype(R.CommInitRank))sym("ncclCommInitRank");
  R.CommDestroy = (decltype(R.CommDestroy))sym("ncclCommDestroy");
  R.AllGather = (decltype(R.AllGather))sym("ncclAllGather");
  R.Broadcast = (decltype(R.Broadcast))sym("ncclBroadcast");
  R.Send = (decltype(R.Send))sym("ncclSend");
  R.Recv = (decltype(R.Recv))sym("ncclRecv");
  R.GroupStart = (decltype(R.GroupStart))sym("ncclGroupStart");
  R.GroupEnd = (decltype(R.GroupEnd))sym("ncclGroupEnd");
  R.GetErrorString = (decltype(R.GetErrorString))sym("ncclGetErrorString");
  if (!ok) R.lib = nullptr;
  return R;
}
static Rccl& rccl_state() { static Rccl R = load_rccl(); return R; }
Rccl* rccl() { Rccl& R = rccl_state(); return R.lib ? &R : nullptr; }
const char* rccl_why() { return rccl_state().why.c_str(); }            // why rccl() is null

#define NCCL_TRY(c, expr) do { ncclResult_t _r = (expr); if (_r != ncclSuccess) { FAIL(c, TSDF_ERR_HIP, "%s failed: %s (%s:%d)", #expr, rccl()->GetErrorString(_r), __FILE__, __LINE__); } } while (0)
// inside ncclGroupStart / ncclGroupEnd: an error closes the group before it returns (an open group would swallow every later collective of the thread)
#define NCCL_TRY_IN_GROUP(c, expr) do { ncclResult_t _r = (expr); if (_r != ncclSuccess) { rccl()->GroupEnd(); FAIL(c, TSDF_ERR_HIP, "%s failed: %s (%s:%d)", #expr, rccl()->GetErrorString(_r), __FILE__, __LINE__); } } while (0)
#define NEED_COMM(c) do { CHECK_CTX(c); if (!(c)->comm.comm) FAIL(c, TSDF_ERR_STATE, "no communicator (tsdf_comm_init)"); } while (0)

void release_comm_buffers(tsdf_ctx* c) {
  tsdf_ctx::Comm& M = c->comm;
  hipFree(M.d_halo_send); hipFree(M.d_halo_gath); hipFree(M.d_hitbuf); hipFree(M.d_hitparts); hipFree(M.d_counts); hipFree(M.d_frame_stage);
  for (int k = 0; k < GatherBook::kRing; ++k) { if (M.h_counts[k]) hipHostFree(M.h_counts[k]); if (M.counts_evt[k]) hipEventDestroy(M.counts_evt[k]); }
  tsdf_ctx::Comm fresh;                                                 // the communicator and the roles stay; of the book, what released() keeps
  fresh.comm = M.comm; fresh.roles = M.roles; fresh.book = M.book;
  fresh.book.released();
  M = fresh;
}

// the largest per-rank hit count among the all-gathered [written, hit] counts in ring slot `slot` (waits for their pinned copy: for a frame
// GatherBook::kLag frames back it arrived long ago)
uint32_t max_hits(tsdf_ctx* c, int slot) {
  tsdf_ctx::Comm& M = c->comm;
  if (M.book.recorded(slot)) hipEventSynchronize(M.counts_evt[slot]);
  const int32_t* h = M.h_counts[slot];
  int32_t m = 0;
  for (int r = 0; r < M.roles.world; ++r) m = std::max(m, h[2 * r + 1]);
  return (uint32_t)m;
}

// One exchange of `cap` records per rank, then rank 0 composites.  first: the frame's first exchange, which also all-gathers the hit counts into the
// ring slot the book names; a repeated one (tsdf_composite_finish) does not.  Who exports what, sends and receives: SlabRoles
int32_t exchange_hits(tsdf_ctx* c, uint32_t cap, bool first) {
  tsdf_ctx::Comm& M = c->comm;
  const SlabRoles& P = M.roles;
  Rccl* R = rccl();
  float* const own = P.own_in_parts() ? M.d_hitparts : M.d_hitbuf;
  if (P.exports(first)) {
    if (int32_t rc = tsdf_export_hits_dev(c, own, P.export_records((uint32_t)(c->vw * c->vh), cap))) return rc;
  }
  if (first) {
    NCCL_TRY(c, R->AllGather(own, M.d_counts, 2, ncclInt32, (ncclComm_t)M.comm, c->stream));
    const int slot = M.book.open_slot();
    HIP_TRY(c, hipMemcpyAsync(M.h_counts[slot], M.d_counts, (size_t)P.world * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipEventRecord(M.counts_evt[slot], c->stream));
  }
  const size_t n = SlabRoles::exchange_floats(cap);
  if (P.grouped()) {
    NCCL_TRY(c, R->GroupStart());
    for (int r = P.recv_begin(); r < P.world; ++r) NCCL_TRY_IN_GROUP(c, R->Recv(M.d_hitparts + SlabRoles::row_offset(r, M.hit_floats), n, ncclFloat, r, (ncclComm_t)M.comm, c->stream));
    if (P.send_to() != SlabRoles::kNone) NCCL_TRY_IN_GROUP(c, R->Send(M.d_hitbuf, n, ncclFloat, P.send_to(), (ncclComm_t)M.comm, c->stream));
    NCCL_TRY(c, R->GroupEnd());
  }
  if (P.gathers()) {
    if (int32_t rc = tsdf_composite_hits_dev(c, M.d_hitparts, (uint32_t)P.world, (uint64_t)M.hit_floats * sizeof(float))) return rc;
    if (c->fill_holes) { if (int32_t rc = tsdf_fill_colors(c)) return rc; }
  }
  return TSDF_OK;
}
}  // namespace

extern "C" {

int32_t tsdf_comm_unique_id(uint8_t id[TSDF_COMM_ID_BYTES]) {
  if (!id) return TSDF_ERR_INVALID_ARGUMENT;
  static_assert(TSDF_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "the id is RCCL's");
  Rccl* R = rccl();
  if (!R) { g_create_error = std::string("RCCL is not available in this process: ") + rccl_why(); return TSDF_ERR_STATE; }   // (no context here: tsdf_last_error(NULL) returns it)
  ncclUniqueId u;
  if (R->GetUniqueId(&u) != ncclSuccess) return TSDF_ERR_HIP;
  memcpy(id, u.internal, NCCL_UNIQUE_ID_BYTES);
  return TSDF_OK;
}

int32_t tsdf_comm_init(tsdf_ctx* c, const uint8_t id[TSDF_COMM_ID_BYTES], uint32_t rank, uint32_t world, uint32_t flags) {
  CHECK_CTX(c);
  if (!id || world < 1 || world > 32 || rank >= world) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "rank / world out of range (1 <= world <= 32)");
  const bool dedicated = (flags & TSDF_COMM_DEDICATED_COMPOSITOR) != 0;
  if (dedicated && world < 2) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "a dedicated compositor needs at least one worker rank");
  if (c->comm.comm) FAIL(c, TSDF_ERR_STATE, "the context already has a communicator (tsdf_comm_destroy first)");
  Rccl* R = rccl();
  if (!R) FAIL(c, TSDF_ERR_STATE, "RCCL is not available in this process: %s", rccl_why());
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, sync_ctx(c));
  ncclUniqueId u;
  memcpy(u.internal, id, NCCL_UNIQUE_ID_BYTES);
  ncclComm_t comm = nullptr;
  NCCL_TRY(c, R->CommInitRank(&comm, (int)world, u, (int)rank));        // (collective: every rank of the world calls it, each on its own device)
  tsdf_ctx::Comm& M = c->comm;
  M = tsdf_ctx::Comm{};
  M.comm = comm; M.roles = SlabRoles{(int)rank, (int)world, dedicated};
  return TSDF_OK;
}

int32_t tsdf_comm_destroy(tsdf_ctx* c) {
  CHECK_CTX(c);
  if (!c->comm.comm) return TSDF_OK;
  hipSetDevice(c->device);
  sync_ctx(c);
  release_comm_buffers(c);
  if (Rccl* R = rccl()) R->CommDestroy((ncclComm_t)c->comm.comm);
  c->comm = tsdf_ctx::Comm{};
  return TSDF_OK;
}

// bounds of the lagged guess of a frame's gather size: at least min_records (default 4096), at most max_records (0 = one per view pixel).  The
// result never depends on the guess -- tsdf_composite_finish repairs a gather that was too small --; tests force that path with a small maximum.
int32_t tsdf_comm_set_capacity_limits(tsdf_ctx* c, uint32_t min_records, uint32_t max_records) {
  NEED_COMM(c);
  if (min_records < 1 || (max_records && max_records < min_records)) return TSDF_ERR_INVALID_ARGUMENT;
  c->comm.book.set_limits(min_records, max_records);
  return TSDF_OK;
}
// Was frame `frame` (0 = the first tsdf_composite_gather of this communicator's buffers) composited from TRUNCATED record lists and left that way?
// A gather is sized from the hit counts of two frames earlier; a frame that hit more rays than that is repaired by tsdf_composite_finish only while
// it is the latest frame.  *truncated: 0 = complete (or repaired), 1 = pixels of that frame may be missing (a caller that kept it must redraw).
// The verdict of a frame is known once its counts have reached the host: at once for the latest three frames (the call waits for the pinned copy),
// from a ring of the last 64 frames otherwise; TSDF_ERR_STATE: not gathered yet, or too old.
int32_t tsdf_comm_frame_status(tsdf_ctx* c, uint64_t frame, int32_t* truncated) {
  NEED_COMM(c);
  if (!truncated) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "null argument");
  const GatherBook::Status S = c->comm.book.status(frame);
  switch (S.kind) {
    case GatherBook::Status::kNotGathered:
      FAIL(c, TSDF_ERR_STATE, "frame %llu has not been gathered yet (%llu frames so far)", (unsigned long long)frame, (unsigned long long)c->comm.book.frame_no);
    case GatherBook::Status::kVerdict: *truncated = S.truncated; return TSDF_OK;
    case GatherBook::Status::kCompare:                                    // its counts are still in the ring of pinned copies
      HIP_TRY(c, hipSetDevice(c->device));
      *truncated = max_hits(c, S.slot) > S.cap ? 1 : 0;
      return TSDF_OK;
    default: break;
  }
  FAIL(c, TSDF_ERR_STATE, "the verdict of frame %llu is no longer kept (the last %d frames are)", (unsigned long long)frame, GatherBook::kVerdicts);
}
int32_t tsdf_comm_stats(tsdf_ctx* c, uint32_t* regathers, uint32_t* overflowed_frames) {
  NEED_COMM(c);
  if (regathers) *regathers = c->comm.book.regathers;
  if (overflowed_frames) *overflowed_frames = c->comm.book.overflowed_frames;
  return TSDF_OK;
}

// SURVEY.md section 8e "Per-frame images are replicated: uploaded to every rank, or ncclBroadcast from the receiving rank".  The root passes the
// frame's four arrays (host or device memory), the others NULL.
int32_t tsdf_broadcast_frame(tsdf_ctx* c, uint32_t root, const float* depth_rg, const float* quality, const float* silhouette, const uint8_t* colour) {
  NEED_COMM(c);
  tsdf_ctx::Comm& M = c->comm;
  const SlabRoles& P = M.roles;
  if ((int)root >= P.world) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "root out of range");
  HIP_TRY(c, hipSetDevice(c->device));
  const FrameImages& F = c->frame;
  const size_t np = (size_t)c->cfg.num_streams * F.w * F.h, nc = (size_t)c->cfg.num_streams * F.cw * F.ch;
  const size_t bytes = np * 16 + ((nc * 3 + 15) & ~(size_t)15);         // [depth_rg 8 B][quality 4 B][silhouette 4 B] per pixel, then RGB8
  if (!M.d_frame_stage) { HIP_TRY(c, hipMalloc((void**)&M.d_frame_stage, bytes)); M.frame_stage_bytes = bytes; }
  uint8_t* st = (uint8_t*)M.d_frame_stage;
  if ((int)root == P.rank) {
    if (!depth_rg || !quality || !silhouette || !colour) FAIL(c, TSDF_ERR_INVALID_ARGUMENT, "the root passes all four arrays");
    // (hipMemcpyDefault: the root's arrays may lie in host memory -- pinned, for a copy that really is asynchronous -- or in device memory)
    HIP_TRY(c, hipMemcpyAsync(st, depth_rg, np * 8, hipMemcpyDefault, c->stream));
    HIP_TRY(c, hipMemcpyAsync(st + np * 8, quality, np * 4, hipMemcpyDefault, c->stream));
    HIP_TRY(c, hipMemcpyAsync(st + np * 12, silhouette, np * 4, hipMemcpyDefault, c->stream));
    HIP_TRY(c, hipMemcpyAsync(st + np * 16, colour, nc * 3, hipMemcpyDefault, c->stream));
  }
  if (P.grouped()) NCCL_TRY(c, rccl()->Broadcast(st, st, bytes, ncclUint8, (int)root, (ncclComm_t)M.comm, c->stream));
  if (!P.worker()) return TSDF_OK;                                      // a compositor without a slab reads no frame
  return tsdf_upload_frame_dev(c, (const float*)st, (const float*)(st + np * 8), (const float*)(st + np * 12), st + np * 16, 0);   // (behind the broadcast on the context's stream)
}

int32_t tsdf_halo_exchange(tsdf_ctx* c) {
  NEED_COMM(c);
  tsdf_ctx::Comm& M = c->comm;
  const SlabRoles& P = M.roles;
  HIP_TRY(c, hipSetDevice(c->device));
  uint32_t layers = 0; uint64_t face_bytes = 0;
  tsdf_halo_info(c, &layers, &face_bytes);
  const size_t n = (size_t)(face_bytes / sizeof(float));
  if (!M.d_halo_send || M.halo_floats != n) {
    HIP_TRY(c, sync_ctx(c));
    hipFree(M.d_halo_send); hipFree(M.d_halo_gath); M.d_halo_send = M.d_halo_gath = nullptr;
    HIP_TRY(c, hipMalloc((void**)&M.d_halo_send, 2 * n * sizeof(float)));
    HIP_TRY(c, hipMalloc((void**)&M.d_halo_gath, (size_t)P.world * 2 * n * sizeof(float)));
    HIP_TRY(c, hipMemsetAsync(M.d_halo_send, 0, 2 * n * sizeof(float), c->stream));       // (a compositor sends these zeros: nobody reads them)
    M.halo_floats = n;
  }
  if (P.worker()) { if (int32_t rc = tsdf_halo_pack_dev(c, M.d_halo_send, M.d_halo_send + n)) return rc; }
  NCCL_TRY(c, rccl()->AllGather(M.d_halo_send, M.d_halo_gath, 2 * n, ncclFloat, (ncclComm_t)M.comm, c->stream));
  if (!P.worker()) return TSDF_OK;                                      // (took part in the collective; has no slab faces of its own)
  const SlabRoles::Face lo = P.below(), hi = P.above();                 // the lower neighbour's HIGH face, the upper neighbour's LOW face
  const float* below = lo.row != SlabRoles::kNone ? M.d_halo_gath + SlabRoles::face_offset(lo, n) : nullptr;
  const float* above = hi.row != SlabRoles::kNone ? M.d_halo_gath + SlabRoles::face_offset(hi, n) : nullptr;
  return tsdf_halo_unpack_dev(c, below, above);
}

int32_t tsdf_composite_gather(tsdf_ctx* c) {
  NEED_COMM(c);
  tsdf_ctx::Comm& M = c->comm;
  HIP_TRY(c, hipSetDevice(c->device));
  const SlabRoles& P = M.roles;
  const size_t hf = SlabRoles::row_floats((size_t)c->vw * c->vh);
  if (!(M.d_hitbuf || M.d_hitparts) || M.hit_floats != hf) {
    HIP_TRY(c, sync_ctx(c));
    release_comm_buffers(c);                                            // (the book counts frames from 0 again)
    if (!P.gathers()) {
      HIP_TRY(c, hipMalloc((void**)&M.d_hitbuf, hf * sizeof(float)));
      HIP_TRY(c, hipMemsetAsync(M.d_hitbuf, 0, hf * sizeof(float), c->stream));
    } else {
      HIP_TRY(c, hipMalloc((void**)&M.d_hitparts, (size_t)P.world * hf * sizeof(float)));
      HIP_TRY(c, hipMemsetAsync(M.d_hitparts, 0, (size_t)P.world * hf * sizeof(float), c->stream));
    }
    HIP_TRY(c, hipMalloc((void**)&M.d_counts, (size_t)P.world * 2 * sizeof(int32_t)));
    for (int k = 0; k < GatherBook::kRing; ++k) {
      HIP_TRY(c, hipHostMalloc((void**)&M.h_counts[k], (size_t)P.world * 2 * sizeof(int32_t), hipHostMallocDefault));
      memset(M.h_counts[k], 0, (size_t)P.world * 2 * sizeof(int32_t));
      HIP_TRY(c, hipEventCreateWithFlags(&M.counts_evt[k], hipEventDisableTiming));
    }
    M.hit_floats = hf;
  }
  const int lagged = M.book.lagged_slot();                              // (none for the first kLag frames: no history yet)
  const uint32_t cap = M.book.open((uint32_t)(c->vw * c->vh), lagged >= 0 ? max_hits(c, lagged) : 0);
  if (int32_t rc = exchange_hits(c, cap, true)) return rc;
  M.book.queued(cap);
  return TSDF_OK;
}

// Completes the latest frame: call before reading its result (and at the end of a timed region).  A COLLECTIVE when the gather of that
// frame turned out too small -- every rank sees the same counts and re-gathers together (the hit list stays valid until the next draw).
int32_t tsdf_composite_finish(tsdf_ctx* c, uint32_t* regathered) {
  NEED_COMM(c);
  tsdf_ctx::Comm& M = c->comm;
  HIP_TRY(c, hipSetDevice(c->device));
  if (regathered) *regathered = 0;
  const int pending = M.book.pending_slot();
  if (pending >= 0) {
    const GatherBook::Repair fix = M.book.finish((uint32_t)(c->vw * c->vh), max_hits(c, pending));
    if (fix.regather) {
      if (regathered) *regathered = 1;
      if (int32_t rc = exchange_hits(c, fix.cap, false)) return rc;
    }
  }
  HIP_TRY(c, sync_ctx(c));
  return TSDF_OK;
}

}  // extern "C"
