// The frame intake's bookkeeping: what the two frame slots hold, the two pinned host rings, the raw frame and what was made of it, and the read
// fences behind draws that read a single-buffered image.  Host only, free of HIP: the state and one named transition per event, handing back
// plain values (booleans, 0 / 1 indices into slots[], h_stage[] / stage_done[], h_wire[] / wire_done[], a small enum for a source or a verdict).
// Streams, events, device and pinned pointers, allocations and launches stay in abi.cpp, which acts on what a transition returns.  Three small
// structs, because a site that touches two of them calls two transitions and nothing else couples them: tests/test_frame_intake.py walks every
// state, event and input of each on a CPU.
#pragma once
#include <cstdint>

namespace rr {

// where the frame in a slot came from: what the sensor texture windows may show of it
enum FrameKind { kFrameNone = 0, kFramePre = 1, kFrameRawPending = 2, kFrameRawDone = 3 };

// Two frame slots (the reference's double PBO + texture arrays, NetKinectArray.cpp:225-236): while the path computes on the current slot,
// tsdf_upload_frame_async fills the other one on a copy stream, out of a pinned host staging ring of two buffers; tsdf_select_frame_slot makes
// it current.  The lane ahead flips between the same two slots (lane_ahead.hpp decides when; here: which one is current).  Per slot two events,
// `ready` (recorded on the copy stream after the slot's upload + pack) and `released` (recorded on the context's stream when the slot stopped
// being current); per staging buffer stage_done (recorded on the copy stream behind the copy out of it).
struct FrameSlots {
  // ---- state
  int cur = 0;                                  // the CURRENT slot: what mark / integrate / draw read
  bool have[2] = {false, false};                // the slot holds a frame
  bool pending[2] = {false, false};             // `ready` was recorded and the context's stream has not waited for it
  bool in_use[2] = {false, false};              // `released` was recorded at least once (never cleared: a wait for an old record is free)
  int origin[2] = {kFrameNone, kFrameNone};     // FrameKind of what was written last (a raw upload sets it without `have`)
  bool stage_busy[2] = {false, false};          // stage_done[k] was recorded and the host has not waited for it
  int stage_k = 0;                              // the staging buffer the next asynchronous upload takes

  // ---- read only
  int current() const { return cur; }
  bool have_frame() const { return have[cur]; }
  int kind() const { return have[cur] ? origin[cur] : kFrameNone; }

  // ---- the current slot
  void made_current(int k) { cur = k; }                                               // (creation, the lane's flip, behind select())
  void preprocessed_written() { have[cur] = true; origin[cur] = kFramePre; }          // a pre-processed frame was written into it
  void raw_arrived() { origin[cur] = kFrameRawPending; }                              // a raw frame became resident: its passes will write the slot
  void passes_completed() { have[cur] = true; origin[cur] = kFrameRawDone; }          // ... and have
  // an explicit selection, in front of made_current(slot): record `released` of the old slot on the context's stream (old_events: it has its
  // events; the current slot selected again records nothing), the stream waits for `ready` of the new one
  struct Select { bool record_released, wait_ready; };
  Select select(int slot, bool old_events) {
    const Select S{slot != cur && old_events, pending[slot]};
    if (S.record_released) in_use[cur] = true;
    pending[slot] = false;
    return S;
  }

  // ---- the staging ring and the other slot
  // a staging buffer is handed to the caller: the host waits for stage_done[index] first (its last upload has left the buffer)
  struct Staging { int index; bool wait; };
  Staging staging() {
    const Staging S{stage_k, stage_busy[stage_k]};
    stage_busy[stage_k] = false;
    return S;
  }
  // a pre-processed frame is queued out of staging buffer `staging` into slot `slot`, the one that is not current: the copy stream first waits
  // for `released` of that slot (the path's reads of it were all queued before the record)
  struct Async { int staging, slot; bool wait_released; };
  Async async_queued() {
    const int t = cur ^ 1;
    const Async A{stage_k, t, in_use[t]};
    stage_busy[stage_k] = true; stage_k ^= 1;
    pending[t] = have[t] = true; origin[t] = kFramePre;
    return A;
  }
};

// The raw frame (NetKinectArray::update(): depth + colour of every sensor) and what tsdf_process_textures has made of it.  Its depth is read
// where it lies -- our d_raw (host upload, wire unpack) or the caller's device array (tsdf_upload_raw_frame_dev) --, its RGB8 colour waits to be
// re-laid out into the frame slot: that rides along in the passes' first launch, and whoever reads the slot's colour before asks for it
// (take_colour).  The two generations say which raw upload the passes' products belong to: the Lab image is produced on request from the
// processed frame's inputs, which must still be the resident ones.  A wire message travels through a pinned double buffer (the reference's
// double_pbo): the copy out of buffer k, wire_done[k] behind it, may still be in flight from two frames ago.
enum RawSource { kRawNone = 0, kRawOwn = 1, kRawCaller = 2 };
// what a sensor texture window of type t may show: one of the two kinds of frame, or why not
enum WindowVerdict { kWindowPre, kWindowRaw, kWindowNoFrame, kWindowRawUnprocessed, kWindowNoSuchImage, kWindowNoNormals, kWindowLabStale };

struct RawFrame {
  // ---- state
  int source = kRawNone;                        // RawSource: where the passes read the raw depth (none: no raw frame is resident)
  bool colour_waiting = false;                  // the colour of the raw frame uploaded last is still to be re-laid out
  uint64_t raw_generation = 0, pre_generation = 0;   // the raw uploads so far; the one the passes started on last
  bool pre_processed_depth = true;              // use_processed_depth as the passes found it
  bool use_processed_depth = true;              // the filter pass samples the morphed depth (else the raw one)
  bool normals_uploaded = false;                // the normal image is tsdf_upload_normals', not the passes'
  bool wire_pending[2] = {false, false};        // wire_done[k] was recorded at least once since the buffers were allocated (never cleared by a wait)
  int wire_slot = 0;                            // the pinned buffer the next message takes

  // ---- read only
  bool resident() const { return source != kRawNone; }
  int read_from() const { return source; }
  bool colour_pending() const { return colour_waiting; }
  bool processed_depth() const { return use_processed_depth; }
  // the Lab image's inputs are still those of the frame that was processed
  bool lab_current() const { return pre_generation == raw_generation && pre_processed_depth == use_processed_depth; }
  WindowVerdict window(unsigned type, int kind) const {
    if (kind == kFrameNone) return kWindowNoFrame;
    if (kind == kFrameRawPending) return kWindowRawUnprocessed;
    const bool raw = kind == kFrameRawDone;
    if (!raw && type >= 5) return kWindowNoSuchImage;                                // a frame handed over processed has no morphed raw depth and no Lab image
    if (!raw && type == 3 && !normals_uploaded) return kWindowNoNormals;              // ... and normals only after tsdf_upload_normals
    if (raw && type == 6 && !lab_current()) return kWindowLabStale;
    return raw ? kWindowRaw : kWindowPre;
  }

  // ---- the raw frame
  // a raw frame became resident; colour_pending: its colour waits in RGB8 (else it was written into the slot directly, and a colour that was
  // waiting before still is)
  void uploaded(RawSource from, bool colour_pending) {
    if (colour_pending) colour_waiting = true;
    source = from; ++raw_generation;
  }
  // the colour is taken for re-layout: true = there is one waiting
  bool take_colour() {
    const bool waiting = colour_waiting;
    colour_waiting = false;
    return waiting;
  }
  void set_processed_depth(bool on) { use_processed_depth = on; }
  void passes_started() { pre_generation = raw_generation; pre_processed_depth = use_processed_depth; }   // (any phase: the first one already)
  void passes_completed() { normals_uploaded = false; }
  void normals_were_uploaded() { normals_uploaded = true; }

  // ---- the wire ring
  // a message takes a pinned buffer and its copy is queued behind: the host first waits for wire_done[index]
  struct Wire { int index; bool wait; };
  Wire wire_taken() {
    const Wire W{wire_slot, wire_pending[wire_slot]};
    wire_pending[wire_slot] = true; wire_slot ^= 1;
    return W;
  }
  void wire_reallocated() { wire_pending[0] = wire_pending[1] = false; }             // behind a wait of the host for the streams
};

// The read fences: a draw still queued on the context's stream reads a single-buffered image that the lane ahead is about to rewrite for the
// next frame.  One event per fence, recorded on the context's stream behind the reader; the writer's lane waits for it.
//   kNormalsRead    behind a point draw: the next tsdf_process_textures rewrites the normal image
//   kRawRead        behind an MVT draw or a Lab window: the next raw upload rewrites d_raw
//   kProductsRead   behind a sensor texture window that read one of the products (d_depth2, d_depth_b, d_normal, d_lab): the next
//                   tsdf_process_textures rewrites them, its first two passes in front of the lane's gate
// A writer on the context's stream itself is behind the reader already and takes the fence without a wait.  A wait of the host for the streams
// leaves the flags alone: the wait it leaves behind is for an event long reached.
enum ReadFence { kNormalsRead = 0, kRawRead = 1, kProductsRead = 2, kReadFences = 3 };

struct ReadFences {
  bool pending[kReadFences] = {false, false, false};   // recorded behind a reader, and no writer has taken it since
  void reader_queued(int f) { pending[f] = true; }
  // a writer on a lane takes the fence: true = the lane waits for the event
  bool writer_takes(int f, bool other_stream) {
    const bool wait = pending[f] && other_stream;
    pending[f] = false;
    return wait;
  }
};

struct FrameIntake { FrameSlots slots; RawFrame raw; ReadFences fences; };

}  // namespace rr
