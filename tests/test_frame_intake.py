"""csrc/frame_intake.hpp: the frame intake's bookkeeping as three small state machines -- the two frame slots with the staging ring (14 one-bit
fields or pairs: 16 384 states), the raw frame with the wire ring (source, colour, the two generation counters as opaque tokens from a domain
of three values each, five flags, the ring; beside it the two pointers abi.cpp keeps, as tokens: 13 824 states) and the three read fences
(8 states) --, each for every combination of its fields, every event and every combination of the event's inputs, against a restatement of
the statements abi.cpp held at each of those places before the header existed: written over the loose fields tsdf_ctx had then, with every
HIP call replaced by a value handed back in order.  The fields are compared one by one after the event, so an incremented generation may
leave its domain.  Then a breadth-first walk of each from the initial state with a shadow kept from what the transitions HAND BACK alone, for
what the protocol promises.  The header is host-only and free of HIP, so a plain g++ builds the walk -- and a second time with
-fsanitize=address,undefined, as an executable of its own; the program compares the rows itself and prints how many it walked."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbd-recon_amd", "csrc")

# per part: states, and per event the number of input combinations
SLOT_STATES, RAW_STATES, FENCE_STATES = 1 << 14, 3 * 2 * 9 * 2 ** 6 * 2 * 2, 8
SLOT_EVENTS = dict(made_current=2, pre_written=1, raw_arrived=1, passes_completed=1, staging=1, async_upload=1, select=4, have_frame=1, kind=1, current=1)
RAW_EVENTS = dict(upload_host=1, upload_dev=1, upload_wire=1, wire_realloc=1, flush_colour=1, process=3, lab_current=1, window=28, normals_uploaded=1,
                  set_preprocess=2, resident=1, raw_depth=1)
FENCE_EVENTS = dict(points_drawn=1, mvt_drawn=1, window_drawn=2, raw_upload=2, process=4)

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "frame_intake.hpp"
using namespace rr;

enum { kOut = 3 };
static long rows = 0, mismatches = 0, violations = 0;
static void mismatch(const char* part, int s, int ev, int in, const int* got, const int* want, bool fields) {
  if (++mismatches <= 10) std::printf("mismatch: %s state %05x event %d inputs %d: fields %s; returned %d %d %d, was %d %d %d\n", part, s, ev, in, fields ? "equal" : "DIFFER",
                                      got[0], got[1], got[2], want[0], want[1], want[2]);
}
static void violated(const char* what, int s, int ev, int in) {
  if (++violations <= 10) std::printf("violated: %s (state %05x, event %d, inputs %d)\n", what, s, ev, in);
}

// ================================================================ the frame slots and the staging ring
// ---- tsdf_ctx as it stood: FrameSlot's four bookkeeping members and the loose fields
struct OldSlot { bool have, pending, in_use; int origin; };
struct OldSlots { OldSlot slots[2]; int cur_slot; bool stage_busy[2]; int stage_k; };
static const int kSlotStates = 1 << 14;
static OldSlots old_slots(int s) {
  OldSlots c;
  c.cur_slot = s & 1; c.stage_k = (s >> 9) & 1;
  for (int k = 0; k < 2; ++k) {
    c.slots[k].have = (s >> (1 + k)) & 1; c.slots[k].pending = (s >> (3 + k)) & 1; c.slots[k].in_use = (s >> (5 + k)) & 1; c.stage_busy[k] = (s >> (7 + k)) & 1;
    c.slots[k].origin = (s >> (10 + 2 * k)) & 3;
  }
  return c;
}
static FrameSlots new_slots(int s) {
  FrameSlots f;
  f.cur = s & 1; f.stage_k = (s >> 9) & 1;
  for (int k = 0; k < 2; ++k) {
    f.have[k] = (s >> (1 + k)) & 1; f.pending[k] = (s >> (3 + k)) & 1; f.in_use[k] = (s >> (5 + k)) & 1; f.stage_busy[k] = (s >> (7 + k)) & 1;
    f.origin[k] = (s >> (10 + 2 * k)) & 3;
  }
  return f;
}
static int index_of(const FrameSlots& f) {
  int s = f.cur | (f.stage_k << 9);
  for (int k = 0; k < 2; ++k) s |= (f.have[k] << (1 + k)) | (f.pending[k] << (3 + k)) | (f.in_use[k] << (5 + k)) | (f.stage_busy[k] << (7 + k)) | (f.origin[k] << (10 + 2 * k));
  return s;
}
static bool same(const OldSlots& c, const FrameSlots& f) {
  bool ok = c.cur_slot == f.cur && c.stage_k == f.stage_k;
  for (int k = 0; k < 2; ++k)
    ok = ok && c.slots[k].have == f.have[k] && c.slots[k].pending == f.pending[k] && c.slots[k].in_use == f.in_use[k] && c.slots[k].origin == f.origin[k] && c.stage_busy[k] == f.stage_busy[k];
  return ok;
}
enum SlotEvent { MADE_CURRENT, PRE_WRITTEN, RAW_ARRIVED, PASSES_COMPLETED, STAGING, ASYNC_UPLOAD, SELECT, HAVE_FRAME, KIND, CURRENT, N_SLOT_EVENTS };
static const int slot_inputs[N_SLOT_EVENTS] = {2, 1, 1, 1, 1, 1, 4, 1, 1, 1};
// ---- abi.cpp as it stood, one case per site.  o[] = what the site did with HIP, in the order it did it (-1: nothing)
static void run_old(OldSlots* c, int ev, int in, int* o) {
  switch (ev) {
    case MADE_CURRENT: c->cur_slot = in; break;                           // use_frame_slot(c, k): tsdf_create, begin_slot_write's flip
    case PRE_WRITTEN: c->slots[c->cur_slot].have = true; c->slots[c->cur_slot].origin = 1 /* kFramePre */; break;   // tsdf_upload_frame, tsdf_upload_frame_dev
    case RAW_ARRIVED: c->slots[c->cur_slot].origin = 2 /* kFrameRawPending */; break;                               // the three raw uploads' tail
    case PASSES_COMPLETED: c->slots[c->cur_slot].have = true; c->slots[c->cur_slot].origin = 3 /* kFrameRawDone */; break;   // process_textures_impl, phase != 1
    case STAGING: {                                                       // tsdf_frame_staging.  o = {h_stage[.] handed out; after hipEventSynchronize(stage_done[.])}
      const int k = c->stage_k;
      if (c->stage_busy[k]) { o[1] = 1; c->stage_busy[k] = false; }
      o[0] = k;
      break;
    }
    case ASYNC_UPLOAD: {                                                  // tsdf_upload_frame_async behind tsdf_frame_staging.  o = {the copy out of h_stage[.] + stage_done[.]; the slot packed into, whose `ready` is recorded; the copy stream waits for its `released`}
      const int k = c->stage_k, t = c->cur_slot ^ 1;
      OldSlot& S = c->slots[t];
      if (S.in_use) o[2] = 1;
      o[0] = k;
      c->stage_busy[k] = true; c->stage_k ^= 1;
      o[1] = t;
      S.pending = true; S.have = true; S.origin = 1;
      break;
    }
    case SELECT: {                                                        // tsdf_select_frame_slot.  in = slot | (the old slot has its events) << 1.  o = {`released` of the old slot recorded; the stream waits for `ready` of the new one}
      const int slot = in & 1;
      OldSlot& N = c->slots[slot];
      if (slot != c->cur_slot) {
        OldSlot& O = c->slots[c->cur_slot];
        if (in & 2) { o[0] = 1; O.in_use = true; }
      }
      if (N.pending) { o[1] = 1; N.pending = false; }
      c->cur_slot = slot;                                                 // use_frame_slot(c, slot)
      break;
    }
    case HAVE_FRAME: o[0] = c->slots[c->cur_slot].have; break;            // require_inputs
    case KIND: { const OldSlot& S = c->slots[c->cur_slot]; o[0] = S.have ? S.origin : 0; break; }   // tsdf_draw_sensor_texture
    default: o[0] = c->cur_slot; break;                                   // tsdf_current_frame_slot, c->slots[c->cur_slot].ranges
  }
}
// ---- the same places as abi.cpp drives the header now
static void run_new(FrameSlots* f, int ev, int in, int* o) {
  switch (ev) {
    case MADE_CURRENT: f->made_current(in); break;
    case PRE_WRITTEN: f->preprocessed_written(); break;
    case RAW_ARRIVED: f->raw_arrived(); break;
    case PASSES_COMPLETED: f->passes_completed(); break;
    case STAGING: { const FrameSlots::Staging G = f->staging(); if (G.wait) o[1] = 1; o[0] = G.index; break; }
    case ASYNC_UPLOAD: { const FrameSlots::Async A = f->async_queued(); if (A.wait_released) o[2] = 1; o[0] = A.staging; o[1] = A.slot; break; }
    case SELECT: {
      const FrameSlots::Select T = f->select(in & 1, (in & 2) != 0);
      if (T.record_released) o[0] = 1;
      if (T.wait_ready) o[1] = 1;
      f->made_current(in & 1);
      break;
    }
    case HAVE_FRAME: o[0] = f->have_frame(); break;
    case KIND: o[0] = f->kind(); break;
    default: o[0] = f->current(); break;
  }
}

// ================================================================ the raw frame and the wire ring
// pointers as tokens
enum { kNull = 0, kDRaw = 1, kCaller = 2, kStageCol = 3, kDepth2 = 4 };
struct OldRaw {
  bool have_raw; int raw_src, pending_rgb; uint64_t raw_generation, pre_generation; bool pre_processed_depth, use_processed_depth, normals_uploaded, wire_pending[2]; int wire_slot;
};
// abi.cpp's side now: the header's state and the two pointers abi.cpp keeps (the caller's raw depth; the RGB8 colour, stale once taken)
struct NewRaw { RawFrame raw; int raw_src, pending_rgb; };
static int raw_depth(const NewRaw& n) { return n.raw.read_from() == kRawOwn ? kDRaw : n.raw_src; }
static int pending_colour(const NewRaw& n) { return n.raw.colour_pending() ? n.pending_rgb : kNull; }
static const int kRawRadix[12] = {3, 2, 3, 3, 2, 2, 2, 2, 2, 2, 2, 2};   // source, colour waiting, raw / pre generation, pre_processed_depth, use_processed_depth, normals_uploaded, wire_pending[2], wire_slot, raw_src, pending_rgb
static const int kRawStates = 3 * 2 * 9 * 64 * 4;
static NewRaw new_raw(int s) {
  int d[12];
  for (int k = 0; k < 12; ++k) { d[k] = s % kRawRadix[k]; s /= kRawRadix[k]; }
  NewRaw n;
  n.raw.source = d[0]; n.raw.colour_waiting = d[1]; n.raw.raw_generation = d[2]; n.raw.pre_generation = d[3]; n.raw.pre_processed_depth = d[4]; n.raw.use_processed_depth = d[5];
  n.raw.normals_uploaded = d[6]; n.raw.wire_pending[0] = d[7]; n.raw.wire_pending[1] = d[8]; n.raw.wire_slot = d[9];
  n.raw_src = d[10] ? kCaller : kNull; n.pending_rgb = d[11] ? kCaller : kStageCol;
  return n;
}
static int index_of(const NewRaw& n) {
  const int d[12] = {n.raw.source, n.raw.colour_waiting, (int)n.raw.raw_generation, (int)n.raw.pre_generation, n.raw.pre_processed_depth, n.raw.use_processed_depth, n.raw.normals_uploaded,
                     n.raw.wire_pending[0], n.raw.wire_pending[1], n.raw.wire_slot, n.raw_src == kCaller, n.pending_rgb == kCaller};
  int s = 0;
  for (int k = 11; k >= 0; --k) s = s * kRawRadix[k] + d[k];
  return s;
}
static OldRaw old_raw(const NewRaw& n) {
  OldRaw c;
  c.have_raw = n.raw.source != kRawNone; c.raw_src = raw_depth(n); c.pending_rgb = pending_colour(n);
  c.raw_generation = n.raw.raw_generation; c.pre_generation = n.raw.pre_generation; c.pre_processed_depth = n.raw.pre_processed_depth; c.use_processed_depth = n.raw.use_processed_depth;
  c.normals_uploaded = n.raw.normals_uploaded; c.wire_pending[0] = n.raw.wire_pending[0]; c.wire_pending[1] = n.raw.wire_pending[1]; c.wire_slot = n.raw.wire_slot;
  return c;
}
static bool same(const OldRaw& c, const NewRaw& n) {
  return c.have_raw == n.raw.resident() && c.raw_src == raw_depth(n) && c.pending_rgb == pending_colour(n) && c.raw_generation == n.raw.raw_generation && c.pre_generation == n.raw.pre_generation &&
         c.pre_processed_depth == n.raw.pre_processed_depth && c.use_processed_depth == n.raw.use_processed_depth && c.normals_uploaded == n.raw.normals_uploaded &&
         c.wire_pending[0] == n.raw.wire_pending[0] && c.wire_pending[1] == n.raw.wire_pending[1] && c.wire_slot == n.raw.wire_slot;
}
enum RawEvent { UPLOAD_HOST, UPLOAD_DEV, UPLOAD_WIRE, WIRE_REALLOC, FLUSH_COLOUR, PROCESS, LAB_CURRENT, WINDOW, NORMALS_UPLOADED, SET_PREPROCESS, RESIDENT, RAW_DEPTH, N_RAW_EVENTS };
static const int raw_inputs[N_RAW_EVENTS] = {1, 1, 1, 1, 1, 3, 1, 28, 1, 2, 1, 1};
static bool old_lab_stale(const OldRaw* c) { return c->pre_generation != c->raw_generation || c->pre_processed_depth != c->use_processed_depth; }
static void run_old(OldRaw* c, int ev, int in, int* o) {
  switch (ev) {
    case UPLOAD_HOST: c->pending_rgb = kStageCol; c->raw_src = kDRaw; c->have_raw = true; ++c->raw_generation; break;   // tsdf_upload_raw_frame
    case UPLOAD_DEV: c->pending_rgb = kCaller; c->raw_src = kCaller; c->have_raw = true; ++c->raw_generation; break;    // upload_raw_frame_dev_impl
    case UPLOAD_WIRE: {                                                   // tsdf_upload_wire_frame.  o = {h_wire[.] taken, wire_done[.] recorded behind its copy; after hipEventSynchronize(wire_done[.])}
      const int k = c->wire_slot; c->wire_slot ^= 1;
      if (c->wire_pending[k]) o[1] = 1;
      o[0] = k;
      c->wire_pending[k] = true;
      c->raw_src = kDRaw; c->have_raw = true; ++c->raw_generation;
      break;
    }
    case WIRE_REALLOC: c->wire_pending[0] = false; c->wire_pending[1] = false; break;   // the message grew: behind sync_ctx
    case FLUSH_COLOUR:                                                    // flush_pending_colour.  o = {what launch_pack_color reads}
      if (!c->pending_rgb) break;
      o[0] = c->pending_rgb;
      c->pending_rgb = kNull;
      break;
    case PROCESS: {                                                       // process_textures_impl, phase = in.  o = {B.raw; B.fdepth; the rgb the launches get}
      o[0] = c->raw_src; o[1] = c->use_processed_depth ? (int)kDepth2 : c->raw_src;
      c->pre_generation = c->raw_generation; c->pre_processed_depth = c->use_processed_depth;
      o[2] = in == 1 ? (int)kNull : c->pending_rgb;
      if (in != 1) { c->pending_rgb = kNull; c->normals_uploaded = false; }
      break;
    }
    case LAB_CURRENT: o[0] = !old_lab_stale(c); break;                    // produce_lab
    case WINDOW: {                                                        // tsdf_draw_sensor_texture.  in = type + 7 * origin.  o = {which FAIL (0: none); raw}
      const int type = in % 7, origin = in / 7;
      if (origin == 0) { o[0] = 1; break; }
      if (origin == 2) { o[0] = 2; break; }
      const bool raw = origin == 3;
      if (!raw && type >= 5) { o[0] = 3; break; }
      if (!raw && type == 3 && !c->normals_uploaded) { o[0] = 4; break; }
      if (raw && type == 6) { if (old_lab_stale(c)) { o[0] = 5; break; } }
      o[0] = 0; o[1] = raw;
      break;
    }
    case NORMALS_UPLOADED: c->normals_uploaded = true; break;             // tsdf_upload_normals
    case SET_PREPROCESS: c->use_processed_depth = in != 0; break;         // tsdf_set_preprocess
    case RESIDENT: o[0] = c->have_raw; break;                             // tsdf_draw_mvt, tsdf_download_raw_frame, tsdf_download_preprocessed, process_textures_impl
    default: o[0] = c->raw_src; break;                                    // tsdf_download_raw_frame, tsdf_draw_mvt
  }
}
static void run_new(NewRaw* n, int ev, int in, int* o) {
  RawFrame& r = n->raw;
  switch (ev) {
    case UPLOAD_HOST: n->pending_rgb = kStageCol; r.uploaded(kRawOwn, true); break;
    case UPLOAD_DEV: n->pending_rgb = kCaller; n->raw_src = kCaller; r.uploaded(kRawCaller, true); break;
    case UPLOAD_WIRE: { const RawFrame::Wire W = r.wire_taken(); if (W.wait) o[1] = 1; o[0] = W.index; r.uploaded(kRawOwn, false); break; }
    case WIRE_REALLOC: r.wire_reallocated(); break;
    case FLUSH_COLOUR: if (r.take_colour()) o[0] = n->pending_rgb; break;
    case PROCESS: {
      o[0] = raw_depth(*n); o[1] = r.processed_depth() ? (int)kDepth2 : o[0];
      r.passes_started();
      o[2] = in != 1 && r.take_colour() ? n->pending_rgb : (int)kNull;
      if (in != 1) r.passes_completed();
      break;
    }
    case LAB_CURRENT: o[0] = r.lab_current(); break;
    case WINDOW: {
      const WindowVerdict v = r.window((unsigned)(in % 7), in / 7);
      if ((v == kWindowRaw) != (in / 7 == kFrameRawDone && v <= kWindowRaw)) violated("a window verdict of 'raw, processed' on another kind of frame", 0, ev, in);
      switch (v) {
        case kWindowNoFrame: o[0] = 1; break;
        case kWindowRawUnprocessed: o[0] = 2; break;
        case kWindowNoSuchImage: o[0] = 3; break;
        case kWindowNoNormals: o[0] = 4; break;
        case kWindowLabStale: o[0] = 5; break;
        default: o[0] = 0; o[1] = v == kWindowRaw; break;
      }
      break;
    }
    case NORMALS_UPLOADED: r.normals_were_uploaded(); break;
    case SET_PREPROCESS: r.set_processed_depth(in != 0); break;
    case RESIDENT: o[0] = r.resident(); break;
    default: o[0] = raw_depth(*n); break;
  }
}

// ================================================================ the read fences
struct OldFences { bool normals_read_pending, raw_read_pending, products_read_pending; };
enum FenceEvent { POINTS_DRAWN, MVT_DRAWN, WINDOW_DRAWN, RAW_UPLOAD, PROCESS_WAITS, N_FENCE_EVENTS };
static const int fence_inputs[N_FENCE_EVENTS] = {1, 1, 2, 2, 4};
// o[f] = 1: fence f's event recorded on the context's stream / waited for by the lane
static void run_old(OldFences* c, int ev, int in, int* o) {
  switch (ev) {
    case POINTS_DRAWN: o[0] = 1; c->normals_read_pending = true; break;   // tsdf_draw_points (with a normal image, pipelined)
    case MVT_DRAWN: o[1] = 1; c->raw_read_pending = true; break;          // tsdf_draw_mvt (pipelined)
    case WINDOW_DRAWN:                                                    // tsdf_draw_sensor_texture on a product (pipelined); in = type 6
      o[2] = 1; c->products_read_pending = true;
      if (in) { o[1] = 1; c->raw_read_pending = true; }
      break;
    case RAW_UPLOAD:                                                      // wait_raw_read; in = lane != c->stream
      if (!c->raw_read_pending) break;
      if (in) o[1] = 1;
      c->raw_read_pending = false;
      break;
    default:                                                              // process_textures_impl; in = (lane != c->stream) | (phase == 1) << 1
      if (!(in & 2) && c->normals_read_pending) {
        if (in & 1) o[0] = 1;
        c->normals_read_pending = false;
      }
      if (c->products_read_pending) {
        if (in & 1) o[2] = 1;
        c->products_read_pending = false;
      }
      break;
  }
}
static void run_new(ReadFences* f, int ev, int in, int* o) {
  auto record = [&](int k) { f->reader_queued(k); o[k] = 1; };
  auto wait = [&](int k, bool other) { if (f->writer_takes(k, other)) o[k] = 1; };
  switch (ev) {
    case POINTS_DRAWN: record(kNormalsRead); break;
    case MVT_DRAWN: record(kRawRead); break;
    case WINDOW_DRAWN: record(kProductsRead); if (in) record(kRawRead); break;
    case RAW_UPLOAD: wait(kRawRead, in != 0); break;
    default: if (!(in & 2)) wait(kNormalsRead, (in & 1) != 0); wait(kProductsRead, (in & 1) != 0); break;
  }
}
static OldFences old_fences(int s) { return OldFences{(s & 1) != 0, (s & 2) != 0, (s & 4) != 0}; }
static ReadFences new_fences(int s) { ReadFences f; for (int k = 0; k < 3; ++k) f.pending[k] = (s >> k) & 1; return f; }
static int index_of(const ReadFences& f) { return f.pending[0] | (f.pending[1] << 1) | (f.pending[2] << 2); }
static bool same(const OldFences& c, const ReadFences& f) { return c.normals_read_pending == f.pending[0] && c.raw_read_pending == f.pending[1] && c.products_read_pending == f.pending[2]; }

template <class Old, class New, class MakeOld, class MakeNew> static void product(const char* part, int states, int events, const int* inputs, MakeOld make_old, MakeNew make_new) {
  for (int s = 0; s < states; ++s) for (int ev = 0; ev < events; ++ev) for (int in = 0; in < inputs[ev]; ++in) {
    New n = make_new(s);
    Old c = make_old(s);
    int want[kOut], got[kOut];
    for (int k = 0; k < kOut; ++k) want[k] = got[k] = -1;
    run_old(&c, ev, in, want);
    run_new(&n, ev, in, got);
    ++rows;
    const bool fields = same(c, n);
    if (!fields || std::memcmp(want, got, sizeof(want)) != 0) mismatch(part, s, ev, in, got, want, fields);
  }
}

int main() {
  // ---- the full products
  { const FrameSlots fresh; const OldSlots was = old_slots(0); if (index_of(fresh) != 0 || !same(was, fresh)) violated("the slots' initial state", 0, -1, 0); }
  product<OldSlots, FrameSlots>("slots", kSlotStates, N_SLOT_EVENTS, slot_inputs, old_slots, new_slots);
  product<OldRaw, NewRaw>("raw", kRawStates, N_RAW_EVENTS, raw_inputs, [](int s) { return old_raw(new_raw(s)); }, new_raw);
  product<OldFences, ReadFences>("fences", 8, N_FENCE_EVENTS, fence_inputs, old_fences, new_fences);
  for (int s = 0; s < kSlotStates; ++s) if (index_of(new_slots(s)) != s) violated("the slots' packing", s, -1, 0);
  for (int s = 0; s < kRawStates; ++s) if (index_of(new_raw(s)) != s) violated("the raw frame's packing", s, -1, 0);
  std::printf("rows %ld\nmismatches %ld\n", rows, mismatches);

  // ---- breadth-first from a context just created, each part with a shadow kept from what its transitions hand back
  // the fences: fresh[f] = fence f was recorded and no writer has taken it since.  A lane is told to wait exactly when the writer is on another
  // stream and the fence is fresh: at most one wait per record, and none missed
  long fence_states = 0, fence_waits = 0;
  {
    std::vector<unsigned char> seen(64, 0);
    std::vector<int> frontier;
    seen[0] = 1; frontier.push_back(index_of(ReadFences()) * 8);
    while (!frontier.empty()) {
      const int key = frontier.back(); frontier.pop_back(); ++fence_states;
      for (int ev = 0; ev < N_FENCE_EVENTS; ++ev) for (int in = 0; in < fence_inputs[ev]; ++in) {
        ReadFences f = new_fences(key / 8);
        int fresh = key % 8, o[kOut] = {-1, -1, -1};
        run_new(&f, ev, in, o);
        const bool writer = ev >= RAW_UPLOAD, other = (in & 1) != 0;
        for (int k = 0; k < 3; ++k) {
          const bool takes = writer && (ev == RAW_UPLOAD ? k == kRawRead : (k == kProductsRead || (k == kNormalsRead && !(in & 2))));
          if (!writer && o[k] == 1) fresh |= 1 << k;
          if (takes) {
            if ((o[k] == 1) != (other && ((fresh >> k) & 1))) violated("a fence waited for twice, or not at all", key, ev, in);
            if (o[k] == 1) ++fence_waits;
            fresh &= ~(1 << k);
          } else if (writer && o[k] == 1) violated("a wait for a fence the writer does not take", key, ev, in);
        }
        const int t = index_of(f) * 8 + fresh;
        if (!seen[t]) { seen[t] = 1; frontier.push_back(t); }
      }
    }
  }
  // the slots: unawaited[k] = a copy out of staging buffer k was queued and the host has not waited for stage_done[k] since: the buffer is never
  // handed out without that wait.  done = the passes completed after the last raw upload; moved = another slot became current since the last raw
  // upload (the lane's flip, an explicit selection).  A frame of kind "raw, processed" -- what a window verdict of that kind needs -- implies
  // done, as long as the slot stayed: the kind is the SLOT's history, so behind a flip or a selection it speaks of the frame that slot holds
  // (kept as found; `stale` counts those states)
  long slot_states = 0, slot_keys = 0, staging_waits = 0, raw_done = 0, stale = 0;
  {
    enum Site { PRE_UPLOAD, RAW_UPLOADED, PROCESSED, FRAME_STAGING, ASYNC, SELECTED, N_SITES };
    const int site_inputs[N_SITES] = {2, 2, 4, 1, 1, 4};                   // flip; flip; flip | (phase == 1) << 1; -; -; slot | events << 1
    std::vector<unsigned char> seen((size_t)kSlotStates * 16, 0), seen_state(kSlotStates, 0);
    std::vector<int> frontier;
    frontier.push_back(index_of(FrameSlots()) * 16); seen[frontier[0]] = 1;
    while (!frontier.empty()) {
      const int key = frontier.back(); frontier.pop_back(); ++slot_keys;
      const int s = key / 16;
      if (!seen_state[s]) { seen_state[s] = 1; ++slot_states; }
      {
        const FrameSlots f = new_slots(s);
        const bool done = key & 4, moved = key & 8;
        if (f.kind() == kFrameRawDone) { ++raw_done; if (!done && !moved) violated("a frame of kind 'raw, processed' with no process behind the last raw upload", s, -1, 0); if (!done) ++stale; }
      }
      for (int site = 0; site < N_SITES; ++site) for (int in = 0; in < site_inputs[site]; ++in) {
        FrameSlots f = new_slots(s);
        int unawaited = key & 3; bool done = key & 4, moved = key & 8;
        auto flip = [&] { if (in & 1) { f.made_current(f.current() ^ 1); moved = true; } };
        auto staging = [&] {
          const FrameSlots::Staging G = f.staging();
          if (((unawaited >> G.index) & 1) && !G.wait) violated("a staging buffer handed out while its copy is unawaited", s, site, in);
          if (G.wait) { ++staging_waits; unawaited &= ~(1 << G.index); }
          return G.index;
        };
        switch (site) {
          case PRE_UPLOAD: flip(); f.preprocessed_written(); break;
          case RAW_UPLOADED: flip(); f.raw_arrived(); done = false; moved = false; break;
          case PROCESSED: flip(); if (!(in & 2)) { f.passes_completed(); done = true; } break;
          case FRAME_STAGING: staging(); break;
          case ASYNC: {
            const int k = staging(), cur = f.current();
            const FrameSlots::Async A = f.async_queued();
            if (A.staging != k || A.slot != (cur ^ 1) || f.current() != cur) violated("the asynchronous upload's buffer or slot", s, site, in);
            unawaited |= 1 << k;
            break;
          }
          default: {
            const int cur = f.current();
            const FrameSlots::Select T = f.select(in & 1, (in & 2) != 0);
            if (T.record_released && (in & 1) == cur) violated("`released` recorded for a slot that stays current", s, site, in);
            f.made_current(in & 1);
            if ((in & 1) != cur) moved = true;
            break;
          }
        }
        const int t = index_of(f) * 16 + unawaited + (done ? 4 : 0) + (moved ? 8 : 0);
        if (!seen[t]) { seen[t] = 1; frontier.push_back(t); }
      }
    }
  }
  // the raw frame: unawaited[k] = a copy out of pinned buffer k was queued and the host has not waited for wire_done[k] since (a wait for the
  // streams at a reallocation counts): no message takes the buffer without that wait.  The generations are compared for equality alone and the
  // second is only ever set to the first, so the walk keeps them as 0 / 0 or 1 / 0
  long raw_states = 0, wire_waits = 0;
  {
    std::vector<unsigned char> seen((size_t)kRawStates * 4, 0);
    std::vector<int> frontier;
    { NewRaw n; n.raw_src = kNull; n.pending_rgb = kStageCol; frontier.push_back(index_of(n) * 4); seen[frontier[0]] = 1; }
    while (!frontier.empty()) {
      const int key = frontier.back(); frontier.pop_back(); ++raw_states;
      for (int ev = 0; ev < N_RAW_EVENTS; ++ev) for (int in = 0; in < raw_inputs[ev]; ++in) {
        NewRaw n = new_raw(key / 4);
        int unawaited = key % 4, o[kOut] = {-1, -1, -1};
        run_new(&n, ev, in, o);
        if (ev == UPLOAD_WIRE) {
          if (((unawaited >> o[0]) & 1) && o[1] != 1) violated("a pinned wire buffer taken while its copy is unawaited", key, ev, in);
          if (o[1] == 1) ++wire_waits;
          unawaited |= 1 << o[0];
        }
        if (ev == WIRE_REALLOC) unawaited = 0;
        if (n.raw.pre_generation > n.raw.raw_generation) violated("the passes ran on a raw upload that has not happened", key, ev, in);
        const bool newer = n.raw.pre_generation != n.raw.raw_generation;
        n.raw.pre_generation = 0; n.raw.raw_generation = newer ? 1 : 0;
        const int t = index_of(n) * 4 + unawaited;
        if (!seen[t]) { seen[t] = 1; frontier.push_back(t); }
      }
    }
  }
  std::printf("fence_states %ld\nfence_waits %ld\nslot_states %ld\nslot_keys %ld\nstaging_waits %ld\nraw_done %ld\nstale %ld\nraw_states %ld\nwire_waits %ld\nviolations %ld\n",
              fence_states, fence_waits, slot_states, slot_keys, staging_waits, raw_done, stale, raw_states, wire_waits, violations);
  return 0;
}
"""


def build(d, name, *flags):
    src, exe = str(d / "frame_intake_walk.cpp"), str(d / name)
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC, src, "-o", exe])
    return exe


def counts(text):
    return {k: int(v) for k, v in re.findall(r"^(\w+) (\d+)$", text, re.M)}


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    text = subprocess.check_output([build(tmp_path_factory.mktemp("frame_intake"), "frame_intake_walk", "-O2")]).decode()
    return text, counts(text)


def test_program_and_table_agree_on_the_events():
    """the program's event lists are the ones the row count below is computed from"""
    for enum, array, table in (("SlotEvent", "slot_inputs", SLOT_EVENTS), ("RawEvent", "raw_inputs", RAW_EVENTS), ("FenceEvent", "fence_inputs", FENCE_EVENTS)):
        names = re.search(r"enum %s \{(.*?), N_\w+ \}" % enum, PROGRAM, re.S).group(1)
        inputs = re.search(r"%s\[N_\w+\] = \{(.*?)\}" % array, PROGRAM).group(1)
        assert len(names.split(",")) == len(table)
        assert [int(n) for n in inputs.split(",")] == list(table.values())


def test_every_transition_is_abi_cpp_as_it_stood(walk):
    text, n = walk
    assert (SLOT_STATES, RAW_STATES, FENCE_STATES) == (16384, 13824, 8)
    want = SLOT_STATES * sum(SLOT_EVENTS.values()) + RAW_STATES * sum(RAW_EVENTS.values()) + FENCE_STATES * sum(FENCE_EVENTS.values())
    assert n["rows"] == want                                                # the full products: every state, event and input
    print("rows:", n["rows"])
    assert n["mismatches"] == 0, text


def test_what_the_protocol_promises(walk):
    """On the full product: a window verdict of "raw, processed" is given for a frame of that kind alone.  On the reachable states, against
    shadows kept from the returned values: a lane is told to wait for a read fence exactly when it is another stream's and the fence was
    recorded since a writer last took it -- at most once per record; a staging buffer is never handed out, and a pinned wire buffer never
    taken, while a copy out of it is unawaited; a frame of kind "raw, processed" means that the passes completed behind the last raw upload,
    as long as the same slot stayed current (behind the lane's flip or an explicit selection the kind speaks of the frame that slot holds:
    kept as found, and the walk counts those states)."""
    text, n = walk
    assert n["violations"] == 0, text
    print(text)
    assert n["fence_states"] == 8 and n["fence_waits"] > 0
    assert 1 < n["slot_states"] < SLOT_STATES and n["slot_states"] <= n["slot_keys"] and n["staging_waits"] > 0
    assert 0 < n["stale"] < n["raw_done"]
    assert 1 < n["raw_states"] and n["wire_waits"] > 0


def test_the_walk_runs_clean_under_the_sanitizers(tmp_path_factory, walk):
    """the same program as an executable of its own with AddressSanitizer and UndefinedBehaviorSanitizer: same output, nothing reported"""
    exe = build(tmp_path_factory.mktemp("frame_intake_san"), "frame_intake_walk_san", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()
    assert r.stdout.decode() == walk[0]
