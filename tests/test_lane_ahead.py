"""csrc/lane_ahead.hpp: the lane ahead's frame bookkeeping as one state machine, for every combination of its 20 state fields (2^20 states),
every event, and every combination of the event's boolean inputs, against a restatement of the statements abi.cpp held at each of those
places before the header existed -- written over the 20 loose fields tsdf_ctx had then, with every HIP call replaced by a value handed back.
Then a breadth-first walk from the initial state: what the protocol promises on every state the events can reach.  The header is host-only
and free of HIP, so a plain g++ builds the walk; 33 million rows are too many to ship, so the program compares them itself and prints the
number of rows it walked and what did not match."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbd-recon_amd", "csrc")

# the 20 fields: 16 booleans and four 0 / 1 indices
STATE = ("pipeline_blocked", "main_since_gate", "pre_gate_recorded", "gate_flip", "gate_wait_pending", "gate_wait_ev", "pre_pending",
         "slot_flipped", "slot_in_use", "counters_flipped", "counters_in_use", "counters_cur", "counters_zeroed", "spare_clean",
         "occ_flipped", "occ_in_use", "occ_parity", "occ_count_zeroed", "occ_zeroed_word", "occ_counts_stale")
# events and the number of boolean inputs of each
N_INPUTS = dict(pipelined=1, lane_unavailable=0, pre_enter=2, gate_now=0, pre_leave=1, join_pre=0, integrate_deep=0, block_pipeline=0, sync_ctx=1,
                setup_bricks=0, counters_for_upload=2, begin_slot_write=1, clear_bricks=1, mark_bricks=1, update_occupied=1, classify_zero=2)

PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "lane_ahead.hpp"
using rr::LaneAhead;

// ---- tsdf_ctx as it stood: the 20 loose fields.  The two gate events travel as indices (pre_gate = 0, pre_gate_b = 1), and br_counters is
// the index of the buffer c->br.counters pointed at
struct Old {
  bool pipeline_blocked, main_since_gate, pre_gate_recorded, gate_flip, gate_wait_pending; int gate_wait_ev; bool pre_pending;
  bool slot_flipped, slot_in_use, counters_flipped, counters_in_use; int counters_cur; bool counters_zeroed, spare_clean;
  bool occ_flipped, occ_in_use; int occ_parity; bool occ_count_zeroed; int occ_zeroed_word; bool occ_counts_stale;
  int br_counters;
};
static const int kFields = 20, kOut = 6;
static void unpack(unsigned s, int* f) { for (int k = 0; k < kFields; ++k) f[k] = (s >> k) & 1; }
static Old old_of(const int* f) {
  Old c{};
  c.pipeline_blocked = f[0]; c.main_since_gate = f[1]; c.pre_gate_recorded = f[2]; c.gate_flip = f[3]; c.gate_wait_pending = f[4]; c.gate_wait_ev = f[5]; c.pre_pending = f[6];
  c.slot_flipped = f[7]; c.slot_in_use = f[8]; c.counters_flipped = f[9]; c.counters_in_use = f[10]; c.counters_cur = f[11]; c.counters_zeroed = f[12]; c.spare_clean = f[13];
  c.occ_flipped = f[14]; c.occ_in_use = f[15]; c.occ_parity = f[16]; c.occ_count_zeroed = f[17]; c.occ_zeroed_word = f[18]; c.occ_counts_stale = f[19];
  c.br_counters = c.counters_cur;
  return c;
}
static unsigned pack(const Old& c) {
  const int f[kFields] = {c.pipeline_blocked, c.main_since_gate, c.pre_gate_recorded, c.gate_flip, c.gate_wait_pending, c.gate_wait_ev, c.pre_pending,
                          c.slot_flipped, c.slot_in_use, c.counters_flipped, c.counters_in_use, c.counters_cur, c.counters_zeroed, c.spare_clean,
                          c.occ_flipped, c.occ_in_use, c.occ_parity, c.occ_count_zeroed, c.occ_zeroed_word, c.occ_counts_stale};
  unsigned s = 0;
  for (int k = 0; k < kFields; ++k) s |= (unsigned)(f[k] & 1) << k;
  return s;
}
static LaneAhead new_of(const int* f) {
  LaneAhead a;
  a.pipeline_blocked = f[0]; a.main_since_gate = f[1]; a.pre_gate_recorded = f[2]; a.gate_flip = f[3]; a.gate_wait_pending = f[4]; a.gate_wait_ev = f[5]; a.pre_pending = f[6];
  a.slot.flipped = f[7]; a.slot.in_use = f[8]; a.counters.flipped = f[9]; a.counters.in_use = f[10]; a.counters_cur = f[11]; a.counters_zeroed = f[12]; a.spare_clean = f[13];
  a.occ.flipped = f[14]; a.occ.in_use = f[15]; a.occ_parity = f[16]; a.occ_count_zeroed = f[17]; a.occ_zeroed_word = f[18]; a.occ_counts_stale = f[19];
  return a;
}
static unsigned pack(const LaneAhead& a) {
  const int f[kFields] = {a.pipeline_blocked, a.main_since_gate, a.pre_gate_recorded, a.gate_flip, a.gate_wait_pending, a.gate_wait_ev, a.pre_pending,
                          a.slot.flipped, a.slot.in_use, a.counters.flipped, a.counters.in_use, a.counters_cur, a.counters_zeroed, a.spare_clean,
                          a.occ.flipped, a.occ.in_use, a.occ_parity, a.occ_count_zeroed, a.occ_zeroed_word, a.occ_counts_stale};
  unsigned s = 0;
  for (int k = 0; k < kFields; ++k) s |= (unsigned)(f[k] & 1) << k;
  return s;
}
static int alt_of(int x) { return x ^ 1; }

enum Event { PIPELINED, LANE_UNAVAILABLE, PRE_ENTER, GATE_NOW, PRE_LEAVE, JOIN_PRE, INTEGRATE_DEEP, BLOCK_PIPELINE, SYNC_CTX, SETUP_BRICKS, COUNTERS_FOR_UPLOAD,
             BEGIN_SLOT_WRITE, CLEAR_BRICKS, MARK_BRICKS, UPDATE_OCCUPIED, CLASSIFY_ZERO, N_EVENTS };
static const int n_inputs[N_EVENTS] = {1, 0, 2, 0, 1, 0, 0, 0, 1, 0, 2, 1, 1, 1, 1, 2};

// ---- abi.cpp as it stood, one function per site.  o[] = what the site did with HIP, in the order it did it (-1 / 0: nothing)
static void old_gate_now(Old* c, int* waited) {
  if (!c->gate_wait_pending) return;
  c->gate_wait_pending = false;
  *waited = c->gate_wait_ev;                                              // hipStreamWaitEvent(c->pre_lane, c->gate_wait_ev, 0)
}
// pre_enter() behind `if (!pipelined(c)) return c->stream;` and with the lane's stream in place.  o = {first call of a frame, wait for the
// deferred gate, wait for the old gate, wait for the integrate lane, gate recorded, gate whose wait was deferred}
static void old_pre_enter(Old* c, bool defer_gate, bool integ_busy, int* o) {
  o[1] = o[2] = o[4] = o[5] = -1;
  if (c->main_since_gate) {
    o[0] = 1;
    const int gate_old = c->gate_flip ? 1 : 0, gate_new = c->gate_flip ? 0 : 1;   // c->gate_flip ? c->pre_gate_b : c->pre_gate, c->gate_flip ? c->pre_gate : c->pre_gate_b
    if (c->gate_wait_pending) { c->gate_wait_pending = false; o[1] = c->gate_wait_ev; }
    if (c->pre_gate_recorded) {
      if (defer_gate) { c->gate_wait_pending = true; c->gate_wait_ev = gate_old; o[5] = gate_old; }
      else o[2] = gate_old;
    }
    if (integ_busy) o[3] = 1;                                             // c->integ_pending && c->integ_stream && c->pre_lane != c->integ_stream: record integ_done, wait for it
    o[4] = gate_new;                                                      // hipEventRecord(gate_new, c->stream)
    c->gate_flip = !c->gate_flip;
    c->pre_gate_recorded = true; c->main_since_gate = false;
    c->slot_flipped = c->counters_flipped = c->occ_flipped = false;
    c->counters_zeroed = c->occ_count_zeroed = false;
  } else if (!defer_gate) old_gate_now(c, &o[1]);
}
static void old_pre_leave(Old* c, bool on_lane) { if (on_lane) c->pre_pending = true; }   // lane != c->stream
// o = {deferred gate waited for, pre_done recorded and waited for}
static void old_join_pre(Old* c, int* o) {
  o[0] = -1;
  old_gate_now(c, &o[0]);
  c->main_since_gate = true;
  c->slot_in_use = c->counters_in_use = c->occ_in_use = true;
  if (!c->pre_pending) return;
  c->pre_pending = false;
  o[1] = 1;
}
// the deep branch of tsdf_integrate: o = {-1, pre_done recorded and waited for (else: integ_gate)}
static void old_integrate_deep(Old* c, int* o) {
  o[0] = -1;
  c->main_since_gate = true;
  c->slot_in_use = c->counters_in_use = c->occ_in_use = true;
  if (c->pre_pending) {
    c->pre_pending = false;
    o[1] = 1;
  }
}
// o = {the streams were drained}
static void old_block_pipeline(Old* c, int* o) {
  if (c->pipeline_blocked) return;
  c->pipeline_blocked = true;
  o[0] = 1;
  c->pre_pending = false;
}
static void old_sync_ctx(Old* c, bool have_pre_stream) { if (have_pre_stream) c->pre_pending = false; }
// o = {buffer the bricks use, occupancy set the bricks use}
static void old_setup_bricks(Old* c, int* o) {
  c->counters_cur = 0; c->spare_clean = true;
  c->br_counters = 0;
  c->occ_counts_stale = false;
  o[0] = c->br_counters; o[1] = c->occ_parity;
}
// o = {buffer the re-layout launch clears, or -1}
static void old_counters_for_upload(Old* c, bool on_lane, bool have_buffers, int* o) {
  o[0] = -1;
  if (!on_lane || c->counters_zeroed || !have_buffers) return;           // lane == c->stream || c->counters_zeroed || !c->d_counters[0]
  if (!c->counters_flipped && c->counters_in_use) { c->counters_cur = alt_of(c->counters_cur); c->br_counters = c->counters_cur; }
  c->counters_flipped = true; c->counters_in_use = false; c->counters_zeroed = true; c->spare_clean = false;
  o[0] = c->br_counters;
}
// o = {the other slot is allocated, given the colour, made current}
static void old_begin_slot_write(Old* c, bool on_lane, int* o) {
  if (!on_lane || c->slot_flipped) return;
  c->slot_flipped = true;
  if (!c->slot_in_use) return;
  c->slot_in_use = false;
  o[0] = 1;
}
// o = {buffer the bricks use, it is filled}
static void old_clear_bricks(Old* c, bool on_lane, int* o) {
  if (on_lane) {
    if (!c->counters_flipped && c->counters_in_use) { c->counters_cur = alt_of(c->counters_cur); c->br_counters = c->counters_cur; }
    c->counters_flipped = true; c->counters_in_use = false;
    c->spare_clean = false;
    if (c->counters_zeroed) c->counters_zeroed = false;
    else o[1] = 1;
  } else if (c->spare_clean) {
    c->counters_cur = alt_of(c->counters_cur);
    c->br_counters = c->counters_cur;
    c->spare_clean = false;
  } else o[1] = 1;
  o[0] = c->br_counters;
}
// o = {count word the marking launch zeroes, or -1}
static void old_mark_bricks(Old* c, bool on_lane, int* o) {
  o[0] = -1;
  if (on_lane) {
    c->occ_zeroed_word = (!c->occ_flipped && c->occ_in_use) ? alt_of(c->occ_parity) : c->occ_parity;
    o[0] = c->occ_zeroed_word;
    c->occ_count_zeroed = true;
  }
}
// o = {occupancy set and count word the bricks use, the word is filled, word the kernel re-arms}
static void old_update_occupied(Old* c, bool on_lane, int* o) {
  if (on_lane) {
    if (!c->occ_flipped && c->occ_in_use) c->occ_parity = alt_of(c->occ_parity);
    c->occ_flipped = true; c->occ_in_use = false; c->occ_counts_stale = true;
    o[0] = c->occ_parity;
    const bool cleared = c->occ_count_zeroed && c->occ_zeroed_word == c->occ_parity;
    c->occ_count_zeroed = false;
    if (!cleared) o[1] = 1;
    o[2] = 2;
  } else {
    c->occ_parity = alt_of(c->occ_parity);
    o[0] = c->occ_parity;
    if (c->occ_counts_stale) {
      o[1] = 1;
      c->occ_counts_stale = false;
    }
    o[2] = alt_of(c->occ_parity);
  }
}
static bool old_pipelined(const Old* c, bool overlap_fill) { return overlap_fill && !c->pipeline_blocked; }
// the classify launch; o = {buffer it zeroes, or -1}.  bricks = c->use_bricks && !c->full_classify
static void old_classify_zero(Old* c, bool bricks, bool overlap_fill, int* o) {
  o[0] = -1;
  if (bricks && !c->spare_clean && !old_pipelined(c, overlap_fill)) {
    o[0] = alt_of(c->counters_cur);
    c->spare_clean = true;
  }
}

static void run_old(Old* c, int ev, const bool* i, int* o) {
  switch (ev) {
    case PIPELINED: o[0] = old_pipelined(c, i[0]); break;
    case LANE_UNAVAILABLE: c->pipeline_blocked = true; break;             // pre_enter: the lane's stream or events could not be created
    case PRE_ENTER: old_pre_enter(c, i[0], i[1], o); break;
    case GATE_NOW: o[0] = -1; old_gate_now(c, &o[0]); break;
    case PRE_LEAVE: old_pre_leave(c, i[0]); break;
    case JOIN_PRE: old_join_pre(c, o); break;
    case INTEGRATE_DEEP: old_integrate_deep(c, o); break;
    case BLOCK_PIPELINE: old_block_pipeline(c, o); break;
    case SYNC_CTX: old_sync_ctx(c, i[0]); break;
    case SETUP_BRICKS: old_setup_bricks(c, o); break;
    case COUNTERS_FOR_UPLOAD: old_counters_for_upload(c, i[0], i[1], o); break;
    case BEGIN_SLOT_WRITE: old_begin_slot_write(c, i[0], o); break;
    case CLEAR_BRICKS: old_clear_bricks(c, i[0], o); break;
    case MARK_BRICKS: old_mark_bricks(c, i[0], o); break;
    case UPDATE_OCCUPIED: old_update_occupied(c, i[0], o); break;
    default: old_classify_zero(c, i[0], i[1], o); break;
  }
}
// ---- the same places as abi.cpp drives the header now
static void run_new(LaneAhead* a, int ev, const bool* i, int* o) {
  switch (ev) {
    case PIPELINED: o[0] = i[0] && !a->blocked(); break;
    case LANE_UNAVAILABLE: a->lane_unavailable(); break;
    case PRE_ENTER:
      o[1] = o[2] = o[4] = o[5] = -1;
      if (a->at_frame_start()) {
        const LaneAhead::Open O = a->open_frame(i[0], i[1]);
        o[0] = 1; o[1] = O.overdue; o[2] = O.wait; o[3] = O.wait_integ; o[4] = O.record; o[5] = O.deferred;
      } else o[1] = a->later_call(i[0]);
      break;
    case GATE_NOW: o[0] = a->take_deferred_gate(); break;
    case PRE_LEAVE: a->call_queued(i[0]); break;
    case JOIN_PRE: o[0] = a->take_deferred_gate(); o[1] = a->consume(); break;
    case INTEGRATE_DEEP: o[0] = -1; o[1] = a->consume(); break;
    case BLOCK_PIPELINE: o[0] = a->block(); break;
    case SYNC_CTX: if (i[0]) a->lane_synchronised(); break;
    case SETUP_BRICKS: a->new_brick_grid(); o[0] = a->counters_buffer(); o[1] = a->occ_set(); break;
    case COUNTERS_FOR_UPLOAD: o[0] = a->counters_for_upload(i[0] && i[1]); break;
    case BEGIN_SLOT_WRITE: o[0] = a->slot_for_write(i[0]); break;
    case CLEAR_BRICKS: { const LaneAhead::Clear C = a->clear_bricks(i[0]); o[0] = C.buffer; o[1] = C.fill; break; }
    case MARK_BRICKS: o[0] = a->mark_bricks(i[0]); break;
    case UPDATE_OCCUPIED: { const LaneAhead::Update U = a->update_occupied(i[0]); o[0] = U.set; o[1] = U.fill; o[2] = U.rearm; break; }
    default: o[0] = a->counters_zero_spare(i[0] && !(i[1] && !a->blocked())); break;
  }
}

static long violations = 0;
static void violated(const char* what, unsigned s, int ev, int in) {
  if (++violations <= 10) std::printf("violated: %s (state %05x, event %d, inputs %d)\n", what, s, ev, in);
}
static unsigned step(unsigned s, int ev, int in, int* o) {
  int f[kFields];
  unpack(s, f);
  LaneAhead a = new_of(f);
  bool i[2] = {(in & 1) != 0, (in & 2) != 0};
  for (int k = 0; k < kOut; ++k) o[k] = 0;
  run_new(&a, ev, i, o);
  return pack(a);
}

int main() {
  // ---- the full product
  long rows = 0, mismatches = 0;
  for (unsigned s = 0; s < (1u << kFields); ++s) {
    int f[kFields];
    unpack(s, f);
    for (int ev = 0; ev < N_EVENTS; ++ev) for (int in = 0; in < (1 << n_inputs[ev]); ++in) {
      const bool i[2] = {(in & 1) != 0, (in & 2) != 0};
      Old c = old_of(f);
      LaneAhead a = new_of(f);
      int want[kOut] = {0, 0, 0, 0, 0, 0}, got[kOut] = {0, 0, 0, 0, 0, 0};
      run_old(&c, ev, i, want);
      run_new(&a, ev, i, got);
      const unsigned t_old = pack(c), t_new = pack(a);
      ++rows;
      if (t_old != t_new || std::memcmp(want, got, sizeof(want)) != 0 || c.br_counters != c.counters_cur) {
        if (++mismatches <= 10) std::printf("mismatch: state %05x event %d inputs %d: next %05x, was %05x; returned %d %d %d %d %d %d, was %d %d %d %d %d %d\n", s, ev, in, t_new, t_old,
                                            got[0], got[1], got[2], got[3], got[4], got[5], want[0], want[1], want[2], want[3], want[4], want[5]);
      }
      // a deferred wait is never dropped: whatever clears it hands it back; whatever does not leaves it as it is.  The gate flips at the first call of a frame only
      if (a.gate_wait_pending ? false : f[4]) {
        const int handed = ev == PRE_ENTER ? got[1] : got[0];
        if (!(ev == PRE_ENTER || ev == GATE_NOW || ev == JOIN_PRE) || handed != f[5]) violated("a deferred gate wait was dropped", s, ev, in);
      }
      if (f[4] && ev == PRE_ENTER && f[1] && got[1] != f[5]) violated("the first call of a frame kept an overdue wait", s, ev, in);
      if (f[4] && a.gate_wait_pending && !(ev == PRE_ENTER && f[1]) && a.gate_wait_ev != f[5]) violated("a pending wait changed its event", s, ev, in);
      if (!(ev == PRE_ENTER && f[1]) && ((int)a.gate_flip != f[3] || (int)a.pre_gate_recorded != f[2])) violated("the gate moved outside the first call of a frame", s, ev, in);
    }
  }
  std::printf("rows %ld\nmismatches %ld\n", rows, mismatches);

  // ---- breadth-first over what the events can reach from a context just created
  std::vector<unsigned char> seen(1u << kFields, 0);
  std::vector<unsigned> frontier;
  {
    int f0[kFields];
    const LaneAhead fresh;
    const unsigned s0 = pack(fresh);
    unpack(s0, f0);
    if (!(fresh.main_since_gate && !fresh.blocked() && s0 == 2u)) violated("the initial state", s0, -1, 0);
    seen[s0] = 1; frontier.push_back(s0);
  }
  long reachable = 0, lane_updates = 0, lane_updates_cleared = 0;
  const int joins[5][2] = {{-1, -1}, {JOIN_PRE, -1}, {INTEGRATE_DEEP, -1}, {JOIN_PRE, INTEGRATE_DEEP}, {INTEGRATE_DEEP, JOIN_PRE}};
  while (!frontier.empty()) {
    const unsigned s = frontier.back();
    frontier.pop_back();
    ++reachable;
    int f[kFields], o[kOut];
    unpack(s, f);
    // a deferred wait exists behind a recorded gate only and names the gate of the PREVIOUS frame's first call, never this frame's (recorded: index gate_flip)
    if (f[4] && !(f[2] && f[5] == (f[3] ^ 1))) violated("a deferred wait that is not the previous frame's gate", s, -1, 0);
    for (int ev = 0; ev < N_EVENTS; ++ev) for (int in = 0; in < (1 << n_inputs[ev]); ++in) {
      const unsigned t = step(s, ev, in, o);
      int g[kFields];
      unpack(t, g);
      if (!seen[t]) { seen[t] = 1; frontier.push_back(t); }
      // the gate waited for (now or deferred) is the one recorded at the previous frame's first lane call, and the other one is recorded now
      if (ev == PRE_ENTER && f[1]) {
        const int waits = o[2] >= 0 ? o[2] : o[5];
        if (f[2] ? waits != f[3] : waits != -1) violated("the gate waited for is not the previous frame's", s, ev, in);
        if (o[4] != (f[3] ^ 1) || o[4] == waits || g[3] != (f[3] ^ 1) || !g[2] || g[1]) violated("the gate recorded", s, ev, in);
        if ((o[2] >= 0 && o[5] >= 0) || ((in & 1) && o[2] >= 0) || (!(in & 1) && o[5] >= 0)) violated("wait now or later", s, ev, in);
        if (o[5] >= 0 && !(g[4] && g[5] == o[5])) violated("the deferred wait is not pending", s, ev, in);
      }
      // a resource the lane is handed for writing is not marked in use
      if (ev == BEGIN_SLOT_WRITE && (in & 1) && !f[7] && g[8]) violated("the slot handed out is in use", s, ev, in);
      if (ev == BEGIN_SLOT_WRITE && o[0] && !(f[8] && !f[7] && (in & 1))) violated("a slot flip nobody needs", s, ev, in);
      if (((ev == COUNTERS_FOR_UPLOAD && o[0] >= 0) || (ev == CLEAR_BRICKS && (in & 1))) && (g[10] || !g[9])) violated("the counters handed out are in use", s, ev, in);
      if (ev == UPDATE_OCCUPIED && (in & 1) && (g[15] || !g[14])) violated("the occupancy set handed out is in use", s, ev, in);
      // ... and alternates at most once per frame of the lane
      if ((ev == COUNTERS_FOR_UPLOAD || ev == CLEAR_BRICKS) && (in & 1) && f[9] && g[11] != f[11]) violated("a second counter flip in one frame", s, ev, in);
      if (ev == UPDATE_OCCUPIED && (in & 1) && f[14] && g[16] != f[16]) violated("a second occupancy flip in one frame", s, ev, in);
      // spare_clean speaks of the buffer NOT in use: never true for the one in use -- a change of buffer voids it (a new grid zeroes both), and the
      // classify launch zeroes the other one
      if (g[11] != f[11] && g[13] && ev != SETUP_BRICKS) violated("spare_clean survived a change of buffer", s, ev, in);
      if (ev == CLASSIFY_ZERO && o[0] >= 0 && (o[0] == g[11] || !g[13] || f[13])) violated("the classify launch zeroes the buffer in use", s, ev, in);
      if (ev == CLEAR_BRICKS && !(in & 1) && !o[1] && !(f[13] && g[11] != f[11])) violated("a clear without a fill and without a clean spare", s, ev, in);
      if (ev == CLEAR_BRICKS && (in & 1) && !o[1] && !f[12]) violated("a clear on the lane without a fill that the upload did not do", s, ev, in);
      // mark then update on the lane, with any consumer joins in between: the zeroed word is the word the update lands on, or the update fills
      if (ev == MARK_BRICKS && (in & 1)) {
        for (const auto& j : joins) {
          unsigned u = t;
          int o2[kOut];
          for (int k = 0; k < 2; ++k) if (j[k] >= 0) u = step(u, j[k], 0, o2);
          step(u, UPDATE_OCCUPIED, 1, o2);
          ++lane_updates;
          if (!o2[1]) ++lane_updates_cleared;
          if (!o2[1] && o2[0] != o[0]) violated("the update trusts a count word the marking launch did not zero", s, ev, in);
        }
      }
    }
  }
  std::printf("reachable %ld\nlane_updates %ld\nlane_updates_cleared %ld\nviolations %ld\n", reachable, lane_updates, lane_updates_cleared, violations);
  return 0;
}
"""


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    d = tmp_path_factory.mktemp("lane_ahead")
    src, exe = str(d / "lane_walk.cpp"), str(d / "lane_walk")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src, "-o", exe])
    text = subprocess.check_output([exe]).decode()
    return text, {k: int(v) for k, v in re.findall(r"^(\w+) (\d+)$", text, re.M)}


def test_program_and_table_agree_on_the_events():
    """the program's event list is the one the row count below is computed from"""
    enum = re.search(r"enum Event \{(.*?)N_EVENTS \}", PROGRAM, re.S).group(1)
    assert [e.strip().lower() for e in enum.split(",") if e.strip()] == list(N_INPUTS)
    counts = re.search(r"n_inputs\[N_EVENTS\] = \{(.*?)\}", PROGRAM).group(1)
    assert [int(x) for x in counts.split(",")] == list(N_INPUTS.values())


def test_every_transition_is_abi_cpp_as_it_stood(walk):
    text, n = walk
    assert len(STATE) == 20
    assert n["rows"] == 2 ** len(STATE) * sum(1 << k for k in N_INPUTS.values())   # the full product: every state, event and input
    assert n["mismatches"] == 0, text


def test_what_the_protocol_promises(walk):
    """on the full product: a pending deferred gate wait is only ever cleared by a transition that returns it, and the gate moves at the first call
    of a frame only.  On the reachable states: the gate waited for is the previous frame's, a resource handed out for writing is not marked in
    use and flips once per frame, spare_clean never speaks of the buffer in use, and after mark then update on the lane -- with any consumer
    joins in between -- the update lands on the zeroed word or fills"""
    text, n = walk
    assert n["violations"] == 0, text
    assert 1 < n["reachable"] < 2 ** len(STATE)
    assert n["lane_updates"] == 5 * n["reachable"]                       # every reachable state: mark on the lane, then each of the five joins
    assert 0 < n["lane_updates_cleared"] < n["lane_updates"]             # both outcomes occur
