"""csrc/draw_lanes.hpp: the integrate lane's and the fill lane's bookkeeping as one state machine, for every combination of its 13 state fields
-- 9 one-bit fields and the four job numbers, opaque tokens from a domain of three values each, so that a transition handing back the wrong
field's number shows: 2^9 x 3^4 = 41 472 states --, every event, every combination of the event's boolean inputs and, where an event stores a
job number, every number to store, against a restatement of the statements abi.cpp held at each of those places before the header existed --
written over the loose fields tsdf_ctx had then, with every HIP call replaced by a value handed back.  Then a breadth-first walk from the
initial state with a shadow that is kept from what the transitions HAND BACK alone (which events were recorded, which fills queued, with which
job): what the protocol promises on every state the events can reach -- 32 256 states, 122 112 with the shadow.  The header is host-only and free
of HIP, so a plain g++ builds the walk; the program compares the rows itself and prints how many it walked and what did not match."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbd-recon_amd", "csrc")

BITS = ("integ_pending", "draw_pending0", "draw_pending1", "draw_unrecorded", "vol_set", "deep_failed", "fill_pending0", "fill_pending1", "atlas_parity")
JOBS = ("fill_job_no0", "fill_job_no1", "draw_wait_job0", "draw_wait_job1")
# events: (boolean inputs, takes a job number to store)
EVENTS = dict(draw_marched=(1, False), fill_colors=(2, True), integrate_deep=(0, False), join_integ=(0, False), integ_busy=(0, False), take_pyramid=(1, False),
              join_fill=(0, False), overlay_rerecord=(1, False), any_fill_pending=(0, False), sync_ctx=(1, False), block_pipeline=(1, False),
              release_volume=(0, False), release_view=(0, False), setup_view=(0, False), alt_set_failed=(0, False), deep_allowed=(0, False))

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <unordered_set>
#include <vector>
#include "draw_lanes.hpp"
using rr::DrawLanes;

// ---- tsdf_ctx as it stood: the loose fields
struct Old {
  bool integ_pending, draw_pending[2], draw_unrecorded; int vol_set; bool deep_failed, fill_pending[2]; int atlas_parity;
  uint64_t fill_job_no[2], draw_wait_job[2];
};
static const int kBits = 9, kJobs = 4, kOut = 7, kStates = (1 << kBits) * 81;
struct Fields { int b[kBits]; int j[kJobs]; };
static Fields unpack(int s) {
  Fields f;
  for (int k = 0; k < kBits; ++k) f.b[k] = (s >> k) & 1;
  int t = s >> kBits;
  for (int k = 0; k < kJobs; ++k) { f.j[k] = t % 3; t /= 3; }
  return f;
}
static int pack(const Fields& f) {
  int s = 0, t = 0;
  for (int k = 0; k < kBits; ++k) s |= (f.b[k] & 1) << k;
  for (int k = kJobs - 1; k >= 0; --k) t = t * 3 + f.j[k];
  return s | (t << kBits);
}
template <class T> static T state_of(const Fields& f) {
  T c{};
  c.integ_pending = f.b[0]; c.draw_pending[0] = f.b[1]; c.draw_pending[1] = f.b[2]; c.draw_unrecorded = f.b[3]; c.vol_set = f.b[4]; c.deep_failed = f.b[5];
  c.fill_pending[0] = f.b[6]; c.fill_pending[1] = f.b[7]; c.atlas_parity = f.b[8];
  c.fill_job_no[0] = f.j[0]; c.fill_job_no[1] = f.j[1]; c.draw_wait_job[0] = f.j[2]; c.draw_wait_job[1] = f.j[3];
  return c;
}
template <class T> static int pack(const T& c) {
  Fields f;
  const int b[kBits] = {c.integ_pending, c.draw_pending[0], c.draw_pending[1], c.draw_unrecorded, c.vol_set, c.deep_failed, c.fill_pending[0], c.fill_pending[1], c.atlas_parity};
  for (int k = 0; k < kBits; ++k) f.b[k] = b[k];
  f.j[0] = (int)c.fill_job_no[0]; f.j[1] = (int)c.fill_job_no[1]; f.j[2] = (int)c.draw_wait_job[0]; f.j[3] = (int)c.draw_wait_job[1];
  return pack(f);
}

enum Event { DRAW_MARCHED, FILL_COLORS, INTEGRATE_DEEP, JOIN_INTEG, INTEG_BUSY, TAKE_PYRAMID, JOIN_FILL, OVERLAY_RERECORD, ANY_FILL_PENDING, SYNC_CTX, BLOCK_PIPELINE,
             RELEASE_VOLUME, RELEASE_VIEW, SETUP_VIEW, ALT_SET_FAILED, DEEP_ALLOWED, N_EVENTS };
static const int n_bools[N_EVENTS] = {1, 2, 0, 0, 0, 1, 0, 1, 0, 1, 1, 0, 0, 0, 0, 0};
static const int takes_job[N_EVENTS] = {0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// ---- abi.cpp as it stood, one function per site.  o[] = what the site did with HIP, in the order it did it (-1: nothing)
// join_fill_of(): o = {fill_done[pyramid] waited for, after wait_issued(job)}
static void old_join_fill_of(Old* c, int pyramid, int* o) {
  if (!c->fill_pending[pyramid]) return;
  c->fill_pending[pyramid] = false;
  o[0] = 1; o[1] = (int)c->fill_job_no[pyramid];                          // c->fill_worker->wait_issued(c->fill_job_no[pyramid]); hipStreamWaitEvent(c->stream, c->fill_done[pyramid], 0)
}
static void old_join_integ(Old* c, int* o) {
  if (!c->integ_pending) return;
  c->integ_pending = false;
  o[0] = 1;                                                               // hipEventRecord(c->integ_done, c->integ_stream); hipStreamWaitEvent(c->stream, c->integ_done, 0)
}
// the deep branch of tsdf_integrate.  o = {draw_done recorded on the context's stream, after wait_issued(job); integ_done joined; the set in use
// after swap_volume_set; draw_done the lane waits for}
static void old_integrate_deep(Old* c, int* o) {
  if (c->draw_unrecorded) {
    o[1] = (int)c->draw_wait_job[c->vol_set];
    o[0] = c->vol_set;
    c->draw_pending[c->vol_set] = true; c->draw_unrecorded = false;
  }
  old_join_integ(c, &o[2]);
  c->vol_set ^= 1;                                                        // swap_volume_set
  o[3] = c->vol_set;
  if (c->draw_pending[c->vol_set]) { o[4] = c->vol_set; c->draw_pending[c->vol_set] = false; }
  c->integ_pending = true;
}
// raymarch_impl.  o = {pyramid of c->atlas and of the fill mask; join of pyramid 0: waited, job; of pyramid 1}
static void old_take_pyramid(Old* c, bool two_pyramids, int* o) {
  if (two_pyramids) {
    const int p = c->atlas_parity ^ 1;
    c->atlas_parity = p;
    old_join_fill_of(c, p, &o[1 + 2 * p]);
  } else { old_join_fill_of(c, 0, &o[1]); old_join_fill_of(c, 1, &o[3]); }
  o[0] = c->atlas_parity;                                                 // RT.fill_mask = c->d_fill_mask[c->atlas_parity]
}
// fill_colors_impl; by_worker = c->fill_thread && !c->timers_on, job = what FillWorker::submit returned.  o = {draw_done recorded, after
// wait_issued(job); pyramid of the tile mask; the job's wait_ev = draw_done[.], its done_ev = fill_done[.]; queued directly: draw_done the fill
// lane waits for, fill_done recorded}
static void old_fill_colors(Old* c, bool overlap_fill, bool by_worker, uint64_t job, int* o) {
  if (overlap_fill) {
    o[1] = (int)c->draw_wait_job[c->vol_set];
    o[0] = c->vol_set;
    c->draw_pending[c->vol_set] = true; c->draw_unrecorded = false;
  }
  o[2] = c->atlas_parity;
  if (overlap_fill && by_worker) {
    o[3] = c->vol_set; o[4] = c->atlas_parity;
    c->fill_job_no[c->atlas_parity] = c->draw_wait_job[c->vol_set] = job;
    c->fill_pending[c->atlas_parity] = true;
    return;
  }
  if (overlap_fill) o[5] = c->vol_set;
  if (overlap_fill) { o[6] = c->atlas_parity; c->fill_pending[c->atlas_parity] = true; }
}
// overlay_rerecord_draw; have = c->integ_stream && c->draw_done[c->vol_set]
static void old_overlay_rerecord(Old* c, bool have, int* o) {
  if (have) {
    o[1] = (int)c->draw_wait_job[c->vol_set];
    o[0] = c->vol_set;
    c->draw_pending[c->vol_set] = true;
  }
}
static void old_sync_ctx(Old* c, bool integ_stream) {
  if (integ_stream) { c->integ_pending = false; c->draw_pending[0] = c->draw_pending[1] = false; }
  c->fill_pending[0] = c->fill_pending[1] = false;
}

static void run_old(Old* c, int ev, const bool* i, uint64_t job, int* o) {
  switch (ev) {
    case DRAW_MARCHED: c->draw_unrecorded = i[0]; break;                  // c->integ_stream != nullptr
    case FILL_COLORS: old_fill_colors(c, i[0], i[1], job, o); break;
    case INTEGRATE_DEEP: old_integrate_deep(c, o); break;
    case JOIN_INTEG: old_join_integ(c, o); break;
    case INTEG_BUSY: o[0] = c->integ_pending; break;                      // pre_enter: c->integ_pending && c->integ_stream && c->pre_lane != c->integ_stream
    case TAKE_PYRAMID: old_take_pyramid(c, i[0], o); break;
    case JOIN_FILL: old_join_fill_of(c, 0, &o[0]); old_join_fill_of(c, 1, &o[2]); break;
    case OVERLAY_RERECORD: old_overlay_rerecord(c, i[0], o); break;
    case ANY_FILL_PENDING: o[0] = c->fill_pending[0] || c->fill_pending[1]; break;
    case SYNC_CTX: old_sync_ctx(c, i[0]); break;
    case BLOCK_PIPELINE: if (i[0]) c->integ_pending = false; break;       // (behind ahead.block(): if (c->integ_stream) { synchronise it; ... })
    case RELEASE_VOLUME: c->deep_failed = false; break;
    case RELEASE_VIEW: c->atlas_parity = 0; break;
    case SETUP_VIEW: c->atlas_parity = 0; c->atlas_parity = 0; break;     // release_view(c), and again beside atlas_color[0]
    case ALT_SET_FAILED: c->deep_failed = true; break;
    default: o[0] = !c->deep_failed; break;                               // deep_ok's term
  }
}
// ---- the same places as abi.cpp drives the header now
static void put(int* o, DrawLanes::FillJoin J) { if (J.wait) { o[0] = 1; o[1] = (int)J.job; } }
static void put(int* o, DrawLanes::DrawEnd D) { o[0] = D.set; o[1] = (int)D.wait_job; }
static void run_new(DrawLanes* l, int ev, const bool* i, uint64_t job, int* o) {
  switch (ev) {
    case DRAW_MARCHED: l->draw_marched(i[0]); break;
    case FILL_COLORS: {
      const int set = l->set(), pyramid = l->pyramid();
      if (i[0]) put(o, l->draw_end());
      o[2] = pyramid;
      if (i[0] && i[1]) { o[3] = set; o[4] = pyramid; l->fill_queued(job); break; }
      if (i[0]) o[5] = set;
      if (i[0]) { o[6] = pyramid; l->fill_queued(); }
      break;
    }
    case INTEGRATE_DEEP: {
      const DrawLanes::Integrate I = l->integrate();
      if (I.record_end) put(o, I.end);
      if (I.join) o[2] = 1;
      o[3] = l->set();
      o[4] = I.wait_draw;
      break;
    }
    case JOIN_INTEG: if (l->join_integ()) o[0] = 1; break;
    case INTEG_BUSY: o[0] = l->integ_in_flight(); break;
    case TAKE_PYRAMID: { const DrawLanes::Pyramid Y = l->take_pyramid(i[0]); o[0] = Y.index; put(&o[1], Y.join[0]); put(&o[3], Y.join[1]); break; }
    case JOIN_FILL: put(&o[0], l->join_fill(0)); put(&o[2], l->join_fill(1)); break;
    case OVERLAY_RERECORD: if (i[0]) put(o, l->draw_end(true)); break;
    case ANY_FILL_PENDING: o[0] = l->any_fill_pending(); break;
    case SYNC_CTX: l->host_synchronised(i[0]); break;
    case BLOCK_PIPELINE: if (i[0]) l->integ_lane_drained(); break;
    case RELEASE_VOLUME: l->volume_released(); break;
    case RELEASE_VIEW: l->view_released(); break;
    case SETUP_VIEW: l->view_released(); break;
    case ALT_SET_FAILED: l->second_set_unavailable(); break;
    default: o[0] = !l->second_set_failed(); break;
  }
}

static long violations = 0;
static void violated(const char* what, int s, int ev, int in) {
  if (++violations <= 10) std::printf("violated: %s (state %05x, event %d, inputs %d)\n", what, s, ev, in);
}
// what an event handed back, in one vocabulary
struct Handed { int record[2] = {-1, -1}; int record_job[2] = {0, 0}; bool integ_joined = false; int taken_set = -1, wait_draw = -1; bool fill_joined[2] = {false, false};
                int fill_join_job[2] = {0, 0}; int pyramid = -1; int fill_queued = -1; bool by_worker = false; };
static Handed handed_of(int ev, const int* o) {
  Handed H;
  int n = 0;
  auto rec = [&](int set, int job) { if (set >= 0) { H.record[n] = set; H.record_job[n] = job; ++n; } };
  if (ev == FILL_COLORS) { rec(o[0], o[1]); H.fill_queued = o[4] >= 0 ? o[4] : o[6]; H.by_worker = o[4] >= 0; }
  if (ev == INTEGRATE_DEEP) { rec(o[0], o[1]); H.integ_joined = o[2] == 1; H.taken_set = o[3]; H.wait_draw = o[4]; }
  if (ev == JOIN_INTEG) H.integ_joined = o[0] == 1;
  if (ev == OVERLAY_RERECORD) rec(o[0], o[1]);
  if (ev == TAKE_PYRAMID || ev == JOIN_FILL) {
    const int* j = ev == TAKE_PYRAMID ? o + 1 : o;
    for (int p = 0; p < 2; ++p) if (j[2 * p] == 1) { H.fill_joined[p] = true; H.fill_join_job[p] = j[2 * p + 1]; }
    if (ev == TAKE_PYRAMID) H.pyramid = o[0];
  }
  return H;
}

int main() {
  // ---- the full product
  long rows = 0, mismatches = 0;
  for (int s = 0; s < kStates; ++s) {
    const Fields f = unpack(s);
    for (int ev = 0; ev < N_EVENTS; ++ev) for (int in = 0; in < (1 << n_bools[ev]); ++in) for (int job = 0; job < (takes_job[ev] ? 3 : 1); ++job) {
      const bool i[2] = {(in & 1) != 0, (in & 2) != 0};
      Old c = state_of<Old>(f);
      DrawLanes l = state_of<DrawLanes>(f);
      int want[kOut], got[kOut];
      for (int k = 0; k < kOut; ++k) want[k] = got[k] = -1;
      run_old(&c, ev, i, (uint64_t)job, want);
      run_new(&l, ev, i, (uint64_t)job, got);
      const int t_old = pack(c), t_new = pack(l);
      ++rows;
      if (t_old != t_new || std::memcmp(want, got, sizeof(want)) != 0) {
        if (++mismatches <= 10) std::printf("mismatch: state %05x event %d inputs %d job %d: next %05x, was %05x; returned %d %d %d %d %d %d %d, was %d %d %d %d %d %d %d\n", s, ev, in, job, t_new, t_old,
                                            got[0], got[1], got[2], got[3], got[4], got[5], got[6], want[0], want[1], want[2], want[3], want[4], want[5], want[6]);
      }
      // no transition drops a pending flag without handing back the corresponding wait (or, for a draw's end, its record); a wait of the host for
      // the streams is the exception, and so is a march on a context without an integrate lane, whose draws' ends nobody waits for
      const Handed H = handed_of(ev, got);
      const Fields g = unpack(t_new);
      const bool host_integ = (ev == SYNC_CTX || ev == BLOCK_PIPELINE) && i[0];
      if (f.b[0] && !g.b[0] && !(H.integ_joined || host_integ)) violated("integ_pending dropped", s, ev, in);
      if (f.b[0] && ev == INTEGRATE_DEEP && !H.integ_joined) violated("integ_pending dropped", s, ev, in);
      for (int k = 0; k < 2; ++k) {
        if (f.b[1 + k] && !g.b[1 + k] && !(H.wait_draw == k || (ev == SYNC_CTX && i[0]))) violated("draw_pending dropped", s, ev, in);
        if (f.b[6 + k] && !g.b[6 + k] && !((H.fill_joined[k] && H.fill_join_job[k] == f.j[k]) || ev == SYNC_CTX)) violated("fill_pending dropped", s, ev, in);
      }
      if (f.b[3] && !g.b[3] && !(H.record[0] == f.b[4] || (ev == DRAW_MARCHED && !i[0]))) violated("draw_unrecorded dropped", s, ev, in);
    }
  }
  std::printf("rows %ld\nmismatches %ld\n", rows, mismatches);

  // ---- breadth-first over what the events can reach from a context just created, with a shadow kept from what the transitions hand back:
  // recorded[s]: draw_done[s] was recorded and no integrate has been told to wait for it since, nor has the host waited for the integrate lane;
  // job_on_set[s]: the latest hole filling handed to the worker against set s; queued[p] / by_worker[p] / job_on_pyramid[p]: a hole filling of
  // pyramid p was queued and nobody has been told to join it since, nor has the host waited
  struct Shadow { int recorded[2], job_on_set[2], queued[2], by_worker[2], job_on_pyramid[2]; };
  auto pack_shadow = [](const Shadow& h) {
    int k = 0;
    for (int s = 0; s < 2; ++s) k = k * 2 + h.recorded[s];
    for (int s = 0; s < 2; ++s) k = k * 3 + h.job_on_set[s];
    for (int p = 0; p < 2; ++p) { k = k * 2 + h.queued[p]; k = k * 2 + h.by_worker[p]; k = k * 3 + h.job_on_pyramid[p]; }
    return k;
  };
  auto unpack_shadow = [](int k) {
    Shadow h;
    for (int p = 1; p >= 0; --p) { h.job_on_pyramid[p] = k % 3; k /= 3; h.by_worker[p] = k % 2; k /= 2; h.queued[p] = k % 2; k /= 2; }
    for (int s = 1; s >= 0; --s) { h.job_on_set[s] = k % 3; k /= 3; }
    for (int s = 1; s >= 0; --s) { h.recorded[s] = k % 2; k /= 2; }
    return h;
  };
  const int kShadows = 4 * 9 * 12 * 12;
  std::unordered_set<long> seen;
  std::vector<unsigned char> seen_state(kStates, 0);
  std::vector<long> frontier;
  {
    const DrawLanes fresh;
    const int s0 = pack(fresh);
    if (s0 != 0) violated("the initial state", s0, -1, 0);
    seen.insert((long)s0 * kShadows); frontier.push_back((long)s0 * kShadows);
  }
  long reachable = 0, reachable_states = 0, integrates_waiting = 0, integrates = 0, pyramids_joining = 0, pyramids = 0, records = 0;
  while (!frontier.empty()) {
    const long key = frontier.back();
    frontier.pop_back();
    ++reachable;
    const int s = (int)(key / kShadows);
    if (!seen_state[s]) { seen_state[s] = 1; ++reachable_states; }
    const Shadow h = unpack_shadow((int)(key % kShadows));
    const Fields f = unpack(s);
    for (int ev = 0; ev < N_EVENTS; ++ev) for (int in = 0; in < (1 << n_bools[ev]); ++in) for (int job = 0; job < (takes_job[ev] ? 3 : 1); ++job) {
      const bool i[2] = {(in & 1) != 0, (in & 2) != 0};
      DrawLanes l = state_of<DrawLanes>(f);
      int o[kOut];
      for (int k = 0; k < kOut; ++k) o[k] = -1;
      run_new(&l, ev, i, (uint64_t)job, o);
      const Handed H = handed_of(ev, o);
      Shadow g = h;
      // every returned "record draw_done[s]" carries the job number of the latest hole filling queued against s
      for (int n = 0; n < 2; ++n) if (H.record[n] >= 0) {
        ++records;
        if (H.record_job[n] != g.job_on_set[H.record[n]]) violated("a draw's end recorded behind another job than the latest of its set", s, ev, in);
        g.recorded[H.record[n]] = 1;
      }
      // an integrate that takes set s for writing is told to wait for draw_done[s] whenever a draw's end was recorded on s
      if (ev == INTEGRATE_DEEP) {
        ++integrates;
        if (H.taken_set != (f.b[4] ^ 1) || l.set() != H.taken_set) violated("the integrate does not take the other set", s, ev, in);
        if (g.recorded[H.taken_set] ? H.wait_draw != H.taken_set : H.wait_draw != -1) violated("the integrate's wait for the draw that read its set", s, ev, in);
        if (H.wait_draw >= 0) ++integrates_waiting;
        g.recorded[H.taken_set] = 0;
        if (!l.integ_in_flight()) violated("an integrate that is not in flight", s, ev, in);
      }
      // a draw that takes pyramid p is told to join p's fill iff one is pending (with one pyramid: every fill), behind the job that records its event
      if (ev == TAKE_PYRAMID) {
        ++pyramids;
        if (H.pyramid != (i[0] ? f.b[8] ^ 1 : f.b[8]) || l.pyramid() != H.pyramid) violated("the pyramid taken", s, ev, in);
        if (H.fill_joined[H.pyramid] != (g.queued[H.pyramid] != 0)) violated("the draw's join of its pyramid's fill", s, ev, in);
        if (!i[0] && H.fill_joined[H.pyramid ^ 1] != (g.queued[H.pyramid ^ 1] != 0)) violated("one pyramid: the draw's join of the other fill", s, ev, in);
        if (i[0] && H.fill_joined[H.pyramid ^ 1]) violated("two pyramids: a join of the other pyramid's fill", s, ev, in);
        if (H.fill_joined[H.pyramid]) ++pyramids_joining;
      }
      for (int p = 0; p < 2; ++p) if (H.fill_joined[p]) {
        if (!g.queued[p]) violated("a join of a fill nobody queued", s, ev, in);
        if (g.by_worker[p] && H.fill_join_job[p] != g.job_on_pyramid[p]) violated("a fill joined behind another job than the one that records its event", s, ev, in);
        g.queued[p] = 0;
      }
      if (ev == JOIN_FILL && (l.any_fill_pending() || g.queued[0] || g.queued[1])) violated("join_fill left a fill", s, ev, in);
      if (H.fill_queued >= 0) {
        if (H.fill_queued != f.b[8]) violated("a fill queued on another pyramid than the draw's", s, ev, in);
        g.queued[H.fill_queued] = 1; g.by_worker[H.fill_queued] = H.by_worker;
        if (H.by_worker) { g.job_on_pyramid[H.fill_queued] = job; g.job_on_set[f.b[4]] = job; }
      }
      if (ev == SYNC_CTX) { g.queued[0] = g.queued[1] = 0; if (i[0]) g.recorded[0] = g.recorded[1] = 0; }
      if (ev == ANY_FILL_PENDING && o[0] != (h.queued[0] || h.queued[1])) violated("any_fill_pending", s, ev, in);
      const long t = (long)pack(l) * kShadows + pack_shadow(g);
      if (seen.insert(t).second) frontier.push_back(t);
    }
  }
  std::printf("reachable %ld\nreachable_states %ld\nintegrates %ld\nintegrates_waiting %ld\npyramids %ld\npyramids_joining %ld\nrecords %ld\nviolations %ld\n",
              reachable, reachable_states, integrates, integrates_waiting, pyramids, pyramids_joining, records, violations);
  return 0;
}
"""


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    d = tmp_path_factory.mktemp("draw_lanes")
    src, exe = str(d / "draw_lanes_walk.cpp"), str(d / "draw_lanes_walk")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", CSRC, src, "-o", exe])
    text = subprocess.check_output([exe]).decode()
    return text, {k: int(v) for k, v in re.findall(r"^(\w+) (\d+)$", text, re.M)}


def test_program_and_table_agree_on_the_events():
    """the program's event list is the one the row count below is computed from"""
    enum = re.search(r"enum Event \{(.*?)N_EVENTS \}", PROGRAM, re.S).group(1)
    assert [e.strip().lower() for e in enum.split(",") if e.strip()] == list(EVENTS)
    bools = re.search(r"n_bools\[N_EVENTS\] = \{(.*?)\}", PROGRAM).group(1)
    jobs = re.search(r"takes_job\[N_EVENTS\] = \{(.*?)\}", PROGRAM).group(1)
    assert [(int(b), bool(int(j))) for b, j in zip(bools.split(","), jobs.split(","))] == list(EVENTS.values())


def test_every_transition_is_abi_cpp_as_it_stood(walk):
    text, n = walk
    states = 2 ** len(BITS) * 3 ** len(JOBS)
    assert states == 41472
    assert n["rows"] == states * sum((1 << b) * (3 if j else 1) for b, j in EVENTS.values())   # the full product: every state, event, input and job number
    assert n["mismatches"] == 0, text


def test_what_the_protocol_promises(walk):
    """on the full product: no transition drops integ_pending, draw_pending[s], fill_pending[p] or draw_unrecorded without handing back the
    wait (for the last: the record) that goes with it, a fill's with the job number stored for its pyramid; the host's waits are the exception.
    On the reachable states, against a shadow kept from the returned values alone: an integrate takes the other set and is told to wait for
    draw_done of that set whenever a draw's end was recorded on it since the host last waited for the lane (and no integrate has waited for it
    since); every record of draw_done[s] comes with the job number of the latest hole filling the worker was handed against s; a draw that
    takes pyramid p is told to join p's fill iff one is pending -- every fill with one pyramid, never the other's with two --, behind the job
    that records its event; join_fill leaves none"""
    text, n = walk
    assert n["violations"] == 0, text
    assert 1 < n["reachable_states"] < 41472 and n["reachable_states"] <= n["reachable"]
    print("reachable:", n["reachable_states"], "states,", n["reachable"], "with the shadow")
    assert n["integrates"] == n["reachable"] and 0 < n["integrates_waiting"] < n["integrates"]       # both outcomes occur
    assert n["pyramids"] == 2 * n["reachable"] and 0 < n["pyramids_joining"] < n["pyramids"]
    assert n["records"] > n["reachable"]
