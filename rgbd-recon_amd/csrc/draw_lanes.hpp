// The integrate lane's and the fill lane's bookkeeping: the two lanes that run beside the draw on the context's stream, and the two things that
// alternate under them -- the volume sets and the pyramids.  Host only, free of HIP: the state and one named transition per event, handing back
// plain values (booleans, 0 / 1 indices into draw_done[], fill_done[], the volume sets and the pyramids, job numbers of the fill worker; -1 =
// none).  Streams, events, device pointers, allocations, the worker thread and the launches stay in abi.cpp, which acts on what a transition
// returns.  tests/test_draw_lanes.py walks every state, event and input on a CPU.
//
// Stage overlap (round 3): the hole filling of draw f runs on a stream of its own beside whatever the caller queues next -- the brick passes and
// the integrate of frame f + 1 do not touch the pyramid or the framebuffer --, tied to the context's stream by two events: draw_done[set] (the
// fill waits for the march) and fill_done[pyramid] (the next writer / reader of the pyramid or the framebuffer waits for it: join_fill).  Two
// pyramids alternate while that is on: a draw takes the other one and only has to wait for the hole filling of the draw BEFORE the previous
// one -- long finished -- instead of the previous draw's (take_pyramid).
//
// The fill lane's calls are ISSUED by a helper thread (abi.cpp: FillWorker): issuing a c2 frame costs the calling thread ~100 us of HIP runtime
// calls -- as long as the device needs for the frame --, 28 of them for the hole filling's 6 launches and 2 event operations, and nothing the
// caller does next depends on them having been issued.  fillColors() records draw_done on the context's stream itself and hands the rest over
// as a job; whoever needs fill_done[p] first waits (host side, spinning) until the helper has issued that job's record: the job number travels
// with every join.  And whoever records draw_done[set] AGAIN first waits until the job that waits for its previous record has issued that wait
// (DrawEnd::wait_job).  Off while timers are on (their bookkeeping is the caller's thread's) and with RR_FILL_THREAD=0: fill_queued().
//
// ... and a fourth lane (round 3): integrate() of frame f + 1 beside the draw of frame f on the context's stream.  Everything integrate() writes
// and the draw reads exists twice and alternates per integrate() (here the index of the set in use, which abi.cpp binds: bind_volume_set; what a
// set remembers from one integrate() to the next: volume_sets.hpp), and each set evolves exactly like the single volume of rounds 1 / 2, seeing
// every other frame (the reference rebuilds the TSDF from scratch every frame, recon_integration.cpp:249-250: no state is carried from frame to
// frame).  Events: integ_done (the draw waits for its integrate: join_integ),
// draw_done[set] (recorded behind the draw that read the set -- by fillColors(), else by the next integrate(), and again behind an overlay or
// the mesh stream, which read the set after fillColors() --: the hole filling waits for it, and so does the integrate two frames later that
// overwrites the set).
#pragma once
#include <cstdint>

namespace rr {

struct DrawLanes {
  // ---- state (abi.cpp goes through the transitions and the accessors below)
  bool integ_pending = false;                   // the integrate lane holds an integrate() nobody has waited for
  bool draw_pending[2] = {false, false};        // draw_done[set] has been recorded since the host last waited for the integrate lane
  bool draw_unrecorded = false;                 // a draw has marched and draw_done[set] has not been recorded behind it
  int vol_set = 0;                              // the volume set in use
  bool deep_failed = false;                     // no memory for the second set: one volume, no integrate lane
  bool fill_pending[2] = {false, false};        // (per pyramid) a hole filling nobody has waited for
  uint64_t fill_job_no[2] = {0, 0};             // (per pyramid) the worker's job that records fill_done[p]
  uint64_t draw_wait_job[2] = {0, 0};           // (per set) the worker's job that waits for draw_done[set]
  int atlas_parity = 0;                         // the pyramid the latest draw took

  // ---- read only
  int set() const { return vol_set; }
  int pyramid() const { return atlas_parity; }
  bool second_set_failed() const { return deep_failed; }
  bool integ_in_flight() const { return integ_pending; }   // (LaneAhead::open_frame's integ_busy, with what abi.cpp knows of the streams)
  bool any_fill_pending() const { return fill_pending[0] || fill_pending[1]; }

  // ---- the draw's end on the set in use
  // a draw has marched; with an integrate lane its end has to be recorded (by fillColors(), or by the next integrate())
  void draw_marched(bool integ_lane) { draw_unrecorded = integ_lane; }
  // Record draw_done[set] on the context's stream, behind whatever last read the set: first wait until the worker has issued job `wait_job`
  // (it waits for the event's previous record), then record.  again = behind an overlay / the mesh stream, which leaves draw_unrecorded alone
  struct DrawEnd { int set; uint64_t wait_job; };
  DrawEnd draw_end(bool again = false) {
    draw_pending[vol_set] = true;
    if (!again) draw_unrecorded = false;
    return DrawEnd{vol_set, draw_wait_job[vol_set]};
  }

  // ---- the integrate lane
  // the context's stream joins the lane: true = record integ_done on the lane and wait for it
  bool join_integ() {
    const bool join = integ_pending;
    integ_pending = false;
    return join;
  }
  // integrate() on the lane, in the order abi.cpp acts on it
  struct Integrate {
    bool record_end; DrawEnd end;   // a draw without hole filling behind it: mark its end first
    bool join;                      // join_integ() (bookkeeping only: the lane is in order, and a draw has normally consumed it)
    int wait_draw;                  // then the other set becomes the one in use, and the lane waits for draw_done[wait_draw]: the draw two frames back read this set (-1: none)
  };
  Integrate integrate() {
    Integrate I{};
    I.record_end = draw_unrecorded;
    if (I.record_end) I.end = draw_end();
    I.join = join_integ();
    vol_set ^= 1;
    I.wait_draw = draw_pending[vol_set] ? vol_set : -1;
    draw_pending[vol_set] = false;
    integ_pending = true;
    return I;
  }

  // ---- the pyramids and the fill lane
  // the context's stream joins the hole filling of pyramid p: wait = until the worker has issued job `job`, then for fill_done[p]
  struct FillJoin { bool wait; uint64_t job; };
  FillJoin join_fill(int p) {
    const FillJoin J{fill_pending[p], fill_job_no[p]};
    fill_pending[p] = false;
    return J;
  }
  // a draw takes its pyramid -- the other one where two alternate, else the one in use, behind every hole filling in flight
  struct Pyramid { int index; FillJoin join[2]; };
  Pyramid take_pyramid(bool two_pyramids) {
    Pyramid Y{};
    if (two_pyramids) atlas_parity ^= 1;
    for (int p = 0; p < 2; ++p) Y.join[p] = (two_pyramids && p != atlas_parity) ? FillJoin{false, 0} : join_fill(p);
    Y.index = atlas_parity;
    return Y;
  }
  // a hole filling of the draw's pyramid has been queued on the fill lane: by the caller's thread (earlier jobs drained) ...
  void fill_queued() { fill_pending[atlas_parity] = true; }
  // ... or handed to the worker as job `job`, which waits for draw_done[set] and records fill_done[pyramid]
  void fill_queued(uint64_t job) {
    fill_job_no[atlas_parity] = draw_wait_job[vol_set] = job;
    fill_queued();
  }

  // ---- the resets
  // the host has waited for the context's streams (integ_lane: there is an integrate stream among them)
  void host_synchronised(bool integ_lane) {
    if (integ_lane) { integ_pending = false; draw_pending[0] = draw_pending[1] = false; }
    fill_pending[0] = fill_pending[1] = false;
  }
  // the pipelined mode was left and the integrate lane drained
  void integ_lane_drained() { integ_pending = false; }
  void second_set_unavailable() { deep_failed = true; }
  void volume_released() { deep_failed = false; }
  void view_released() { atlas_parity = 0; }
};

}  // namespace rr
