// The lane ahead's frame bookkeeping: the stream that prepares frame f + 1 while the context's stream still works on frame f, and the double
// buffers that alternate under it.  Host only, free of HIP: the state and one named transition per event, handing back plain values (booleans,
// 0 / 1 indices into the two gate events, the two counter buffers, the two occupancy sets, the three count words; -1 = none).  Streams, events,
// device pointers, allocations and launches stay in abi.cpp, which acts on what a transition returns.  tests/test_lane_ahead.py walks every
// state, event and input on a CPU.
//
// A third lane AHEAD of the context's stream (round 3): what a new frame needs before integrate() can run -- its re-layout and the brick passes
// (clear / mark / update) -- reads only the new frame and writes state nobody else writes, so it runs on tsdf_ctx::pre_stream while the
// context's stream still works on the previous frame.  Everything the lane writes exists twice and alternates: the frame slots (flip at the
// first upload of a frame), the brick counters (flip at clearOccupiedBricks), flags + occupied list + count (flip at updateOccupiedBricks).
// Each flips once per frame of the lane, and only when a consumer has been queued since the copy was last written (Twin, below).  Two events
// tie the lanes: pre_done (integrate / draw wait for the lane; recorded once, when a consumer asks: every record costs the lane ~4 us) and
// the gate (recorded on the context's stream at the lane's first call of a frame, waited for at its first call of the NEXT frame: what the
// lane overwrites then was last read two frames ago).  (A third copy of everything, letting the lane run two frames ahead, was built and
// measured: the lanes then crowd each other -- every stage stretches -- and the frame takes 140 instead of 121 us: DESIGN.md section 5.)
// Off with stage overlap off, after an explicit frame-slot call (tsdf_select_frame_slot, tsdf_upload_frame_async) and for the
// pre-processing path: blocked().
//
// (round 4) The gate's wait can be DEFERRED inside tsdf_frame_raw_dev: the first two pre-processing passes write nothing the previous draws
// read, so they run in front of it.  Two gate events alternate so that a deferred wait still refers to the record of the previous frame after
// this frame's record has been made.  A deferred wait is never dropped: every transition that clears it returns it.
//
// Brick counters: two buffers.  On the lane the frame's re-layout launch clears the buffer the frame's clearOccupiedBricks() is going to use
// (counters_for_upload; the clear then has no fill of its own).  Off the lane integrate(f)'s classify launch zeroes the buffer not in use
// (counters_zero_spare) and clearOccupiedBricks() of frame f + 1 is a swap instead of a fill launch; spare_clean says whether that happened.
//
// Occupancy: two sets (flags, list) and three count words.  Off the lane the sets and the words 0 / 1 alternate per update, and the update's
// kernel re-arms (zeroes) the other word for the next one.  On the lane the marking launch zeroes the word the coming update will land on and
// the update re-arms none (word 2 takes the kernel's store); once the lane has used the words the context's stream zeroes its word itself
// (counts_stale).
#pragma once

namespace rr {

struct LaneAhead {
  // One resource that exists twice and alternates under the lane
  struct Twin {
    bool flipped = false;         // the lane has taken it for writing in this frame of the lane
    bool in_use = false;          // a consumer has been queued since it was last written
    bool would_flip() const { return !flipped && in_use; }
    // the lane takes it for writing: true = the other copy (the context's stream may still read this one), once per frame of the lane
    bool take() { const bool flip = would_flip(); flipped = true; in_use = false; return flip; }
  };

  // ---- state (abi.cpp goes through the transitions and the accessors below)
  bool pipeline_blocked = false;
  // the gate
  bool main_since_gate = true;    // a consumer has been queued since the gate was recorded: the lane's next call opens a new frame
  bool pre_gate_recorded = false, gate_flip = false;
  bool gate_wait_pending = false; int gate_wait_ev = 0;   // the deferred wait
  bool pre_pending = false;       // the lane holds work no consumer has waited for
  Twin slot, counters, occ;
  int counters_cur = 0; bool counters_zeroed = false;     // zeroed: the re-layout launch has cleared them already
  bool spare_clean = false;
  int occ_parity = 0;
  bool occ_count_zeroed = false; int occ_zeroed_word = 0; // the marking launch has cleared a count word, and which
  bool occ_counts_stale = false;

  // ---- read only
  bool blocked() const { return pipeline_blocked; }
  bool at_frame_start() const { return main_since_gate; }
  int counters_buffer() const { return counters_cur; }
  int occ_set() const { return occ_parity; }

  // ---- the gate
  // the deferred wait, now: the gate event to wait for, or -1
  int take_deferred_gate() {
    if (!gate_wait_pending) return -1;
    gate_wait_pending = false;
    return gate_wait_ev;
  }
  // The lane's first call of a new frame (at_frame_start()), in the order abi.cpp acts on it.  integ_busy: an integrate() on the fourth lane
  // that no draw has joined may still read what this frame overwrites, and the lane is not that stream itself
  struct Open {
    int overdue;                  // a deferred wait nobody asked for: never skipped
    int wait;                     // the gate recorded at the previous frame's first call (the consumers of the frame before that): wait now ...
    int deferred;                 // ... or later (take_deferred_gate, later_call)
    bool wait_integ;              // then the lane waits for the integrate lane
    int record;                   // and the context's stream records this frame's gate
  };
  Open open_frame(bool defer_gate, bool integ_busy) {
    Open O{};
    const int gate_old = gate_flip ? 1 : 0, gate_new = gate_flip ? 0 : 1;
    O.overdue = take_deferred_gate();
    O.wait = O.deferred = -1;
    if (pre_gate_recorded) {
      if (defer_gate) { gate_wait_pending = true; gate_wait_ev = O.deferred = gate_old; }
      else O.wait = gate_old;
    }
    O.wait_integ = integ_busy;
    O.record = gate_new;
    gate_flip = !gate_flip;
    pre_gate_recorded = true; main_since_gate = false;
    slot.flipped = counters.flipped = occ.flipped = false;
    counters_zeroed = occ_count_zeroed = false;
    return O;
  }
  // a later call of the frame: the deferred wait to perform, or -1 (a call that defers the gate itself leaves it)
  int later_call(bool defer_gate) { return defer_gate ? -1 : take_deferred_gate(); }
  // a call has queued its work (on the lane, or on the context's stream with the lane off)
  void call_queued(bool on_lane) { if (on_lane) pre_pending = true; }

  // ---- consumers of a frame's images / brick state (every draw, integrate(), the reads): true = record pre_done on the lane and wait for it
  bool consume() {
    main_since_gate = true;
    slot.in_use = counters.in_use = occ.in_use = true;
    const bool join = pre_pending;
    pre_pending = false;
    return join;
  }

  // ---- leaving and draining
  // the lane's stream or events cannot be created: everything on the context's stream
  void lane_unavailable() { pipeline_blocked = true; }
  // leave the pipelined mode for good; false = it was left already, true = drain the lanes
  bool block() {
    if (pipeline_blocked) return false;
    pipeline_blocked = true;
    pre_pending = false;
    return true;
  }
  // the host has waited for the lane's stream
  void lane_synchronised() { pre_pending = false; }

  // ---- the frame slot: true = write the other slot (allocate it, take the colour along if the caller brings none, make it current), false = in place
  bool slot_for_write(bool on_lane) {
    if (!on_lane || slot.flipped) return false;
    return slot.take();
  }

  // ---- the brick counters.  Buffer: 0 / 1 = tsdf_ctx::d_counters[], the buffer the bricks use from now on
  // a new brick grid: both buffers are zero
  void new_brick_grid() { counters_cur = 0; spare_clean = true; occ_counts_stale = false; }
  // the re-layout launch of an upload on the lane: the buffer to clear along the way, or -1 (off the lane, no buffers yet, or done for this frame)
  int counters_for_upload(bool on_lane_with_buffers) {
    if (!on_lane_with_buffers || counters_zeroed) return -1;
    if (counters.take()) counters_cur ^= 1;
    counters_zeroed = true; spare_clean = false;
    return counters_cur;
  }
  struct Clear { int buffer; bool fill; };   // fill: the buffer still has to be zeroed by a fill of its own
  Clear clear_bricks(bool on_lane) {
    Clear C{};
    if (on_lane) {
      if (counters.take()) counters_cur ^= 1;
      spare_clean = false;
      C.fill = !counters_zeroed;                                         // (a second clear of the frame fills again)
      counters_zeroed = false;
    } else if (spare_clean) {                                            // the other buffer was zeroed by the last integrate(): swap
      counters_cur ^= 1;
      spare_clean = false;
    } else C.fill = true;
    C.buffer = counters_cur;
    return C;
  }
  // the classify launch of integrate(); can = bricks in use, an incremental classification, the lanes off (the lane ahead clears its own).
  // Returns the buffer it zeroes for the next clearOccupiedBricks(), or -1
  int counters_zero_spare(bool can) {
    if (!can || spare_clean) return -1;
    spare_clean = true;
    return counters_cur ^ 1;
  }

  // ---- the occupancy sets and their count words
  // markBricks(): the count word the launch zeroes -- that of the set the coming update flips to (or stays on) --, or -1 off the lane
  int mark_bricks(bool on_lane) {
    if (!on_lane) return -1;
    occ_zeroed_word = occ.would_flip() ? occ_parity ^ 1 : occ_parity;
    occ_count_zeroed = true;
    return occ_zeroed_word;
  }
  struct Update { int set; bool fill; int rearm; };   // set: flags / list / count word to use; fill: zero that word first; rearm: the word the kernel zeroes
  Update update_occupied(bool on_lane) {
    Update U{};
    if (on_lane) {
      if (occ.take()) occ_parity ^= 1;
      occ_counts_stale = true;
      // the frame's marking launch cleared a count word -- THE one this update lands on, unless a call between the two (a draw, tsdf_occupied_ratio,
      // an integrate on the context's stream) joined the lane and made this update flip after all: then, and for a second update of
      // the frame, fill again
      U.fill = !(occ_count_zeroed && occ_zeroed_word == occ_parity);
      occ_count_zeroed = false;
      U.rearm = 2;                                                       // (a third word takes the kernel's re-arming store)
    } else {
      occ_parity ^= 1;                                                   // zero since the previous update (or creation) re-armed it ...
      U.fill = occ_counts_stale;                                         // ... unless the lane ahead has used the words in between (it zeroes its own and re-arms none)
      occ_counts_stale = false;
      U.rearm = occ_parity ^ 1;
    }
    U.set = occ_parity;
    return U;
  }
};

}  // namespace rr
