// The result paths' bookkeeping: the ring of slots a result travels to the host through (the frame read-out's, the mesh stream's), and the staging and
// chunking of a call that takes host arrays (the ray queries, the texture taps).  Host only, free of HIP: the state and one named transition per event,
// handing back plain values (a slot index, a boolean, a small verdict).  The slots' buffers, events and tags, the staging's device buffers, allocations and
// launches stay in abi.cpp, which acts on what a transition returns.  tests/test_result_paths.py walks every state and event of the ring on a CPU.
#pragma once
#include <stdint.h>

namespace rr {

constexpr uint32_t kMaxResultSlots = 8;          // a ring is configured with 2 .. kMaxResultSlots slots
enum ResultVerdict { kResultGo = 0, kResultNoneQueued = 1, kResultAlreadyHeld = 2 };   // what acquire() answers

// A ring of `slots` slots, written and handed out in order: `head` is the oldest frame not yet released, `count` the frames queued or held, `held` whether
// the head is in the caller's hands.  A frame is written into slot (head + count) % slots, the oldest is handed out once, release advances the head.
struct ResultRing {
  uint32_t slots = 0, head = 0, count = 0; bool held = false;
  void configure(uint32_t n) { slots = n; reset(); }
  void reset() { head = 0; count = 0; held = false; }                    // the slots' buffers were released: nothing queued, the next frame goes to slot 0
  bool idle() const { return count == 0; }                               // nothing queued or held: the ring may be reconfigured, its buffers dropped
  bool full() const { return count >= slots; }                           // every slot is queued or held
  uint32_t queued(uint32_t k) const { return (head + k) % slots; }       // the k-th frame queued or held (k < count), oldest first
  uint32_t oldest() const { return head; }
  ResultVerdict acquire() const { return !count ? kResultNoneQueued : held ? kResultAlreadyHeld : kResultGo; }   // may the oldest frame be handed out?
  int push() { return full() ? -1 : (int)queued(count++); }              // a frame is queued: the slot to write, or -1 (full: nothing changes)
  bool hold() { if (acquire() != kResultGo) return false; held = true; return true; }   // the oldest frame goes to the caller; refused unless acquire() says go
  bool release() {                                                       // the caller gives the held frame back; refused when none is held
    if (!held) return false;
    held = false; head = (head + 1) % slots; --count;
    return true;
  }
};

// Staging of a call's synchronous form (host arrays in and out): one capacity, in elements of the call (rays, points), for the input and result buffers,
// one for the buffer only some calls ask for (a cast's surface records, a tap call's sensor records: allocated by the first call that does); grown to the
// next power of two at or above the need (at least 1024 elements), never shrunk.
struct CallStaging {
  uint64_t capacity = 0;          // elements the input / result buffers hold
  uint64_t extra_capacity = 0;    // elements the optional buffer holds
  static uint64_t round_up(uint64_t n) { uint64_t c = 1024; while (c < n) c <<= 1; return c; }   // (n <= 2^40, kRayMaxCount / kTapsMaxPoints: no overflow)
  // the capacity to allocate before a call of n elements, or 0 when the buffers do
  uint64_t grow(uint64_t n) const { return n > capacity ? round_up(n) : 0; }
  uint64_t grow_extra(uint64_t n, bool wanted) const { return wanted && n > extra_capacity ? round_up(n) : 0; }
  void grown(uint64_t c) { capacity = c; }
  void extra_grown(uint64_t c) { extra_capacity = c; }
  void released() { capacity = 0; extra_capacity = 0; }
};

// A call runs as launches (a cast: launch pairs) of at most `chunk` elements: launch k covers elements [first, first + count)
struct CallChunks {
  uint64_t n; uint32_t chunk;
  uint64_t launches() const { return (n + chunk - 1) / chunk; }
  uint64_t first(uint64_t k) const { return k * chunk; }
  uint32_t count(uint64_t k) const { const uint64_t left = n - first(k); return left < chunk ? (uint32_t)left : chunk; }
};

}  // namespace rr
