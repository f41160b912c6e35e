// The volume sets' bookkeeping: what the incremental tile classification remembers of a set from one integrate() to the next, and where the integrated
// tiles' classes start in a set's class array.  Host only, free of HIP: the state and one named transition per event, handing back plain values (0 / 1
// indices into a set's two tile lists and two count words, the frame stamp, booleans).  The sets' device buffers, which set is in use (DrawLanes::set()),
// allocations and launches stay in abi.cpp, which acts on what a transition returns.  tests/test_volume_sets.py walks every state and event on a CPU.
//
// A culled integrate() writes one of a set's two lists and clears only the tiles on the other, the previous integrate()'s: the only tiles that can hold
// anything but the clear value -- unless something else may have written the volume since, or changed the clear value: then the next one walks every
// tile.  One history per set: with two sets alternating (draw_lanes.hpp) each evolves like the single volume, seeing every other frame.
#pragma once
#include <cstddef>
#include <cstdint>

namespace rr {

struct TileHistory {
  // ---- state (abi.cpp goes through the transitions and the accessors below)
  int parity = 0;          // the list and count word the next culled integrate() writes
  bool full = true;        // the next culled integrate() walks every tile (it may not trust the previous list)
  uint32_t stamp = 0;      // the frame stamp of the last culled integrate(); 0 = what the set's stamps are initialised to

  // ---- read only
  bool full_walk() const { return full; }
  // the list and count word the last culled integrate() wrote: end() has flipped the parity behind its launches
  int last() const { return parity ^ 1; }

  // ---- integrate()
  // Before the launches.  Culled: this frame's list / count word, the previous integrate()'s -- its count word is also the one the integrate kernel
  // re-arms for the next frame --, and the frame's stamp; the stamp runs from 0xffffffff round to 1, never to 0: wipe = zero the set's stamps first,
  // and that frame is a full walk.  Dense: nothing changes (the values are the ones a culled frame would start from; no launch reads them)
  struct Begin { int list, prev; uint32_t stamp; bool wipe; };
  Begin begin(bool culled) {
    bool wipe = false;
    if (culled && ++stamp == 0) { stamp = 1; full = true; wipe = true; }
    return Begin{parity, parity ^ 1, stamp, wipe};
  }
  // Behind the launches.  A dense pass wrote every tile: the next culled frame must look at all of them
  void end(bool culled) {
    if (culled) { parity ^= 1; full = false; }
    else full = true;
  }

  // ---- the resets
  // something else may have written the volume (an upload), or its clear value changed (the limit), or the brick grid is a new one
  void invalidate() { full = true; }
  // the set's buffers were released, or allocated and initialised
  void reset() { *this = TileHistory{}; }
};

// Where the first integrated tile layer starts in a set's class array, which has one entry per STORED tile (layers [tz0, tz1) of nty x ntx tiles; the
// integrated ones start at int_tz0 >= tz0)
inline size_t class_offset(int tz0, int int_tz0, int nty, int ntx) { return (size_t)(int_tz0 - tz0) * nty * ntx; }

}  // namespace rr
