// The slab exchange's bookkeeping: who does what in a world of ranks, and what the compact composite remembers of a frame from its gather to its verdict.
// Host only, free of HIP and RCCL: the state and one named transition per event, handing back plain values (ranks, rows, ring slots, record counts,
// booleans).  The communicator, the device and pinned buffers, the count events and every HIP / RCCL call stay in comm.cpp, which acts on what a
// transition returns.  rgbd-recon_amd/slab_exchange.py is the same protocol for the torch.distributed path (SlabDriver);
// tests/test_slab_exchange.py walks both on a CPU, against the statements they replaced and against each other.
#pragma once
#include <algorithm>
#include <cstdint>

namespace rr {

// ---- roles and rows: rank 0 gathers, composites and fills holes; with a dedicated compositor it holds no slab and the workers are ranks 1 .. world - 1
struct SlabRoles {
  int rank = 0, world = 1;
  bool dedicated = false;                  // rank 0 holds no slab: it only receives, composites and fills holes
  static constexpr int kNone = -1;

  bool worker() const { return !(dedicated && rank == 0); }      // owns a slab: marks bricks, integrates, marches, exports
  int first_worker() const { return dedicated ? 1 : 0; }
  bool gathers() const { return rank == 0; }                     // holds the parts (one row per rank), composites them

  // the halo: every rank's {low, high} face all-gathered, [world][2][n] floats.  A slab's lower neighbour hands it its HIGH face, the upper one its
  // LOW face; row kNone: no neighbour on that side (the first and the last worker; a compositor has none at all)
  struct Face { int row, face; };
  Face below() const { return worker() && rank > first_worker() ? Face{rank - 1, 1} : Face{kNone, 0}; }
  Face above() const { return worker() && rank < world - 1 ? Face{rank + 1, 0} : Face{kNone, 0}; }
  static size_t face_offset(Face f, size_t n) { return ((size_t)f.row * 2 + f.face) * n; }

  // the hit records: rank 0's own block is row 0 of the parts -- its records never travel --, every other rank's the send buffer
  bool own_in_parts() const { return rank == 0; }
  // Rank 0 exports ALL its records, whatever the capacity of the gather, once per frame, and must not export them again for a repeated gather (the
  // first composite has overwritten the march target they are read from); the others export `cap` records for every gather.  A compositor without a
  // slab never exports: its header stays {0 records, 0 hits}
  bool exports(bool first) const { return worker() && (first || rank != 0); }
  uint32_t export_records(uint32_t npx, uint32_t cap) const { return rank == 0 ? npx : cap; }
  // the send / recv group (none with one rank): rank 0 receives from ranks [recv_begin, world) into their rows, every other rank sends once to send_to
  bool grouped() const { return world > 1; }
  int recv_begin() const { return rank == 0 ? 1 : world; }
  int send_to() const { return rank == 0 ? kNone : 0; }
  static size_t exchange_floats(uint32_t cap) { return 8 + (size_t)cap * 8; }    // one exchange: 32-byte header + cap 32-byte records
  static size_t row_floats(size_t npx) { return 8 + npx * 8; }                   // one row of the parts: a slab cannot hit more rays than there are pixels
  static size_t row_offset(int row, size_t row_floats) { return (size_t)row * row_floats; }
};

// ---- the gather book.  A frame is gathered with a FIXED number of records per rank, 1.5 x the largest per-rank hit count of the frame kLag frames
// earlier (every rank computes the same number from the same all-gathered counts).  The counts of the latest kRing frames lie in a ring of pinned
// copies: the book says which slot to write, read or wait on, the caller hands it the slot's largest hit count.  A frame that hit more rays than were
// gathered is repaired by finish() while it is the latest frame; otherwise it was composited from truncated lists -- counted, and marked in a ring of
// the last kVerdicts verdicts.  Arithmetic in uint32_t: exact for m * 3 < 2^32, which m <= view pixels + 1 <= 16384^2 + 1 guarantees
struct GatherBook {
  static constexpr int kLag = 2;           // frames between a hit count and its use as a gather size: its pinned copy has long arrived
  static constexpr int kRing = kLag + 1;
  static constexpr int kVerdicts = 64;

  // ---- state (comm.cpp goes through the events below)
  uint32_t min_capacity = 4096, max_capacity = 0;                // bounds of the lagged guess; max_capacity 0 = one record per pixel
  uint32_t regathers = 0, overflowed_frames = 0;                 // frames finish() repaired / frames left truncated
  uint64_t frame_no = 0;                                         // frames gathered since the buffers were allocated
  bool have_last = false; uint64_t last_frame = 0; uint32_t last_cap = 0;   // the latest frame, until finish() has checked it
  uint32_t caps[kRing] = {};               // capacity each of the ring's frames was gathered with
  bool counts_rec[kRing] = {};             // the slot's count event has been recorded: a reader waits for it
  uint64_t verdict_frame[kVerdicts] = {}; uint8_t verdict[kVerdicts] = {}; bool verdict_set[kVerdicts] = {};   // 1 = left truncated

  // ---- read only
  bool recorded(int slot) const { return counts_rec[slot]; }
  int open_slot() const { return (int)(frame_no % kRing); }                       // where the frame being gathered leaves its counts
  int lagged_slot() const { return frame_no < (uint64_t)kLag ? -1 : (int)((frame_no - kLag) % kRing); }   // the counts open() wants; -1: none, no history yet
  int pending_slot() const { return have_last ? (int)(last_frame % kRing) : -1; }   // the counts finish() wants; -1: nothing pending

  // ---- (a) open frame frame_no: the records to gather per rank.  m: the largest hit count in lagged_slot() (ignored without history).  Settles the
  // verdict of frame frame_no - kLag: it was gathered with caps[...] (finish() raises the capacity of a frame it repairs)
  uint32_t open(uint32_t view_px, uint32_t m) {
    const uint32_t npx = max_capacity ? std::min(max_capacity, view_px) : view_px;
    if (frame_no < (uint64_t)kLag) return npx;                   // no history yet: a slab cannot hit more rays than there are pixels
    const uint64_t f = frame_no - kLag;
    const bool truncated = m > caps[f % kRing];
    if (truncated) ++overflowed_frames;
    set_verdict(f, truncated);
    const uint32_t cap = std::max(min_capacity, ((m * 3u) / 2u + 1024u + 1023u) / 1024u * 1024u);
    return std::min(cap, npx);
  }
  // ---- (b) the frame's first exchange has been queued with `cap` records, its counts on their way into open_slot()
  void queued(uint32_t cap) {
    const int slot = open_slot();
    counts_rec[slot] = true; caps[slot] = cap;
    have_last = true; last_frame = frame_no; last_cap = cap;
    ++frame_no;
  }
  // ---- (c) finish: the latest frame is complete, or must be gathered again with `cap` records (its exact size; max_capacity bounds the guess only).
  // m: the largest hit count in pending_slot().  Nothing pending: nothing happens
  struct Repair { bool regather; uint32_t cap; };
  Repair finish(uint32_t view_px, uint32_t m) {
    Repair r{false, 0};
    if (!have_last) return r;
    have_last = false;
    if (m > last_cap) {
      ++regathers;
      r = Repair{true, std::min(view_px, m)};
      caps[last_frame % kRing] = r.cap;
    }
    set_verdict(last_frame, false);                              // complete: gathered in full, or repaired by the caller now
    return r;
  }
  // ---- (d) was frame f left truncated?  kVerdict: `truncated` says; kCompare: its counts are still in the ring -- truncated if the largest hit count
  // in `slot` exceeds `cap` (not stored: the latest frame may still be repaired); kNotGathered; kNotKept: older than the ring of verdicts
  struct Status { enum Kind { kVerdict, kCompare, kNotGathered, kNotKept } kind; int truncated, slot; uint32_t cap; };
  Status status(uint64_t f) const {
    if (f >= frame_no) return Status{Status::kNotGathered, 0, -1, 0};
    const int k = (int)(f % kVerdicts);
    if (verdict_set[k] && verdict_frame[k] == f) return Status{Status::kVerdict, verdict[k], -1, 0};
    if (f + kRing >= frame_no) return Status{Status::kCompare, 0, (int)(f % kRing), caps[f % kRing]};
    return Status{Status::kNotKept, 0, -1, 0};
  }
  // ---- (e) the limits (the caller has checked them: min_records >= 1, max_records 0 or >= min_records)
  void set_limits(uint32_t min_records, uint32_t max_records) { min_capacity = min_records; max_capacity = max_records; }
  // ---- (f) the buffers were released: frames count from 0 again; the limits and the statistics stay.  (g) a new communicator: GatherBook{}
  void released() {
    GatherBook fresh;
    fresh.set_limits(min_capacity, max_capacity); fresh.regathers = regathers; fresh.overflowed_frames = overflowed_frames;
    *this = fresh;
  }

  // ---- inside the events
  void set_verdict(uint64_t f, bool truncated) {
    const int k = (int)(f % kVerdicts);
    verdict_frame[k] = f; verdict[k] = truncated ? 1 : 0; verdict_set[k] = true;
  }
};

}  // namespace rr
