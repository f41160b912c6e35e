"""CPU: the slab exchange's bookkeeping (rgbd-recon_amd/csrc/slab_exchange.hpp, HIP-free, and its Python twin rgbd-recon_amd/slab_exchange.py) as a
stand-alone program with its own main, built with the host address and undefined-behaviour sanitizers.  No machine this project has run on holds more
than one GPU: these walks are the only execution the multi-rank decisions have had.

(a) GatherBook against the statements it replaced -- tsdf_ctx::Comm's loose fields and the bookkeeping of capacity_for, set_verdict, max_hits,
exchange_hits, release_comm_buffers, tsdf_comm_frame_status, tsdf_composite_gather and tsdf_composite_finish, restated here as one small struct, the
HIP / RCCL calls left out, the pinned counts a table of three integers per form.  Every sequence of seven state-changing events (gather at each of six
hit levels, finish, four limit settings, buffers released), from a fresh book and from a used one whose buffers were released; after EVERY event both
forms are asked the status of each frame in [frame_no - 5, frame_no].  The status query is const in both forms (the compiler holds it to that), so a
sequence with status events anywhere in it decides what its state-changing events alone decide: every sequence of seven events over the whole alphabet
is one of the walked prefixes with its queries answered.  Then 260 frames with hit counts from a fixed LCG: the verdicts pass the ring of 64.
(b) SlabRoles for every world 1 .. 32, shared and dedicated, every rank: against the old expressions, and the structural facts on their own.
(c) The same event scripts through the header and through the Python book: the decision lines must be identical; the Python roles against (b)'s rows."""
import importlib.util
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbd-recon_amd", "csrc")

MAIN = r'''
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "slab_exchange.hpp"
using namespace rr;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #x); std::exit(1); } } while (0)

// ---- (a) the statements GatherBook replaced, as they stood (the HIP / RCCL calls between them left out).  h_counts[slot] is `table[slot]`: the largest
// per-rank hit count of the frame whose counts were copied there last
struct OldComm {
  static constexpr int kLag = 2, kRing = kLag + 1;
  int vw = 160, vh = 90;
  uint32_t table[3] = {0, 0, 0}; bool counts_rec[3] = {false, false, false};
  uint32_t caps[3] = {0, 0, 0};
  uint64_t frame_no = 0; bool have_last = false; uint64_t last_frame = 0; uint32_t last_cap = 0;
  uint32_t regathers = 0, overflowed_frames = 0, min_capacity = 4096, max_capacity = 0;
  static constexpr int kVerdicts = 64;
  uint64_t verdict_frame[kVerdicts] = {}; uint8_t verdict[kVerdicts] = {}; bool verdict_set[kVerdicts] = {};
  mutable int slot_read = -1; int slot_written = -1;       // what the last call read (counts_of) and wrote (the copy behind the all-gather)

  void release_comm_buffers() {
    OldComm fresh;
    fresh.vw = vw; fresh.vh = vh;                          // (the context's, not the communicator's)
    fresh.regathers = regathers; fresh.overflowed_frames = overflowed_frames; fresh.min_capacity = min_capacity; fresh.max_capacity = max_capacity;
    *this = fresh;                                         // (h_counts freed: the next gather allocates and zeroes them)
  }
  uint32_t max_hits(uint64_t f) const { const int slot = (int)(f % kRing); slot_read = slot; return table[slot]; }
  void set_verdict(uint64_t f, bool truncated) {
    const int k = (int)(f % kVerdicts);
    verdict_frame[k] = f; verdict[k] = truncated ? 1 : 0; verdict_set[k] = true;
  }
  uint32_t capacity_for(uint64_t f) {
    const uint32_t npx = max_capacity ? std::min(max_capacity, (uint32_t)(vw * vh)) : (uint32_t)(vw * vh);
    if (f < (uint64_t)kLag) return npx;
    const uint32_t m = max_hits(f - kLag);
    const bool truncated = m > caps[(f - kLag) % kRing];
    if (truncated) ++overflowed_frames;
    set_verdict(f - kLag, truncated);
    const uint32_t cap = std::max(min_capacity, ((m * 3u) / 2u + 1024u + 1023u) / 1024u * 1024u);
    return std::min(cap, npx);
  }
  void exchange_hits(uint32_t cap, bool first, uint64_t f, uint32_t level) {
    const bool record_counts = first;
    if (record_counts) {
      const int slot = (int)(f % kRing);
      table[slot] = level; slot_written = slot;            // hipMemcpyAsync(h_counts[slot], ...)
      counts_rec[slot] = true;
      caps[slot] = cap;
    }
  }
  void set_capacity_limits(uint32_t lo, uint32_t hi) { min_capacity = lo; max_capacity = hi; }
  // tsdf_comm_frame_status: 0 = TSDF_OK with *truncated, 1 = "not gathered yet", 2 = "no longer kept"
  int frame_status(uint64_t frame, int* truncated) const {
    if (frame >= frame_no) return 1;
    const int k = (int)(frame % kVerdicts);
    if (verdict_set[k] && verdict_frame[k] == frame) { *truncated = verdict[k]; return 0; }
    if (frame + kRing >= frame_no) {
      const bool t = max_hits(frame) > caps[frame % kRing];
      *truncated = t ? 1 : 0;
      return 0;
    }
    return 2;
  }
  // tsdf_composite_gather in two halves: the level of the frame's own counts is chosen from the capacity it was handed
  void buffers_released() {                                // its allocation branch (a view of another size; the first gather)
    release_comm_buffers();
    frame_no = 0; have_last = false;
    for (bool& b : verdict_set) b = false;
  }
  uint32_t gather_open() { slot_read = slot_written = -1; return capacity_for(frame_no); }
  void gather_queue(uint32_t cap, uint32_t level) {
    const uint64_t f = frame_no;
    exchange_hits(cap, true, f, level);
    have_last = true; last_frame = f; last_cap = cap;
    frame_no = f + 1;
  }
  struct Repair { bool regather; uint32_t cap; };
  Repair composite_finish() {
    Repair r{false, 0};
    slot_read = slot_written = -1;
    if (have_last) {
      have_last = false;
      const uint32_t m = max_hits(last_frame);
      if (m > last_cap) {
        ++regathers;
        const uint32_t cap = std::min((uint32_t)(vw * vh), m);
        r = Repair{true, cap};
        exchange_hits(cap, false, last_frame, 0);
        caps[last_frame % kRing] = cap;
      }
      set_verdict(last_frame, false);
    }
    return r;
  }
};

// the new form: comm.cpp's statements over the book, the same halves
struct NewComm {
  int vw = 160, vh = 90;
  GatherBook book; uint32_t table[3] = {0, 0, 0};
  int slot_read = -1, slot_written = -1;
  uint32_t npx() const { return (uint32_t)(vw * vh); }
  void buffers_released() { book.released(); std::memset(table, 0, sizeof table); }
  uint32_t gather_open() {
    slot_read = slot_written = -1;
    const int lagged = book.lagged_slot();
    if (lagged >= 0) slot_read = lagged;
    return book.open(npx(), lagged >= 0 ? table[lagged] : 0);
  }
  void gather_queue(uint32_t cap, uint32_t level) { slot_written = book.open_slot(); table[slot_written] = level; book.queued(cap); }
  GatherBook::Repair composite_finish() {
    slot_read = slot_written = -1;
    const int pending = book.pending_slot();
    if (pending < 0) return book.finish(npx(), 0);           // (comm.cpp does not call it then: it must be a no-op)
    slot_read = pending;
    return book.finish(npx(), table[pending]);
  }
  int frame_status(uint64_t frame, int* truncated, int* read) const {
    const GatherBook::Status S = book.status(frame);
    *read = -1;
    switch (S.kind) {
      case GatherBook::Status::kNotGathered: return 1;
      case GatherBook::Status::kVerdict: *truncated = S.truncated; return 0;
      case GatherBook::Status::kCompare: *read = S.slot; *truncated = table[S.slot] > S.cap ? 1 : 0; return 0;
      default: return 2;
    }
  }
};

static const uint32_t kLimits[4][2] = {{4096, 0}, {4, 0}, {4, 64}, {1, 1}};
enum { GATHER0 = 0, FINISH = 6, LIMITS0 = 7, RELEASED = 11, N_EVENTS = 12 };
static uint32_t level_of(int k, uint32_t cap, uint32_t min_capacity, uint32_t npx) {
  switch (k) {
    case 0: return 0;
    case 1: return min_capacity - 1;
    case 2: return cap;
    case 3: return cap + 1;
    case 4: return npx;
    default: return npx + 1;                                 // an impossible count: the old code tolerated it, and so must the book
  }
}
static unsigned long g_rows = 0, g_status_rows = 0, g_sequences = 0;
static void fail(const char* what, const int* seq, int len) {
  std::fprintf(stderr, "the forms disagree on %s after events", what);
  for (int k = 0; k < len; ++k) std::fprintf(stderr, " %d", seq[k]);
  std::fprintf(stderr, "\n");
  std::exit(1);
}
static void statuses_agree(const OldComm& o, const NewComm& n, const int* seq, int len) {
  for (uint64_t back = 0; back <= 5; ++back) {
    const uint64_t f = o.frame_no - back;                    // (below frame 0 the number wraps: "not gathered yet" in both forms)
    int to = -1, tn = -1, read = -1;
    o.slot_read = -1;
    const int co = o.frame_status(f, &to), cn = n.frame_status(f, &tn, &read);
    if (co != cn || to != tn || o.slot_read != read) fail("a frame's status", seq, len);
    ++g_status_rows;
  }
}
static void step(OldComm& o, NewComm& n, int ev, const int* seq, int len) {
  if (ev < FINISH) {
    const uint32_t co = o.gather_open(), cn = n.gather_open();
    if (co != cn || o.slot_read != n.slot_read) fail("the capacity handed out", seq, len);
    const uint32_t level = level_of(ev - GATHER0, co, o.min_capacity, (uint32_t)(o.vw * o.vh));
    CHECK((uint64_t)level * 3 < (1ull << 32) && level <= (uint32_t)(o.vw * o.vh) + 1);          // the range the uint32_t arithmetic is exact in
    o.gather_queue(co, level); n.gather_queue(cn, level);
    if (o.slot_written != n.slot_written) fail("the slot written", seq, len);
  } else if (ev == FINISH) {
    const OldComm::Repair a = o.composite_finish(); const GatherBook::Repair b = n.composite_finish();
    if (a.regather != b.regather || a.cap != b.cap || o.slot_read != n.slot_read) fail("the repair", seq, len);
  } else if (ev < RELEASED) {
    const uint32_t* L = kLimits[ev - LIMITS0];
    o.set_capacity_limits(L[0], L[1]); n.book.set_limits(L[0], L[1]);
  } else {
    o.buffers_released(); n.buffers_released();
  }
  if (o.regathers != n.book.regathers || o.overflowed_frames != n.book.overflowed_frames || o.frame_no != n.book.frame_no) fail("the statistics or frame_no", seq, len);
  if (std::memcmp(o.table, n.table, sizeof o.table) != 0) fail("the counts", seq, len);
  ++g_rows;
  statuses_agree(o, n, seq, len);
}
static const int kLen = 7;
static void walk_from(const OldComm& o, const NewComm& n, int* seq, int depth) {
  if (depth == kLen) { ++g_sequences; return; }
  for (int ev = 0; ev < N_EVENTS; ++ev) {
    OldComm p = o; NewComm q = n;
    seq[depth] = ev;
    step(p, q, ev, seq, depth + 1);
    walk_from(p, q, seq, depth + 1);
  }
}
static void walk_book() {
  int seq[kLen] = {};
  for (int start = 0; start < 2; ++start) {
    OldComm o; NewComm n;                                    // tsdf_comm_init: M = Comm{} / a fresh book
    if (start == 1) {                                        // a used communicator: frames, a repair, an overflow, other limits -- then its buffers released
      const int used[] = {GATHER0 + 4, GATHER0 + 4, GATHER0 + 4, LIMITS0 + 1, GATHER0 + 5, GATHER0 + 3, FINISH, GATHER0 + 2, RELEASED};
      for (int ev : used) step(o, n, ev, seq, 0);
      CHECK(n.book.regathers == 1 && n.book.overflowed_frames == 1 && n.book.frame_no == 0 && n.book.min_capacity == 4);
      g_rows = g_rows - 9; g_status_rows -= 9 * 6;           // (the preamble is not part of the count below)
    }
    walk_from(o, n, seq, 0);
  }
}

// ---- 260 frames, hit counts from a fixed LCG, a finish behind every seventh frame and the last: the verdicts pass the ring of 64
static unsigned long walk_long() {
  OldComm o; NewComm n;
  o.vw = n.vw = 1280; o.vh = n.vh = 720;
  const uint32_t npx = 1280u * 720u;
  uint32_t x = 12345u;
  std::vector<char> finished;
  unsigned long gone = 0;
  for (int f = 0; f < 260; ++f) {
    x = x * 1664525u + 1013904223u;
    const uint32_t level = (x & 3u) == 0 ? (x >> 8) % (npx + 2) : (x >> 8) % 30000u;
    const uint32_t co = o.gather_open(), cn = n.gather_open();
    CHECK(co == cn && o.slot_read == n.slot_read);
    o.gather_queue(co, level); n.gather_queue(cn, level);
    CHECK(o.slot_written == n.slot_written);
    finished.push_back(0);
    if (f % 7 == 6 || f == 259) {
      const OldComm::Repair a = o.composite_finish(); const GatherBook::Repair b = n.composite_finish();
      CHECK(a.regather == b.regather && a.cap == b.cap);
      finished[f] = 1;
    }
    CHECK(o.regathers == n.book.regathers && o.overflowed_frames == n.book.overflowed_frames && o.frame_no == n.book.frame_no);
    // every frame so far: both forms agree, and "no longer kept" exactly where a later frame has taken the verdict's place in the ring of 64
    const uint64_t now = n.book.frame_no;
    gone = 0;
    for (uint64_t g = 0; g <= now; ++g) {
      int to = -1, tn = -1, read = -1;
      const int c0 = o.frame_status(g, &to), c1 = n.frame_status(g, &tn, &read);
      CHECK(c0 == c1 && to == tn);
      bool replaced = false;                                 // a frame h = g + 64 k has a verdict: settled by the gather of h + kLag, or finished while the latest
      for (uint64_t h = g + 64; h < now; h += 64) replaced = replaced || h + GatherBook::kLag < now || finished[h];
      CHECK((c1 == 2) == (g + GatherBook::kRing < now && replaced));
      if (c1 == 2) ++gone;
      ++g_status_rows;
    }
  }
  CHECK(n.book.regathers > 0 && n.book.overflowed_frames > 0);
  return gone;
}

// ---- (b) roles and rows
struct OldRoles {                                            // comm.cpp's expressions, as they stood
  int rank, world; bool dedicated;
  bool is_worker() const { return !(dedicated && rank == 0); }
  int first_worker() const { return dedicated ? 1 : 0; }
};
static unsigned long walk_roles(bool print) {
  unsigned long rows = 0;
  const uint32_t npx = 160 * 90, cap = 5120;
  const size_t n = 1000, hit_floats = 8 + (size_t)npx * 8;
  for (int dedicated = 0; dedicated < 2; ++dedicated)
    for (int world = 1 + dedicated; world <= 32; ++world) {
      int sends_to_0 = 0;
      for (int rank = 0; rank < world; ++rank) {
        const OldRoles O{rank, world, dedicated != 0};
        const SlabRoles P{rank, world, dedicated != 0};
        CHECK(P.worker() == O.is_worker() && P.first_worker() == O.first_worker());
        // tsdf_halo_exchange: nothing behind `if (!is_worker(c)) return`; else the two offsets into d_halo_gath, or null
        const long old_below = O.is_worker() && rank > O.first_worker() ? (long)(((size_t)(rank - 1) * 2 + 1) * n) : -1;
        const long old_above = O.is_worker() && rank < world - 1 ? (long)(((size_t)(rank + 1) * 2 + 0) * n) : -1;
        const SlabRoles::Face lo = P.below(), hi = P.above();
        CHECK((lo.row != SlabRoles::kNone ? (long)SlabRoles::face_offset(lo, n) : -1) == old_below);
        CHECK((hi.row != SlabRoles::kNone ? (long)SlabRoles::face_offset(hi, n) : -1) == old_above);
        // exchange_hits
        CHECK(P.own_in_parts() == (rank == 0));
        for (int first = 0; first < 2; ++first) CHECK(P.exports(first != 0) == (O.is_worker() && (first || rank != 0)));
        CHECK(P.export_records(npx, cap) == (rank == 0 ? npx : cap));
        CHECK(SlabRoles::exchange_floats(cap) == 8 + (size_t)cap * 8 && SlabRoles::row_floats(npx) == hit_floats);
        CHECK(P.grouped() == (world > 1) && P.gathers() == (rank == 0));
        if (rank == 0) {                                     // for (r = 1; r < world; ++r) Recv(d_hitparts + r * hit_floats, ..., r)
          int r = 1;
          for (int q = P.recv_begin(); q < P.world; ++q, ++r) CHECK(q == r && SlabRoles::row_offset(q, hit_floats) == (size_t)r * hit_floats);
          CHECK(r == world && P.send_to() == SlabRoles::kNone);
        } else {                                             // Send(d_hitbuf, ..., 0)
          CHECK(P.recv_begin() >= P.world && P.send_to() == 0);
          ++sends_to_0;
        }
        // on their own: a compositor has no neighbours and exports nothing; on a repeated exchange rank 0 does not export, every other worker does
        if (!P.worker()) CHECK(lo.row == SlabRoles::kNone && hi.row == SlabRoles::kNone && !P.exports(true) && !P.exports(false));
        CHECK(P.exports(false) == (P.worker() && rank != 0) && P.exports(true) == P.worker());
        if (print)
          std::printf("%d %d %d : %d %d %d %d %d %d %d %d %d %d %u %d %d %d %d %zu %zu\n", world, dedicated, rank, (int)P.worker(), P.first_worker(), (int)P.gathers(), lo.row, lo.face,
                      hi.row, hi.face, (int)P.own_in_parts(), (int)P.exports(true), (int)P.exports(false), P.export_records(npx, cap), (int)P.grouped(), P.recv_begin(), P.send_to(),
                      0, SlabRoles::exchange_floats(cap), SlabRoles::row_floats(npx));
        ++rows;
      }
      CHECK(sends_to_0 == world - 1);                        // every other rank sends exactly once, to 0
      // the workers' links form ONE chain from the first worker to world - 1: r -> r + 1 reads face 0 of row r + 1, the way back face 1 of row r
      const int first = dedicated ? 1 : 0;
      int r = first, visited = 1;
      CHECK((SlabRoles{r, world, dedicated != 0}.below().row == SlabRoles::kNone));
      while (true) {
        const SlabRoles::Face up = SlabRoles{r, world, dedicated != 0}.above();
        if (up.row == SlabRoles::kNone) break;
        CHECK(up.row == r + 1 && up.face == 0);
        const SlabRoles::Face down = SlabRoles{up.row, world, dedicated != 0}.below();
        CHECK(down.row == r && down.face == 1);
        r = up.row; ++visited;
        CHECK(visited <= world);
      }
      CHECK(r == world - 1 && visited == world - first);
    }
  return rows;
}

// ---- (c) replay event scripts through the header, one decision line per event.  "B npx min max": a new communicator (a fresh book, then its limits);
// "g m": gather, the frame's own largest hit count m; "f": finish; "s frame"; "l min max"; "r": buffers released
static int replay(const char* path) {
  std::FILE* in = std::fopen(path, "r");
  CHECK(in);
  GatherBook book; uint32_t table[3] = {0, 0, 0}; uint32_t npx = 0;
  char line[128];
  while (std::fgets(line, sizeof line, in)) {
    unsigned long long a = 0, b = 0, c = 0;
    const char ev = line[0];
    std::sscanf(line + 1, "%llu %llu %llu", &a, &b, &c);
    if (ev == 'B') {
      CHECK(a <= 16384ull * 16384ull);
      book = GatherBook{}; book.set_limits((uint32_t)b, (uint32_t)c); npx = (uint32_t)a; std::memset(table, 0, sizeof table);
      std::printf("B\n");
      continue;
    } else if (ev == 'g') {
      CHECK(a <= (unsigned long long)npx + 1);               // m <= npx + 1 <= 16384^2 + 1: m * 3 does not wrap
      const int lagged = book.lagged_slot();
      const uint32_t cap = book.open(npx, lagged >= 0 ? table[lagged] : 0);
      const int slot = book.open_slot();
      table[slot] = (uint32_t)a; book.queued(cap);
      std::printf("g %u %d %d", cap, lagged, slot);
    } else if (ev == 'f') {
      const int pending = book.pending_slot();
      const GatherBook::Repair r = book.finish(npx, pending >= 0 ? table[pending] : 0);
      std::printf("f %d %u %d", (int)r.regather, r.cap, pending);
    } else if (ev == 's') {
      const GatherBook::Status S = book.status(a);
      const int t = S.kind == GatherBook::Status::kCompare ? (table[S.slot] > S.cap ? 1 : 0) : S.truncated;
      std::printf("s %d %d %d %u", (int)S.kind, t, S.slot, S.cap);
    } else if (ev == 'l') {
      book.set_limits((uint32_t)a, (uint32_t)b);
      std::printf("l");
    } else {
      CHECK(ev == 'r');
      book.released(); std::memset(table, 0, sizeof table);
      std::printf("r");
    }
    std::printf(" | %u %u %llu\n", book.regathers, book.overflowed_frames, (unsigned long long)book.frame_no);
  }
  std::fclose(in);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "replay")) return replay(argv[2]);
  if (argc == 2 && !std::strcmp(argv[1], "roles")) { walk_roles(true); return 0; }
  // a communicator before its first gather: the loose fields' initial values are a fresh book's, and a fresh book answers "not gathered yet"
  { const OldComm o; const NewComm n; int seq[1] = {0}; statuses_agree(o, n, seq, 0); g_status_rows = 0; CHECK(n.book.min_capacity == 4096 && n.book.max_capacity == 0); }
  static_assert(GatherBook::kLag == 2 && GatherBook::kRing == 3 && GatherBook::kVerdicts == 64, "the lag and the ring sizes are not this change's to move");
  walk_book();
  std::printf("against the old statements: %lu sequences, %lu rows, %lu status rows\n", g_sequences, g_rows, g_status_rows);
  CHECK(g_sequences == 2ul * 35831808);                      // 12^7 per start
  CHECK(g_rows == 2ul * 39089244 && g_status_rows == 6 * g_rows);   // 12 + 12^2 + ... + 12^7 per start, six frames asked about behind each
  g_status_rows = 0;
  const unsigned long gone = walk_long();
  std::printf("260 frames: %lu status rows, %lu frames no longer kept\n", g_status_rows, gone);
  CHECK(g_status_rows == 260ul * 261 / 2 + 260 && gone == 196);   // frames 0 .. f + 1 asked about behind frame f; at the end frames 0 .. 195 have left the ring
  const unsigned long roles = walk_roles(false);
  std::printf("roles: %lu rows\n", roles);
  CHECK(roles == 1055);                                      // 1 + ... + 32 shared, 2 + ... + 32 dedicated
  std::puts("slab exchange ok");
  return 0;
}
'''


def _load_twin():
    spec = importlib.util.spec_from_file_location("slab_exchange_twin", os.path.join(ROOT, "rgbd-recon_amd", "slab_exchange.py"))   # (no torch on this path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("slab_exchange")
    src = d / "slab_exchange_main.cpp"
    src.write_text(MAIN)
    out = str(d / "slab_exchange_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, str(src), "-o", out])
    return out


def test_the_header_includes_only_what_it_may():
    text = open(os.path.join(CSRC, "slab_exchange.hpp")).read()
    assert sorted(l.split()[1] for l in text.splitlines() if l.startswith("#include")) == ["<algorithm>", "<cstdint>"]


def test_book_against_the_old_statements_and_roles_in_every_world(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0 and "slab exchange ok" in p.stdout, p.stdout + p.stderr


# ---- (c) the same scripts through the Python book
def _replay_py(tw, lines, as_the_driver_builds_it=False):
    out, book, table, npx = [], None, [0, 0, 0], 0
    for line in lines:
        ev, args = line[0], [int(v) for v in line[1:].split()]
        if ev == "B":
            npx, table = args[0], [0, 0, 0]
            if as_the_driver_builds_it:
                assert args[2] == 0
                book = tw.GatherBook(args[1])                 # SlabDriver: GatherBook(min_capacity), no maximum
            else:
                book = tw.GatherBook()
                book.set_limits(args[1], args[2])
            out.append("B")
            continue
        if ev == "g":
            lagged = book.lagged_slot()
            cap = book.open(npx, table[lagged] if lagged >= 0 else 0)
            slot = book.open_slot()
            table[slot] = args[0]
            book.queued(cap)
            s = f"g {cap} {lagged} {slot}"
        elif ev == "f":
            pending = book.pending_slot()
            regather, cap = book.finish(npx, table[pending] if pending >= 0 else 0)
            s = f"f {int(regather)} {cap} {pending}"
        elif ev == "s":
            kind, t, slot, cap = book.status(args[0])
            if kind == tw.GatherBook.COMPARE:
                t = int(table[slot] > cap)
            s = f"s {kind} {t} {slot} {cap}"
        elif ev == "l":
            book.set_limits(args[0], args[1])
            s = "l"
        else:
            assert ev == "r"
            book.released()
            table = [0, 0, 0]
            s = "r"
        out.append(f"{s} | {book.regathers} {book.overflowed_frames} {book.frame_no}")
    return out


TRIPLES = [(160 * 90, 4096, 0), (160 * 90, 4, 0), (160 * 90, 4, 64), (1280 * 720, 4096, 0), (1280 * 720, 64, 5000), (16384 * 16384, 4096, 0),
           (16384 * 16384, 1, 1 << 27)]


def _scripts(tw):
    """[(max, lines)]: the long LCG sequence at each triple, then 1001 random scripts of 30 events.  The hit counts are chosen around the capacity the
    (Python) book hands out; the C++ replay is handed the same numbers."""
    rng = random.Random(20240917)
    scripts = []

    def one(npx, lo, hi, n_events, lcg):
        book, table, lines, x = tw.GatherBook(), [0, 0, 0], [f"B {npx} {lo} {hi}"], 12345
        book.set_limits(lo, hi)
        for _ in range(n_events):
            if lcg:
                x = (x * 1664525 + 1013904223) & 0xffffffff
                kind = "g" if (x >> 28) < 13 else "f" if (x >> 28) < 15 else "s"
            else:
                kind = rng.choice("ggggggfffssslr")
            if kind == "g":
                lagged = book.lagged_slot()
                cap = book.open(npx, table[lagged] if lagged >= 0 else 0)
                if lcg:
                    m = (x >> 8) % (npx + 2) if x & 3 == 0 else (x >> 8) % 30000 % (npx + 2)
                else:
                    m = rng.choice([0, book.min_capacity - 1, cap, cap + 1, npx, npx + 1, rng.randrange(npx + 2), rng.randrange(min(npx, 20000) + 1)])
                table[book.open_slot()] = m
                book.queued(cap)
                lines.append(f"g {m}")
            elif kind == "f":
                pending = book.pending_slot()
                book.finish(npx, table[pending] if pending >= 0 else 0)
                lines.append("f")
            elif kind == "s":
                lines.append(f"s {max(0, book.frame_no - rng.randrange(0, 8 if not lcg else 80))}")
            elif kind == "l":
                mn = rng.choice([1, 4, 64, 4096])
                lines.append(f"l {mn} {0 if hi == 0 else rng.choice([0, mn, mn + 60, 1 << 20])}")
            else:
                book.released()
                table = [0, 0, 0]
                lines.append("r")
        scripts.append((hi, lines))

    for npx, lo, hi in TRIPLES:
        one(npx, lo, hi, 300, True)
    for k in range(1001):
        one(*TRIPLES[k % len(TRIPLES)], 30, False)
    return scripts


def test_cpp_book_and_python_book_decide_alike(exe, tmp_path):
    tw = _load_twin()
    scripts = _scripts(tw)
    assert len(scripts) == len(TRIPLES) + 1001 and all(len(s) == 31 for _, s in scripts[len(TRIPLES):])
    path = tmp_path / "scripts.txt"
    path.write_text("".join(l + "\n" for _, s in scripts for l in s))
    p = subprocess.run([exe, "replay", str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr
    got = p.stdout.splitlines()
    want = [l for _, s in scripts for l in _replay_py(tw, s)]
    assert len(got) == len(want) == sum(len(s) for _, s in scripts)
    assert got == want
    # the torch path's book has no maximum: built the way SlabDriver builds it, it decides what the header decides in the scripts without one
    k, n_driver = 0, 0
    for hi, s in scripts:
        if hi == 0:
            assert _replay_py(tw, s, as_the_driver_builds_it=True) == got[k:k + len(s)]
            n_driver += 1
        k += len(s)
    assert n_driver == 4 + 4 * 143                            # four of the seven triples have no maximum
    # the decisions are not all alike: repairs, overflows and every status answer occur
    assert any(l.startswith("f 1") for l in got) and all(any(l.startswith(f"s {kind} ") for l in got) for kind in range(4))
    assert any(l.split(" | ")[1].split()[1] != "0" for l in got if " | " in l)


def test_python_roles_against_the_header(exe):
    tw = _load_twin()
    p = subprocess.run([exe, "roles"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    rows = p.stdout.splitlines()
    assert len(rows) == 1055
    npx, cap = 160 * 90, 5120
    want = []
    for dedicated in (0, 1):
        for world in range(1 + dedicated, 33):
            for rank in range(world):
                P = tw.SlabRoles(rank, world, bool(dedicated))
                lo, hi = P.below(), P.above()
                want.append(f"{world} {dedicated} {rank} : {int(P.worker)} {P.first_worker} {int(P.gathers)} {lo[0]} {lo[1]} {hi[0]} {hi[1]} {int(P.own_in_parts)} "
                            f"{int(P.exports(True))} {int(P.exports(False))} {P.export_records(npx, cap)} {int(P.grouped)} {P.recv_begin()} {P.send_to()} 0 "
                            f"{P.exchange_floats(cap)} {P.row_floats(npx)}")
    assert rows == want
