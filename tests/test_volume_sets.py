"""CPU: the volume sets' bookkeeping (rgbd-recon_amd/csrc/volume_sets.hpp, HIP-free) as a stand-alone program with its own main, built with the host
address and undefined-behaviour sanitizers.  Two walks.  (1) TileHistory against the statements it replaced -- tsdf_ctx's loose tile_parity / full_classify /
frame_stamp, as they stood at each site of abi.cpp, restated here as one small struct: every state (parity x full x stamp in {0, 1, 2, 0xfffffffe,
0xffffffff}) x every event; the values handed out and the next state must agree, row by row, the stamp's wrap to 1 with its wipe and full walk included.
(2) Two sets under DrawLanes, in the old form (the set in use as loose fields, the other one as `alt`, exchanged field by field) and in the new one
(vset[lanes.set()], bound by one function), with small integers for the device buffers: every sequence of six events; after each event both forms must
have bound the same buffers, promise the same next integrate() and select the same last list, in the new form a released pair is all null, and no set is
ever allocated twice."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbd-recon_amd", "csrc")

MAIN = r'''
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>
#include "draw_lanes.hpp"
#include "volume_sets.hpp"
using namespace rr;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #x); std::exit(1); } } while (0)

// ---- (1) the statements TileHistory replaced, as they stood (the HIP calls between them left out).  Each method is one site of abi.cpp
struct OldTiles {                                        // tsdf_ctx::tile_parity, full_classify, frame_stamp
  int tile_parity = 0; bool full_classify = true; uint32_t frame_stamp = 0;
  struct Begin { int list, prev, next; uint32_t stamp; bool wipe, full; };
  Begin integrate_begin(bool use_bricks) {               // tsdf_integrate, in front of the launches: the indices into d_tile_list / d_tile_counts it bound,
    Begin b{-1, -1, -1, 0, false, false};                // whether it wiped the stamps, and what launch_classify_tiles was given
    if (use_bricks) {
      const int p = tile_parity;
      b.list = p; b.prev = p ^ 1; b.next = p ^ 1;
      if (++frame_stamp == 0) { frame_stamp = 1; full_classify = true; b.wipe = true; }
    }
    b.stamp = frame_stamp; b.full = full_classify;
    return b;
  }
  void integrate_end(bool use_bricks) {                  // tsdf_integrate, behind the launches
    if (use_bricks) { tile_parity ^= 1; full_classify = false; }
    else full_classify = true;
  }
  int integrate_stats() const { const int p = tile_parity ^ 1; return p; }          // tsdf_integrate_stats
  int download_active_tiles() const { const int p = tile_parity ^ 1; return p; }    // tsdf_download_active_tiles
  int integrate_form() const { return tile_parity ^ 1; }                            // tsdf_integrate_form
  void setup_bricks() { full_classify = true; }
  void set_tsdf_limit() { full_classify = true; }
  void upload_volume() { full_classify = true; }
  void release_volume() { tile_parity = 0; full_classify = true; frame_stamp = 0; }
  bool same(const TileHistory& h) const { return tile_parity == h.parity && full_classify == h.full && frame_stamp == h.stamp; }
};

static unsigned long walk_history() {
  const uint32_t stamps[5] = {0u, 1u, 2u, 0xfffffffeu, 0xffffffffu};
  enum { BEGIN_CULLED, BEGIN_DENSE, END_CULLED, END_DENSE, LAST, INVALIDATE, RESET, N_EVENTS };
  unsigned long rows = 0;
  for (int parity = 0; parity < 2; ++parity)
    for (int full = 0; full < 2; ++full)
      for (uint32_t stamp : stamps)
        for (int ev = 0; ev < N_EVENTS; ++ev)
          for (int site = 0; site < 3; ++site) {           // LAST and INVALIDATE stood at three sites each
            if (site && ev != LAST && ev != INVALIDATE) continue;
            OldTiles o; o.tile_parity = parity; o.full_classify = full != 0; o.frame_stamp = stamp;
            TileHistory h; h.parity = parity; h.full = full != 0; h.stamp = stamp;
            CHECK(o.same(h) && h.full_walk() == o.full_classify);
            bool ok = true;
            switch (ev) {
              case BEGIN_CULLED: {
                const OldTiles::Begin a = o.integrate_begin(true); const TileHistory::Begin b = h.begin(true);
                ok = a.list == b.list && a.prev == b.prev && a.next == b.prev && a.stamp == b.stamp && a.wipe == b.wipe && a.full == h.full_walk();
                CHECK(b.stamp != 0 && b.list != b.prev);
                if (stamp == 0xffffffffu) CHECK(b.stamp == 1 && b.wipe && h.full_walk());          // the wrap: to 1, never to 0, with the wipe and the full walk
                else CHECK(b.stamp == stamp + 1 && !b.wipe && h.full_walk() == (full != 0));
                break;
              }
              case BEGIN_DENSE: {
                const OldTiles::Begin a = o.integrate_begin(false); const TileHistory::Begin b = h.begin(false);
                ok = a.stamp == b.stamp && !b.wipe && a.full == h.full_walk();                       // (no launch of a dense integrate reads the lists)
                CHECK(h.parity == parity && h.full == (full != 0) && h.stamp == stamp);              // it changes nothing
                break;
              }
              case END_CULLED: o.integrate_end(true); h.end(true); CHECK(!h.full_walk() && h.last() == parity); break;
              case END_DENSE: o.integrate_end(false); h.end(false); CHECK(h.full_walk()); break;
              case LAST: ok = (site == 0 ? o.integrate_stats() : site == 1 ? o.download_active_tiles() : o.integrate_form()) == h.last(); break;
              case INVALIDATE:
                if (site == 0) o.setup_bricks(); else if (site == 1) o.set_tsdf_limit(); else o.upload_volume();
                h.invalidate(); CHECK(h.full_walk());
                break;
              default: o.release_volume(); h.reset(); { const TileHistory fresh; CHECK(h.parity == fresh.parity && h.full == fresh.full && h.stamp == fresh.stamp); } break;
            }
            if (!ok || !o.same(h)) {
              std::fprintf(stderr, "parity %d full %d stamp %u, event %d site %d: new -> parity %d full %d stamp %u\n", parity, full, stamp, ev, site, h.parity, (int)h.full, h.stamp);
              std::exit(1);
            }
            ++rows;
          }
  return rows;
}

// ---- (2) two sets under DrawLanes.  A device buffer is a small integer (0 = null) from one counter, never handed out twice; a count word is its
// buffer's number * 2 + the word's index.  What the kernels are given: Volume::data / cls, and of TileState the pointers
struct Bound {
  int data = 0, vol_cls = 0, cls = 0, stamp = 0, list = 0, prev_list = 0, count = 0, prev_count = 0, next_count = 0;
  bool operator==(const Bound& o) const {
    return data == o.data && vol_cls == o.vol_cls && cls == o.cls && stamp == o.stamp && list == o.list && prev_list == o.prev_list && count == o.count &&
           prev_count == o.prev_count && next_count == o.next_count;
  }
};
struct Last { int list, count; bool operator==(const Last& o) const { return list == o.list && count == o.count; } };
struct Alloc {
  int next = 1; bool fail = false;
  bool get(int* p) { if (fail) return false; *p = next++; return true; }
};

// the old form: abi.cpp's statements over tsdf_ctx's loose fields and `alt`, site by site
struct OldCtx {
  DrawLanes lanes; Alloc mem; Bound b;                   // b.data = vol.data, b.stamp = tiles.stamp: the two the old form owned through the bound copies
  int d_cls_all = 0, d_tile_list[2] = {0, 0}, d_tile_counts = 0; int tile_parity = 0; bool full_classify = true; uint32_t frame_stamp = 0;
  struct VolSet { int data = 0, cls_all = 0, stamp = 0, list[2] = {0, 0}, counts = 0; int parity = 0; bool full = true; uint32_t stampno = 0; } alt;
  std::vector<int> marked;                               // the class arrays launch_mark_all_mixed was given, in order

  void swap_volume_set() {
    VolSet& a = alt;
    std::swap(b.data, a.data); std::swap(d_cls_all, a.cls_all); std::swap(b.stamp, a.stamp);
    std::swap(d_tile_list[0], a.list[0]); std::swap(d_tile_list[1], a.list[1]); std::swap(d_tile_counts, a.counts);
    std::swap(tile_parity, a.parity); std::swap(full_classify, a.full); std::swap(frame_stamp, a.stampno);
    b.vol_cls = d_cls_all;
    b.cls = d_cls_all;
    b.list = d_tile_list[0]; b.count = d_tile_counts * 2;
  }
  bool ensure_alt_set() {
    VolSet& a = alt;
    if (a.data) return true;
    const bool ok = mem.get(&a.data) && mem.get(&a.stamp) && mem.get(&a.cls_all) && mem.get(&a.list[0]) && mem.get(&a.list[1]) && mem.get(&a.counts);
    if (!ok) { a = VolSet{}; lanes.second_set_unavailable(); return false; }
    a.parity = 0; a.full = true; a.stampno = 0;
    return true;
  }
  void release_volume() {
    alt = VolSet{}; lanes.volume_released();
    b.data = 0; b.stamp = 0; d_cls_all = 0;
    d_tile_list[0] = d_tile_list[1] = 0; d_tile_counts = 0;
    tile_parity = 0; full_classify = true; frame_stamp = 0;
  }
  void setup_volume() {
    release_volume();
    mem.get(&b.data);
    mem.get(&b.stamp);
    mem.get(&d_cls_all);
    b.vol_cls = d_cls_all;
    b.cls = d_cls_all;
    for (int k = 0; k < 2; ++k) mem.get(&d_tile_list[k]);
    mem.get(&d_tile_counts);
    b.list = d_tile_list[0]; b.count = d_tile_counts * 2;
  }
  void integrate(bool deep_ok, bool use_bricks) {        // tsdf_integrate
    if (deep_ok && !lanes.second_set_failed() && ensure_alt_set()) { lanes.integrate(); swap_volume_set(); }
    else lanes.join_integ();
    if (use_bricks) {
      const int p = tile_parity;
      b.list = d_tile_list[p]; b.count = d_tile_counts * 2 + p;
      b.prev_list = d_tile_list[p ^ 1]; b.prev_count = d_tile_counts * 2 + (p ^ 1); b.next_count = d_tile_counts * 2 + (p ^ 1);
      if (++frame_stamp == 0) { frame_stamp = 1; full_classify = true; }
    }
    if (use_bricks) { tile_parity ^= 1; full_classify = false; }
    else full_classify = true;
  }
  void setup_bricks() { full_classify = true; alt.full = true; }
  void set_tsdf_limit() {
    marked.push_back(b.cls);
    full_classify = true;
    if (alt.data) { marked.push_back(alt.cls_all); alt.full = true; }
  }
  void upload_volume() { marked.push_back(b.cls); full_classify = true; }
  Last last() const { const int p = tile_parity ^ 1; return Last{d_tile_list[p], d_tile_counts * 2 + p}; }   // the three read-back calls
};

// the new form: tsdf_ctx::vset and abi.cpp's functions over it
struct NewCtx {
  DrawLanes lanes; Alloc mem; Bound b;
  struct VolSet { int data = 0, cls = 0, stamp = 0, list[2] = {0, 0}, counts = 0; TileHistory history{}; } vset[2];
  std::vector<int> marked;

  VolSet& set_in_use() { return vset[lanes.set()]; }
  static void bind_volume_set(const VolSet& s, Bound& B) {
    B.data = s.data; B.vol_cls = s.cls;
    B.cls = s.cls; B.stamp = s.stamp;
    B.list = s.list[0]; B.count = s.counts * 2;
  }
  static void free_volume_set(VolSet& s) { s = VolSet{}; }
  bool alloc_volume_set(VolSet& s) {
    CHECK(!s.data && !s.cls && !s.stamp && !s.list[0] && !s.list[1] && !s.counts);     // never a set that exists
    bool ok = mem.get(&s.data);
    if (ok) ok = mem.get(&s.stamp);
    if (ok) ok = mem.get(&s.cls);
    for (int k = 0; k < 2 && ok; ++k) ok = mem.get(&s.list[k]);
    if (ok) ok = mem.get(&s.counts);
    if (!ok) { free_volume_set(s); return false; }
    s.history.reset();
    return true;
  }
  bool ensure_other_set() {
    VolSet& s = vset[lanes.set() ^ 1];
    if (s.data) return true;
    if (!alloc_volume_set(s)) { lanes.second_set_unavailable(); return false; }
    return true;
  }
  void release_volume() {
    for (VolSet& s : vset) free_volume_set(s);
    lanes.volume_released();
    b.data = 0; b.stamp = 0;
    for (const VolSet& s : vset) {                         // a released pair is all null, its histories a fresh set's
      const TileHistory fresh;
      CHECK(!s.data && !s.cls && !s.stamp && !s.list[0] && !s.list[1] && !s.counts);
      CHECK(s.history.parity == fresh.parity && s.history.full == fresh.full && s.history.stamp == fresh.stamp);
    }
  }
  void setup_volume() {
    release_volume();
    VolSet& s = set_in_use();
    CHECK(alloc_volume_set(s));
    bind_volume_set(s, b);
  }
  void integrate(bool deep_ok, bool use_bricks) {
    if (deep_ok && !lanes.second_set_failed() && ensure_other_set()) { lanes.integrate(); bind_volume_set(set_in_use(), b); }
    else lanes.join_integ();
    VolSet& set = set_in_use();
    const TileHistory::Begin T = set.history.begin(use_bricks);
    if (use_bricks) {
      b.list = set.list[T.list]; b.count = set.counts * 2 + T.list;
      b.prev_list = set.list[T.prev]; b.prev_count = b.next_count = set.counts * 2 + T.prev;
    }
    set.history.end(use_bricks);
  }
  void setup_bricks() { for (VolSet& s : vset) s.history.invalidate(); }
  void set_tsdf_limit() {
    for (int k = 0; k < 2; ++k) {
      VolSet& s = vset[lanes.set() ^ k];
      if (!s.data) continue;
      Bound B = b;
      bind_volume_set(s, B);
      marked.push_back(B.cls);
      s.history.invalidate();
    }
  }
  void upload_volume() { marked.push_back(b.cls); set_in_use().history.invalidate(); }
  Last last() { const VolSet& s = set_in_use(); const int p = s.history.last(); return Last{s.list[p], s.counts * 2 + p}; }
};

enum Event { LANE, CTX_STREAM, LANE_DENSE, CTX_STREAM_DENSE, LIMIT, BRICKS, UPLOAD, NEW_GRID, NO_MEMORY, N_EVENTS };
template <class C> void apply(C& c, int ev) {
  switch (ev) {
    case LANE: c.integrate(true, true); break;                       // integrate() on the lane (on the context's stream once the second set has failed)
    case CTX_STREAM: c.integrate(false, true); break;                // ... on the context's stream (stage overlap off, timers on, ...)
    case LANE_DENSE: c.integrate(true, false); break;                // the same two without brick culling
    case CTX_STREAM_DENSE: c.integrate(false, false); break;
    case LIMIT: c.set_tsdf_limit(); break;                           // invalidate both, marking their classes
    case BRICKS: c.setup_bricks(); break;                            // invalidate both
    case UPLOAD: c.upload_volume(); break;                           // invalidate the one in use
    case NEW_GRID: c.setup_volume(); c.setup_bricks(); break;        // release and set up again (tsdf_set_voxel_size)
    default: c.mem.fail = true; c.integrate(true, true); c.mem.fail = false; break;   // integrate() on the lane with no memory for a set it would allocate
  }
}
// what the next culled integrate() of a history would take
struct Next { bool full; uint32_t stamp; bool operator==(const Next& o) const { return full == o.full && stamp == o.stamp; } };
static Next next_of(bool full, uint32_t stamp) { OldTiles o; o.full_classify = full; o.frame_stamp = stamp; const OldTiles::Begin b = o.integrate_begin(true); return Next{b.full, b.stamp}; }
static Next next_of(TileHistory h) { const TileHistory::Begin b = h.begin(true); return Next{h.full_walk(), b.stamp}; }

static void agree(OldCtx& o, NewCtx& n, const int* seq, int len) {
  bool ok = o.b == n.b && o.last() == n.last() && o.marked == n.marked && o.lanes.set() == n.lanes.set() && o.lanes.second_set_failed() == n.lanes.second_set_failed();
  const NewCtx::VolSet& use = n.vset[n.lanes.set()]; const NewCtx::VolSet& other = n.vset[n.lanes.set() ^ 1];
  ok = ok && next_of(o.full_classify, o.frame_stamp) == next_of(use.history) && o.tile_parity == use.history.parity;
  ok = ok && next_of(o.alt.full, o.alt.stampno) == next_of(other.history) && o.alt.parity == other.history.parity;
  // the buffers each form holds: the set in use, the other one
  ok = ok && o.b.data == use.data && o.d_cls_all == use.cls && o.b.stamp == use.stamp && o.d_tile_list[0] == use.list[0] && o.d_tile_list[1] == use.list[1] && o.d_tile_counts == use.counts;
  ok = ok && o.alt.data == other.data && o.alt.cls_all == other.cls && o.alt.stamp == other.stamp && o.alt.list[0] == other.list[0] && o.alt.list[1] == other.list[1] && o.alt.counts == other.counts;
  ok = ok && o.mem.next == n.mem.next;
  if (!ok) {
    std::fprintf(stderr, "the forms disagree after events");
    for (int k = 0; k < len; ++k) std::fprintf(stderr, " %d", seq[k]);
    std::fprintf(stderr, "\n");
    std::exit(1);
  }
  CHECK(use.data && n.b.data == use.data);                                           // the set in use exists and is the one bound
  CHECK(!n.lanes.second_set_failed() || !other.data);                                // (a failed second set is not there)
}
// every sequence of kLen events, depth first: a sequence's prefix is walked once
static const int kLen = 6;
static unsigned long g_steps = 0, g_sequences = 0;
static void walk_from(const OldCtx& o, const NewCtx& n, int* seq, int depth) {
  if (depth == kLen) { ++g_sequences; return; }
  for (int ev = 0; ev < N_EVENTS; ++ev) {
    OldCtx p = o; NewCtx q = n;
    seq[depth] = ev;
    apply(p, ev); apply(q, ev); agree(p, q, seq, depth + 1); ++g_steps;
    walk_from(p, q, seq, depth + 1);
  }
}
static unsigned long walk_sets() {
  int seq[kLen] = {};
  const uint32_t seeds[2] = {0u, 0xfffffffdu};             // the stamp the first set starts from: the second one reaches the wrap inside a sequence
  for (uint32_t seed : seeds) {
    OldCtx o; NewCtx n;
    o.setup_volume(); o.setup_bricks(); n.setup_volume(); n.setup_bricks();           // tsdf_create
    o.frame_stamp = seed; n.set_in_use().history.stamp = seed;
    agree(o, n, seq, 0);
    walk_from(o, n, seq, 0);
  }
  std::printf("two sets: %lu sequences, %lu steps\n", g_sequences, g_steps);
  return g_sequences;
}

int main() {
  // a context before its first setup_volume: the loose fields' initial values are a fresh history's
  { const OldTiles o; const TileHistory h; CHECK(o.same(h) && h.full_walk()); }
  CHECK(class_offset(0, 0, 7, 5) == 0 && class_offset(2, 5, 7, 5) == 105 && class_offset(0, 1 << 9, 1 << 12, 1 << 12) == (size_t)1 << 33);
  const unsigned long rows = walk_history();
  // 20 states x (5 events at one site + 2 events at three sites)
  std::printf("against the old statements: %lu rows\n", rows);
  CHECK(rows == 20ul * 11);
  CHECK(walk_sets() == 2ul * 531441);                      // 9^6 sequences per seed
  std::puts("volume sets ok");
  return 0;
}
'''


def test_tile_history_against_the_old_statements_and_two_sets_under_the_lanes(tmp_path):
    src = tmp_path / "volume_sets_main.cpp"
    src.write_text(MAIN)
    exe = str(tmp_path / "volume_sets_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, str(src), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0 and "volume sets ok" in p.stdout, p.stdout + p.stderr
