"""CPU: the result rings' protocol (rgbd-recon_amd/csrc/result_paths.hpp, HIP-free) as a stand-alone program with its own main, built with the host
address and undefined-behaviour sanitizers.  Two walks.  (1) ResultRing against the statements it replaced -- the frame read-out's loose present_* fields
and the mesh stream's slots / head / count / held, as they stood in abi.cpp, restated here as two small structs: every state (2..8 slots x head < slots x
count <= slots x held) x every event, the refused ones included; the value handed out and the next state must agree, row by row.  (2) The states reachable
from configure(), with a shadow queue of tags kept from the returned values alone, for what the protocol promises: a frame is never written into a slot
that is queued or held, frames come out in the order they went in, held implies count >= 1, count <= slots, a refused event changes nothing, reset gives
the configured idle ring."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbd-recon_amd", "csrc")

MAIN = r'''
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <set>
#include <vector>
#include "result_paths.hpp"
using namespace rr;
#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #x); std::exit(1); } } while (0)

// ---- the statements ResultRing replaced, as they stood (the HIP calls between them left out).  Each method is one site of abi.cpp; -1 / false = the
// site's FAIL, which returns before anything is written.
struct OldPresent {                                      // tsdf_ctx::present_*
  uint32_t present_slots = 3, present_head = 0, present_count = 0; bool present_held = false;
  void released() { present_head = 0; present_count = 0; present_held = false; }                    // release_present
  void config(uint32_t slots) { released(); present_slots = slots; }                                // tsdf_present_config
  bool busy() const { if (present_count) return true; return false; }                               // tsdf_present_config, tsdf_resize
  bool all_taken() const { if (present_count >= present_slots) return true; return false; }         // tsdf_present
  int push() {
    if (present_count >= present_slots) return -1;
    const uint32_t k = (present_head + present_count) % present_slots;
    ++present_count;
    return (int)k;
  }
  uint32_t queued(uint32_t k) const { return (present_head + k) % present_slots; }                  // (the read-out walks no queue: the same arithmetic)
  uint32_t oldest() const { return present_head; }                                                  // tsdf_present_acquire
  int verdict() const { if (!present_count) return 1; if (present_held) return 2; return 0; }
  bool hold() { if (verdict()) return false; present_held = true; return true; }
  bool release() {                                                                                   // tsdf_present_release
    if (!present_held) return false;
    present_held = false;
    present_head = (present_head + 1) % present_slots;
    --present_count;
    return true;
  }
  void set(uint32_t s, uint32_t h, uint32_t n, bool held) { present_slots = s; present_head = h; present_count = n; present_held = held; }
  bool same(const ResultRing& r) const { return present_slots == r.slots && present_head == r.head && present_count == r.count && present_held == r.held; }
};
struct OldMeshStream {                                   // tsdf_ctx::MeshStream
  uint32_t slots = 0, head = 0, count = 0; bool held = false;
  void released() { head = 0; count = 0; held = false; }                                            // release_mesh_stream
  void config(uint32_t n) { released(); slots = n; }                                                // tsdf_mesh_stream_config_lod
  bool busy() const { if (count) return true; return false; }                                       // tsdf_mesh_stream_config_lod, tsdf_set_voxel_size
  bool all_taken() const { if (count >= slots) return true; return false; }                         // tsdf_mesh_stream
  int push() {
    if (count >= slots) return -1;
    const uint32_t k = (head + count) % slots;
    ++count;
    return (int)k;
  }
  uint32_t queued(uint32_t k) const { return (head + k) % slots; }                                  // mesh_stream_pump
  uint32_t oldest() const { return head; }                                                          // tsdf_mesh_stream_acquire
  int verdict() const { if (!count) return 1; if (held) return 2; return 0; }
  bool hold() { if (verdict()) return false; held = true; return true; }
  bool release() {                                                                                   // tsdf_mesh_stream_release
    if (!held) return false;
    held = false;
    head = (head + 1) % slots;
    --count;
    return true;
  }
  void set(uint32_t s, uint32_t h, uint32_t n, bool hd) { slots = s; head = h; count = n; held = hd; }
  bool same(const ResultRing& r) const { return slots == r.slots && head == r.head && count == r.count && held == r.held; }
};

enum Event { CONFIGURE, RESET, IDLE, FULL, PUSH, QUEUED, OLDEST, ACQUIRE, HOLD, RELEASE, N_EVENTS };

template <class Old> long apply_old(Old& o, int ev, uint32_t in) {
  switch (ev) {
    case CONFIGURE: o.config(in); return 0;
    case RESET: o.released(); return 0;
    case IDLE: return !o.busy();
    case FULL: return o.all_taken();
    case PUSH: return o.push();
    case QUEUED: return (long)o.queued(in);
    case OLDEST: return (long)o.oldest();
    case ACQUIRE: return o.verdict();
    case HOLD: return o.hold();
    default: return o.release();
  }
}
static long apply_new(ResultRing& r, int ev, uint32_t in) {
  switch (ev) {
    case CONFIGURE: r.configure(in); return 0;
    case RESET: r.reset(); return 0;
    case IDLE: return r.idle();
    case FULL: return r.full();
    case PUSH: return r.push();
    case QUEUED: return (long)r.queued(in);
    case OLDEST: return (long)r.oldest();
    case ACQUIRE: return (long)r.acquire();
    case HOLD: return r.hold();
    default: return r.release();
  }
}
// every state x every event x every input of the event
template <class Old> unsigned long walk_against() {
  unsigned long rows = 0;
  for (uint32_t slots = 2; slots <= kMaxResultSlots; ++slots)
    for (uint32_t head = 0; head < slots; ++head)
      for (uint32_t count = 0; count <= slots; ++count)
        for (int held = 0; held < 2; ++held)
          for (int ev = 0; ev < N_EVENTS; ++ev) {
            const uint32_t in_lo = ev == CONFIGURE ? 2 : 0, in_hi = ev == CONFIGURE ? kMaxResultSlots : ev == QUEUED ? kMaxResultSlots - 1 : 0;
            for (uint32_t in = in_lo; in <= in_hi; ++in) {
              Old o; o.set(slots, head, count, held != 0);
              ResultRing r{slots, head, count, held != 0};
              CHECK(o.same(r));
              const long a = apply_old(o, ev, in), b = apply_new(r, ev, in);
              if (a != b || !o.same(r)) {
                std::fprintf(stderr, "slots %u head %u count %u held %d, event %d(%u): old %ld, new %ld -> slots %u head %u count %u held %d\n", slots, head, count, held, ev, in,
                             a, b, r.slots, r.head, r.count, (int)r.held);
                std::exit(1);
              }
              ++rows;
            }
          }
  return rows;
}

// ---- the states reachable from configure(): the ring and what a caller knows of it from the returned values alone
struct Frame { int slot; unsigned long tag; };
struct Shadow {
  ResultRing r;
  std::deque<Frame> fifo;                                // frames queued or held, oldest first
  unsigned long slot_tag[kMaxResultSlots] = {};          // what was written into each slot last
  bool held = false;
};
static unsigned long g_tag = 0;
static std::vector<int> key_of(const Shadow& s) {
  std::vector<int> k = {(int)s.r.slots, (int)s.r.head, (int)s.r.count, (int)s.r.held, (int)s.held};
  for (const Frame& f : s.fifo) k.push_back(f.slot);
  return k;
}
static bool same_ring(const ResultRing& a, const ResultRing& b) { return a.slots == b.slots && a.head == b.head && a.count == b.count && a.held == b.held; }
static void promises(const Shadow& s) {
  CHECK(s.r.count <= s.r.slots);
  CHECK(!s.r.held || s.r.count >= 1);
  CHECK(s.r.count == s.fifo.size() && s.r.held == s.held);
  CHECK(s.r.idle() == s.fifo.empty() && s.r.full() == (s.fifo.size() == s.r.slots));
  for (uint32_t k = 0; k < s.r.count; ++k) CHECK((int)s.r.queued(k) == s.fifo[k].slot);
  CHECK(s.r.acquire() == (s.fifo.empty() ? kResultNoneQueued : s.held ? kResultAlreadyHeld : kResultGo));
}
static unsigned long walk_reachable() {
  std::set<std::vector<int>> seen;
  std::vector<Shadow> todo;
  for (uint32_t slots = 2; slots <= kMaxResultSlots; ++slots) { Shadow s; s.r.configure(slots); todo.push_back(s); }
  unsigned long steps = 0;
  while (!todo.empty()) {
    const Shadow s = todo.back(); todo.pop_back();
    if (!seen.insert(key_of(s)).second) continue;
    promises(s);
    for (int ev = 0; ev < 5; ++ev) {
      Shadow t = s;
      const ResultRing before = t.r;
      switch (ev) {
        case 0: {                                        // a frame is written
          const int k = t.r.push();
          if (t.fifo.size() == t.r.slots) { CHECK(k == -1 && same_ring(t.r, before)); break; }
          CHECK(k >= 0 && k < (int)t.r.slots);
          for (const Frame& f : t.fifo) CHECK(f.slot != k);                   // never a slot that is queued or held
          t.slot_tag[k] = ++g_tag; t.fifo.push_back(Frame{k, g_tag});
          break;
        }
        case 1: {                                        // the oldest is handed out
          const bool go = t.r.hold();
          if (t.fifo.empty() || t.held) { CHECK(!go && same_ring(t.r, before)); break; }
          CHECK(go && (int)t.r.oldest() == t.fifo.front().slot && t.slot_tag[t.r.oldest()] == t.fifo.front().tag);   // in the order they went in
          t.held = true;
          break;
        }
        case 2: {                                        // ... and given back
          const bool ok = t.r.release();
          if (!t.held) { CHECK(!ok && same_ring(t.r, before)); break; }
          CHECK(ok);
          t.fifo.pop_front(); t.held = false;
          break;
        }
        case 3: {                                        // the buffers are dropped
          t.r.reset();
          ResultRing fresh; fresh.configure(before.slots);
          CHECK(same_ring(t.r, fresh));
          t.fifo.clear(); t.held = false;
          break;
        }
        default: {                                       // another size (abi.cpp configures an idle ring only; the ring itself takes it from any state)
          const uint32_t n = before.slots == kMaxResultSlots ? 2 : before.slots + 1;
          t.r.configure(n);
          CHECK(t.r.slots == n && t.r.idle() && !t.r.held && t.r.oldest() == 0);
          t.fifo.clear(); t.held = false;
          break;
        }
      }
      ++steps;
      todo.push_back(t);
    }
  }
  std::printf("reachable: %zu states, %lu steps\n", seen.size(), steps);
  return (unsigned long)seen.size();
}

int main() {
  // a context's read-out ring before any tsdf_present_config: three slots, idle
  { const OldPresent o; const ResultRing r{3, 0, 0, false}; CHECK(o.same(r)); }
  const unsigned long a = walk_against<OldPresent>(), b = walk_against<OldMeshStream>();
  // states: sum over slots 2..8 of slots * (slots + 1) * 2 = 476; inputs per state: 7 sizes + 8 queue positions + 8 events without input = 23
  std::printf("against the read-out's statements: %lu rows; against the mesh stream's: %lu rows\n", a, b);
  CHECK(a == 476ul * 23 && b == a);
  // reachable: per ring of n slots, head < n x (idle | 1..n queued x held or not) = n * (2 n + 1) states; 2..8 slots: 441
  CHECK(walk_reachable() == 441);
  std::puts("result paths ok");
  return 0;
}
'''


def test_result_ring_against_the_old_statements_and_its_promises(tmp_path):
    src = tmp_path / "result_paths_main.cpp"
    src.write_text(MAIN)
    exe = str(tmp_path / "result_paths_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, str(src), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout)
    assert p.returncode == 0 and "result paths ok" in p.stdout, p.stdout + p.stderr
