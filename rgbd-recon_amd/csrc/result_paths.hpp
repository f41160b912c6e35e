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

// The mesh ring's slot and payload arithmetic (include/rgbd_recon_hip.h: "mesh streaming" and "mesh streaming: compact triangles").  A slot is a 64-byte
// header and a payload; the payload holds the packed vertices (stride 8 or 16) and then, in the uint32 format, the triangles (12 bytes each), in the
// tile-local format zero padding to a multiple of 16, the tile table (16 bytes a row) and the triangles (6 bytes each).  The device computes the same
// offsets from its header's counts (k_mesh.hip, k_mesh_stream_filter.hip); tests/test_mesh_compact_layout.py walks these functions on a CPU.
constexpr uint32_t kMeshIndexU32 = 0, kMeshIndexTile16 = 1;             // TSDF_MESH_INDEX_U32 / _TILE16
constexpr uint64_t kMeshHeaderBytes = 64, kMeshTileRowBytes = 16, kMeshSlotLimit = 4ull << 30;
constexpr uint64_t kMeshTapBytes = 8;                                   // sizeof(tsdf_packed_tap)
constexpr uint32_t kMeshStreamTaps = 1u;                                // TSDF_MESH_STREAM_TAPS
struct MeshFrameLayout {
  uint32_t format, stride;
  static uint64_t align16(uint64_t n) { return (n + 15u) & ~(uint64_t)15u; }
  uint64_t triangle_bytes() const { return format == kMeshIndexTile16 ? 6u : 12u; }
  // where the tile table and the triangles begin in a payload of nv vertices and `rows` table rows (the uint32 format has no table: rows is not read)
  uint64_t table_offset(uint64_t nv) const { return format == kMeshIndexTile16 ? align16(nv * stride) : nv * stride; }
  uint64_t triangle_offset(uint64_t nv, uint64_t rows) const { return table_offset(nv) + (format == kMeshIndexTile16 ? rows * kMeshTileRowBytes : 0u); }
  // the bytes of a frame that are copied: exactly its counts', never a capacity's.  A frame without a vertex has no triangle and no row: nothing.
  uint64_t payload_bytes(uint64_t nv, uint64_t nt, uint64_t rows) const { return nv ? triangle_offset(nv, rows) + nt * triangle_bytes() : 0u; }
  uint64_t payload_capacity(uint64_t max_vertices, uint64_t max_triangles, uint64_t max_tiles) const { return triangle_offset(max_vertices, max_tiles) + max_triangles * triangle_bytes(); }
  uint64_t slot_bytes(uint64_t max_vertices, uint64_t max_triangles, uint64_t max_tiles) const { return kMeshHeaderBytes + payload_capacity(max_vertices, max_triangles, max_tiles); }
  // the 4 GiB bound of a configuration: on the payload in the uint32 format (as it always was), on the whole slot, header included, in the tile-local one
  // (every capacity is below 2^32 and every factor at most 16: no sum here comes near 2^64)
  bool fits(uint64_t max_vertices, uint64_t max_triangles, uint64_t max_tiles) const {
    return (format == kMeshIndexTile16 ? slot_bytes(max_vertices, max_triangles, max_tiles) : payload_capacity(max_vertices, max_triangles, max_tiles)) <= kMeshSlotLimit;
  }
  // "mesh streaming: texture taps in the frame": a block of packed taps (kMeshTapBytes per vertex and stream, [vertex][stream]) at a fixed place behind
  // the payload's CAPACITY, so that the payload keeps its layout and its one exact-size copy; the block travels in a copy of its own, of a frame's bytes.
  // tap_offset counts from the payload's first byte, as table_offset and triangle_offset do.  (streams <= 16: no product here comes near 2^64)
  uint64_t tap_offset(uint64_t max_vertices, uint64_t max_triangles, uint64_t max_tiles) const { return align16(payload_capacity(max_vertices, max_triangles, max_tiles)); }
  static uint64_t tap_capacity(uint64_t max_vertices, uint64_t streams) { return max_vertices * streams * kMeshTapBytes; }
  static uint64_t tap_bytes(uint64_t nv, uint64_t streams) { return nv * streams * kMeshTapBytes; }
  uint64_t slot_bytes_taps(uint64_t max_vertices, uint64_t max_triangles, uint64_t max_tiles, uint64_t streams) const {
    return kMeshHeaderBytes + tap_offset(max_vertices, max_triangles, max_tiles) + tap_capacity(max_vertices, streams);
  }
  // the 4 GiB bound with the block: what fits() asks, and the whole slot -- header, payload capacity, padding, block -- in either format
  bool fits_taps(uint64_t max_vertices, uint64_t max_triangles, uint64_t max_tiles, uint64_t streams) const {
    return fits(max_vertices, max_triangles, max_tiles) && slot_bytes_taps(max_vertices, max_triangles, max_tiles, streams) <= kMeshSlotLimit;
  }
};

// A Z-slab's part of the tile-local frame ("mesh streaming: slab parts"): which lattice tile layers of a level a context owns, and what the part ring holds
// beyond a whole-volume ring.  own_tz0 / own_tz1: the owned storage tile layers (8 voxel planes each), storage_ntz those of the whole volume, lattice_ntz
// the level's lattice tile layers.  A slab reaching the volume's top owns the lattice's last layer whatever its height; below the top both faces must lie on
// the level's lattice tiles (1 << level storage layers each).
struct MeshPartLayers {
  int layer0, layer1; bool top, aligned;
  static MeshPartLayers of(int own_tz0, int own_tz1, int storage_ntz, int level, int lattice_ntz) {
    const int stride = 1 << level;
    const bool top = own_tz1 == storage_ntz;
    return MeshPartLayers{own_tz0 >> level, top ? lattice_ntz : (own_tz1 >> level), top, own_tz0 % stride == 0 && (top || own_tz1 % stride == 0)};
  }
  // the seam layer: the tiles of the first layer above the owned ones, whose plane-0 records the part's top cells read (none at the top)
  uint64_t seam_tiles(uint64_t tiles_per_layer) const { return top ? 0u : tiles_per_layer; }
  // record slots: the owned surface tiles the capacity bounds, and every seam tile -- a seam tile never causes an overflow, there is no fourth capacity
  uint64_t record_slots(uint64_t max_tiles, uint64_t tiles_per_layer) const { return max_tiles + seam_tiles(tiles_per_layer); }
};
constexpr uint64_t kMeshPartRecordBytes = 64;                           // MeshStreamPartRecord, in front of a part frame's header

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
