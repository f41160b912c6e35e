// Headless harness: one frame in the reference's call order (source/kinect_client.cpp:569-599,614) through the C++
// adapter, on a hand-made single-stream scene (constant inverse LUT, constant images).  Exit codes: 0 ok,
// 3 no HIP device (the path has no CPU fallback), 1 any other failure.
// Option --draw-bricks: setDrawBricks(true) before the draw, so that drawF() ends with the occupied-brick wireframes; the number of
// pure red (1, 0, 0, 1) pixels is printed and must not be zero.
// Option --sensor-view TYPE WIDTH: after the frame, one "Show textures" window per sensor (SensorTextureViewHip; TYPE 0 Color, 1 Depth,
// 2 Quality, 4 Silhouette for this pre-processed frame), WIDTH wide, side by side from the top left; the number of pixels it changed is
// printed and must not be zero.
// Option --present rgba8|dxt1: five more draws of the frame, each followed by the swap (present, source/kinect_client.cpp:533), the presented frames
// picked up two frames late and the last two after the loop; tags must come back in order, every frame must have the format's size, and the RGBA8
// frames must equal the framebuffer download converted on the host (the frame is the same each time).
// Option --mesh FILE.ply: after the last frame, the fused surface is extracted as a triangle mesh with normals and colours (extractMesh) and written to
// FILE.ply; the counts are printed and the downloaded arrays must have their sizes.  (This scene's TSDF is positive everywhere: the mesh is empty, the file
// a header.)
// Option --mesh-stream: five more draws of the frame, each followed by streamMesh (packed vertices with normals and colours into a 3-slot ring), the
// frames picked up two frames late and the last two after the loop; tags must come back in order, no frame may overflow, and every frame's counts
// must equal those of extractMesh on the same volume (zero for this scene).
// Option --mesh-level N (0, 1, 2), applied to --mesh and --mesh-stream: the mesh at that level of detail (the lattice of every 2^N-th voxel) through the
// adapter's overloads with a level; the streamed frames' counts must equal those of the extract at the same level, and the ring must report the level.
// Option --mesh-stream-compact (implies --mesh-stream): the ring streams 6-byte tile-local triangles (TSDF_MESH_INDEX_TILE16); every frame's uint32
// pointer must be null, its codes decoded on the host (decodeMeshTriangles) must equal downloadMesh's triangles of the same extract, and the payload
// bytes must be the compact sizes.
// Option --mesh-stream-part (implies --mesh-stream-compact; no filter): the ring is configured with configureMeshStreamPart, so every frame is the
// context's part of the tile-local frame -- on this whole-volume context the one-slab case: the part must reach the top, own every lattice tile layer
// and have no seam tile, and the join of that one part (joinMeshParts) must decode to downloadMesh's triangles.
// Option --mesh-stream-taps (implies --mesh-stream; with any of the switches above): meshStreamConfigTaps after the configuration, so every frame
// carries its packed texture taps; the ring must report the flag, every held frame's block must be non-null with the frame's vertex count, one stream
// and 8-byte records, decodeMeshTaps must give a record per pair, and the payload bytes must count the blocks.
//   g++ -std=c++17 frame_harness.cpp -o frame_harness -L.. -lrgbd_recon_hip -Wl,-rpath,'$ORIGIN/..'
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "recon_integration_hip.hpp"

int main(int argc, char** argv) {
  bool draw_bricks = false;
  int view_type = -1;
  float view_width = 0.0f;
  int present_format = -1;
  const char* mesh_path = nullptr;
  bool mesh_stream = false;
  int mesh_level = -1;                                                    // -1: not given (the entries without a level)
  long mesh_stream_min_triangles = -1;                                    // -1: not given (the ring without a filter)
  bool mesh_stream_compact = false, mesh_stream_part = false, mesh_stream_taps = false;
  for (int a = 1; a < argc; ++a) {
    if (std::strcmp(argv[a], "--draw-bricks") == 0) draw_bricks = true;
    else if (std::strcmp(argv[a], "--sensor-view") == 0 && a + 2 < argc) { view_type = std::atoi(argv[a + 1]); view_width = (float)std::atof(argv[a + 2]); a += 2; }
    else if (std::strcmp(argv[a], "--present") == 0 && a + 1 < argc && (std::strcmp(argv[a + 1], "rgba8") == 0 || std::strcmp(argv[a + 1], "dxt1") == 0)) {
      present_format = std::strcmp(argv[a + 1], "dxt1") == 0 ? (int)TSDF_PRESENT_DXT1 : (int)TSDF_PRESENT_RGBA8; a += 1;
    }
    else if (std::strcmp(argv[a], "--mesh") == 0 && a + 1 < argc) { mesh_path = argv[a + 1]; a += 1; }
    else if (std::strcmp(argv[a], "--mesh-stream") == 0) mesh_stream = true;
    else if (std::strcmp(argv[a], "--mesh-level") == 0 && a + 1 < argc && std::strlen(argv[a + 1]) == 1 && argv[a + 1][0] >= '0' && argv[a + 1][0] <= '2') { mesh_level = argv[a + 1][0] - '0'; a += 1; }
    else if (std::strcmp(argv[a], "--mesh-stream-min-triangles") == 0 && a + 1 < argc && argv[a + 1][0] >= '0' && argv[a + 1][0] <= '9') {
      mesh_stream_min_triangles = std::atol(argv[a + 1]); mesh_stream = true; a += 1;
    }
    else if (std::strcmp(argv[a], "--mesh-stream-compact") == 0) { mesh_stream_compact = true; mesh_stream = true; }
    else if (std::strcmp(argv[a], "--mesh-stream-part") == 0) { mesh_stream_part = true; mesh_stream_compact = true; mesh_stream = true; }
    else if (std::strcmp(argv[a], "--mesh-stream-taps") == 0) { mesh_stream_taps = true; mesh_stream = true; }
    else {
      std::fprintf(stderr, "usage: frame_harness [--draw-bricks] [--sensor-view TYPE WIDTH] [--present rgba8|dxt1] [--mesh FILE.ply] [--mesh-stream] [--mesh-level 0|1|2]"
                           " [--mesh-stream-min-triangles N] [--mesh-stream-compact] [--mesh-stream-part] [--mesh-stream-taps]\n");
      return 1;
    }
  }
  if (mesh_stream_part && mesh_stream_min_triangles >= 0) { std::fprintf(stderr, "--mesh-stream-part has no filter\n"); return 1; }
  kinect::ReconInputs in;
  in.num_kinects = 1;
  in.depth_width = in.color_width = 8;
  in.depth_height = in.color_height = 8;
  in.bbox_min = {{0.0f, 0.0f, 0.0f}};
  in.bbox_max = {{1.0f, 1.0f, 1.0f}};
  in.explicit_res = {{16, 16, 16}};
  try {
    kinect::ReconIntegrationHip recon(in, /*limit*/ 0.05f, /*voxel*/ 0.0625f, /*brick*/ 0.5f, 32, 32);
    // every voxel projects to (u, v, z) = (0.5, 0.5, 0.52); the depth image says 0.5 -> sdist 0.02 everywhere
    const uint32_t r2[3] = {2, 2, 2};
    std::vector<float> inv(8 * 4), uv(8 * 2), xyz(8 * 3);
    for (int i = 0; i < 8; ++i) {
      inv[4 * i] = 0.5f; inv[4 * i + 1] = 0.5f; inv[4 * i + 2] = 0.52f; inv[4 * i + 3] = 1.0f;
      uv[2 * i] = 0.5f; uv[2 * i + 1] = 0.5f;
      xyz[3 * i] = 0.25f + 0.5f * (i & 1); xyz[3 * i + 1] = 0.25f + 0.5f * ((i >> 1) & 1); xyz[3 * i + 2] = 0.25f + 0.5f * (i >> 2);
    }
    recon.setCalibration(0, inv.data(), r2, uv.data(), r2, xyz.data(), r2);
    std::vector<float> depth(64 * 2, 0.0f), q(64, 1.0f), s(64, 1.0f);
    for (int i = 0; i < 64; ++i) depth[2 * i] = 0.5f;
    std::vector<uint8_t> col(64 * 3, 200);
    recon.uploadFrame(depth.data(), q.data(), s.data(), col.data());
    recon.setMinVoxelsPerBrick(1);
    recon.clearOccupiedBricks();
    recon.markBricks();
    recon.updateOccupiedBricks();
    recon.integrate();
    const float mv[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, -0.5f, -0.5f, -3.0f, 1};
    const float f = 1.0f / std::tan(0.5f * 0.6f), n = 0.1f, fa = 50.0f;
    const float pr[16] = {f, 0, 0, 0, 0, f, 0, 0, 0, 0, (fa + n) / (n - fa), -1, 0, 0, 2 * fa * n / (n - fa), 0};
    recon.setMatrices(mv, pr);
    recon.setDrawBricks(draw_bricks);
    recon.drawF();
    std::vector<float> tsdf, rgba, d;
    recon.downloadVolume(tsdf);
    recon.downloadFramebuffer(rgba, d, 32, 32);
    int band = 0;
    for (float v : tsdf) band += std::fabs(v - 0.02f) < 1e-6f;
    std::printf("occupied ratio %.4f, %u bricks, %d of %zu voxels at sdist 0.02\n", recon.occupiedRatio(), recon.numBricks(), band, tsdf.size());
    if (draw_bricks) {
      int wire = 0;
      for (std::size_t i = 0; i < d.size(); ++i) wire += rgba[4 * i] == 1.0f && rgba[4 * i + 1] == 0.0f && rgba[4 * i + 2] == 0.0f && rgba[4 * i + 3] == 1.0f;
      std::printf("%d wireframe pixels\n", wire);
      if (wire == 0) return 1;
    }
    if (view_type >= 0) {
      kinect::NetKinectArrayHip nka(recon, TSDF_COLOR_RGB8, false);
      nka.setStartTextureUnit(1);                                         // (any: the view subtracts it again)
      kinect::SensorTextureViewHip view(nka);
      struct { std::uint16_t unit; std::int16_t layer; } info;            // the reference's TexInfo
      const std::array<float, 2> size = view.imageSize(view_width);
      for (unsigned i = 0; i < in.num_kinects; ++i) {
        info.unit = (std::uint16_t)(nka.getStartTextureUnit() + (unsigned)view_type); info.layer = (std::int16_t)(-(int)i - 1);
        const float p_min[2] = {1.0f + (float)i * (size[0] + 2.0f), 1.0f}, p_max[2] = {p_min[0] + size[0], p_min[1] + size[1]};
        view.draw(info, p_min, p_max);
      }
      std::vector<float> rgba2, d2;
      recon.downloadFramebuffer(rgba2, d2, 32, 32);
      int changed = 0;
      for (std::size_t i = 0; i < d.size(); ++i) changed += std::memcmp(&rgba[4 * i], &rgba2[4 * i], 16) != 0;
      std::printf("%d pixels changed by the sensor windows (%g x %g)\n", changed, size[0], size[1]);
      if (changed == 0 || d2 != d) return 1;
    }
    if (present_format >= 0) {
      recon.configurePresent((unsigned)present_format, TSDF_PRESENT_TOP_DOWN, 3);
      recon.downloadFramebuffer(rgba, d, 32, 32);
      const std::uint64_t want_bytes = present_format == (int)TSDF_PRESENT_DXT1 ? 8u * 8u * 8u : 32u * 32u * 4u;
      const int frames = 5, lag = 2;
      int got = 0, wrong = 0;
      auto take = [&](std::uint64_t want_tag) {
        kinect::ReconIntegrationHip::PresentedFrame fr;
        if (!recon.acquirePresented(fr) || fr.tag != want_tag || fr.bytes != want_bytes || fr.width != 32 || fr.height != 32) { ++wrong; return; }
        if (present_format == (int)TSDF_PRESENT_RGBA8) {
          const std::uint8_t* px = (const std::uint8_t*)fr.data;
          for (int j = 0; j < 32; ++j) for (int i = 0; i < 32 * 4; ++i) {
            const float v = rgba[(std::size_t)(31 - j) * 128 + i];                                     // top-down: output row j is window row h - 1 - j
            const float cl = std::isnan(v) ? 0.0f : std::fmin(std::fmax(v, 0.0f), 1.0f);
            wrong += px[j * 128 + i] != (std::uint8_t)std::nearbyint(cl * 255.0f);
          }
        }
        recon.releasePresented();
        ++got;
      };
      for (int f = 0; f < frames; ++f) {
        recon.drawF();
        if (!recon.present((std::uint64_t)(100 + f))) ++wrong;
        if (f >= lag) take((std::uint64_t)(100 + f - lag));
      }
      for (int f = frames - lag; f < frames; ++f) take((std::uint64_t)(100 + f));
      std::printf("%d frames presented as %s, %d picked up in order, %d mismatches\n", frames, present_format ? "dxt1" : "rgba8", got, wrong);
      if (got != frames || wrong != 0) return 1;
    }
    if (mesh_path) {
      const kinect::ReconIntegrationHip::MeshCounts n = mesh_level < 0 ? recon.extractMesh(true, true) : recon.extractMesh(true, true, (unsigned)mesh_level);
      kinect::ReconIntegrationHip::Mesh mesh;
      recon.downloadMesh(mesh);
      recon.writeMeshPly(mesh_path);
      std::printf("mesh: %llu vertices, %llu triangles -> %s\n", (unsigned long long)n.vertices, (unsigned long long)n.triangles, mesh_path);
      if (mesh.position.size() != n.vertices * 3 || mesh.normal.size() != n.vertices * 3 || mesh.colour.size() != n.vertices * 4 || mesh.triangles.size() != n.triangles * 3) return 1;
    }
    if (mesh_stream) {
      const kinect::ReconIntegrationHip::MeshCounts whole = mesh_level < 0 ? recon.extractMesh(false, false) : recon.extractMesh(false, false, (unsigned)mesh_level);
      kinect::ReconIntegrationHip::MeshCounts n = whole;
      const bool filtered = mesh_stream_min_triangles >= 0;
      std::uint64_t components = 0;
      if (mesh_stream_min_triangles >= 1) {                                    // what the ring has to deliver: the one-shot filter's result
        components = recon.meshComponents();
        n = recon.filterMeshComponents((std::uint32_t)mesh_stream_min_triangles);
      }
      kinect::ReconIntegrationHip::Mesh want;                                  // the triangles the decoded codes have to equal
      if (mesh_stream_compact) recon.downloadMesh(want);
      std::uint64_t want_bytes = 0;
      if (mesh_stream_part) recon.configureMeshStreamPart(true, true, (unsigned)(mesh_level < 0 ? 0 : mesh_level), 4096, 8192, 64, 3);
      else if (mesh_stream_compact) recon.configureMeshStream(true, true, (unsigned)(mesh_level < 0 ? 0 : mesh_level), (unsigned)(filtered ? mesh_stream_min_triangles : 0),
                                                         TSDF_MESH_INDEX_TILE16, 4096, 8192, 64, 3);
      else if (filtered) recon.configureMeshStream(true, true, (unsigned)(mesh_level < 0 ? 0 : mesh_level), (unsigned)mesh_stream_min_triangles, 4096, 8192, 64, 3);
      else if (mesh_level < 0) recon.configureMeshStream(true, true, 4096, 8192, 64, 3);
      else recon.configureMeshStream(true, true, (unsigned)mesh_level, 4096, 8192, 64, 3);
      if (recon.meshStreamLevel() != (unsigned)(mesh_level < 0 ? 0 : mesh_level)) return 1;
      if (recon.meshStreamMinTriangles() != (unsigned)(filtered ? mesh_stream_min_triangles : 0)) return 1;
      if (recon.meshStreamIndexFormat() != (mesh_stream_compact ? TSDF_MESH_INDEX_TILE16 : TSDF_MESH_INDEX_U32)) return 1;
      if (recon.meshStreamHasTaps()) return 1;                                 // (every config entry leaves the taps off)
      if (mesh_stream_taps) recon.meshStreamConfigTaps();
      if (recon.meshStreamHasTaps() != mesh_stream_taps) return 1;
      const int frames = 5, lag = 2;
      int got = 0, wrong = 0;
      auto take = [&](std::uint64_t want_tag) {
        tsdf_mesh_frame fr;
        if (!recon.acquireMeshFrame(fr)) { ++wrong; return; }
        bool ok = fr.tag == want_tag && fr.overflow == 0 && fr.vertex_stride == 16 && fr.n_vertices == n.vertices && fr.n_triangles == n.triangles &&
                  fr.needed_vertices == whole.vertices && fr.res[0] == 16;
        if (mesh_stream_min_triangles >= 1) {
          const kinect::ReconIntegrationHip::MeshFrameFilter ff = recon.meshStreamFrameFilter();
          ok = ok && ff.components == components && ff.vertices_removed == whole.vertices - n.vertices && ff.triangles_removed == whole.triangles - n.triangles;
        }
        if (mesh_stream_compact) {
          const tsdf_mesh_compact c = recon.meshFrameCompact();
          ok = ok && fr.triangles == nullptr && kinect::ReconIntegrationHip::decodeMeshTriangles(c, fr.n_triangles) == want.triangles;
          want_bytes += fr.n_vertices ? (fr.n_vertices * 16 + 15) / 16 * 16 + c.n_tile_rows * 16 + fr.n_triangles * 6 : 0;
          if (mesh_stream_part) {
            const tsdf_mesh_part part = recon.meshFramePart();
            ok = ok && part.top == 1 && part.layers[0] == 0 && part.layers[1] == c.tiles[2] && part.seam_tiles == 0 && part.level == c.level;
            kinect::ReconIntegrationHip::MeshPartFrame joined;
            ok = ok && kinect::ReconIntegrationHip::joinMeshParts({recon.takeMeshPart(fr)}, joined) && joined.nVertices() == fr.n_vertices &&
                 kinect::ReconIntegrationHip::decodeMeshTriangles(joined.compact(), joined.nTriangles()) == want.triangles;
          }
        } else want_bytes += fr.n_vertices * 16 + fr.n_triangles * 12;
        if (mesh_stream_taps) {
          const tsdf_mesh_taps t = recon.meshStreamFrameTaps();
          ok = ok && t.taps != nullptr && t.n_vertices == fr.n_vertices && t.n_streams == 1 && t.tap_bytes == sizeof(tsdf_packed_tap) &&
               kinect::ReconIntegrationHip::decodeMeshTaps(t).size() == t.n_vertices * t.n_streams;
          want_bytes += t.n_vertices * t.n_streams * sizeof(tsdf_packed_tap);
        }
        recon.releaseMeshFrame();                                              // (before it is counted: a held frame would fail every later acquire too)
        ++(ok ? got : wrong);
      };
      for (int f = 0; f < frames; ++f) {
        recon.drawF();
        if (!recon.streamMesh((std::uint64_t)(200 + f))) ++wrong;
        if (f >= lag) take((std::uint64_t)(200 + f - lag));
      }
      for (int f = frames - lag; f < frames; ++f) take((std::uint64_t)(200 + f));
      const kinect::ReconIntegrationHip::MeshStreamStats st = recon.meshStreamStats();
      std::printf("%d mesh frames streamed, %d picked up in order, %d mismatches, %llu payload bytes\n", frames, got, wrong, (unsigned long long)st.payload_bytes);
      if (got != frames || wrong != 0 || st.frames != (std::uint64_t)frames || st.payload_bytes != want_bytes) return 1;
    }
    return band > 0 ? 0 : 1;
  } catch (std::exception const& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return std::string(e.what()).find("no HIP device") != std::string::npos ? 3 : 1;
  }
}
