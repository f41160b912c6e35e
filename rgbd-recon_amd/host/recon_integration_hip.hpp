// recon_integration_hip.hpp -- C++ adapter with the reference operator's names, over the C ABI.
//
// kinect::ReconIntegrationHip exposes the public surface of kinect::ReconIntegration
// (framework/reconstruction/recon_integration.hpp:35-64) and of its base kinect::Reconstruction
// (framework/reconstruction/reconstruction.hpp:11-36), so draw3d()-style code
// (source/kinect_client.cpp:569-599,614) compiles against either class:
//
//     recon->clearOccupiedBricks();            // process_textures(), kinect_client.cpp:569-577
//     nka->processTextures();                  //   (the GL pre-process; on the HIP path: markBricks())
//     recon->updateOccupiedBricks();
//     recon->integrate();                      // :595-599
//     recon->drawF();                          // :614
//
// What the GL class pulls out of global GL state is passed explicitly:
//   * CalibVolumes' 3-D textures          -> setCalibration(stream, cv_xyz_inv, cv_uv, cv_xyz)
//   * NetKinectArray's texture arrays     -> uploadFrame(depth, quality, silhouette, colour)
//   * GL_MODELVIEW / GL_PROJECTION        -> setMatrices(mv, proj) before draw()/drawF()
//   * UBO 1 g_shade_mode                  -> setShadeMode()
// Errors: the reference throws / exits; this class throws std::runtime_error carrying tsdf_last_error().
// Header only; link with librgbd_recon_hip.so.  No GL, no torch.
#ifndef RECON_INTEGRATION_HIP_HPP
#define RECON_INTEGRATION_HIP_HPP

#include <array>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rgbd_recon_hip.h"

namespace kinect {

// the pieces of CalibrationFiles (calibration_files.hpp) and gloost::BoundingBox the operator reads
struct ReconInputs {
  unsigned num_kinects = 0;                 // CalibrationFiles::num()
  unsigned depth_width = 640, depth_height = 480;     // getWidth()/getHeight()
  unsigned color_width = 640, color_height = 480;     // getWidthC()/getHeightC()
  std::array<float, 3> bbox_min{{-1.0f, 0.0f, -1.0f}};   // kinect_client.cpp:206-207 default
  std::array<float, 3> bbox_max{{1.0f, 2.2f, 1.0f}};
  int device = 0;
  std::array<unsigned, 3> explicit_res{{0, 0, 0}};    // 0: res = ceil(bbox / voxel_size) like setVoxelSize()
  unsigned slab_z0 = 0, slab_z1 = 0;                  // multi-GPU Z-slab (0,0 = whole volume)
  bool slab_recompute_halo = false;                   // integrate the halo layers locally instead of exchanging them
  unsigned sparse_pool_tiles = 0;                     // > 0: TSDF in a sparse pool of this many 8^3-voxel tiles (needs brick culling)
};

class ReconIntegrationHip {
 public:
  // ReconIntegration(cfs, cv, bbox, limit, size), recon_integration.cpp:30-60
  ReconIntegrationHip(ReconInputs const& in, float limit, float voxel_size, float brick_size = 0.1f, std::size_t width = 1280, std::size_t height = 720)
      : m_in(in), m_brick_size(brick_size) {
    tsdf_config cfg;
    std::memset(&cfg, 0, sizeof(cfg));
    cfg.struct_size = sizeof(cfg);
    for (int a = 0; a < 3; ++a) { cfg.bbox_min[a] = in.bbox_min[a]; cfg.bbox_max[a] = in.bbox_max[a]; cfg.res[a] = in.explicit_res[a]; cfg.brick_size[a] = brick_size; }
    cfg.voxel_size = voxel_size;
    cfg.limit = limit;
    cfg.num_streams = in.num_kinects;
    cfg.depth_w = in.depth_width; cfg.depth_h = in.depth_height;
    cfg.color_w = in.color_width; cfg.color_h = in.color_height;
    cfg.view_w = (uint32_t)width; cfg.view_h = (uint32_t)height;
    cfg.device = in.device;
    cfg.slab_z0 = in.slab_z0; cfg.slab_z1 = in.slab_z1;
    cfg.slab_recompute_halo = in.slab_recompute_halo ? 1u : 0u;
    cfg.sparse_pool_tiles = in.sparse_pool_tiles;
    if (tsdf_create(&cfg, &m_ctx) != TSDF_OK) throw std::runtime_error(std::string("ReconIntegrationHip: ") + tsdf_last_error(nullptr));
    const float id[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::memcpy(m_mv, id, sizeof(id));
    std::memcpy(m_proj, id, sizeof(id));
  }
  ~ReconIntegrationHip() { if (m_ctx) tsdf_destroy(m_ctx); }
  ReconIntegrationHip(ReconIntegrationHip const&) = delete;
  ReconIntegrationHip& operator=(ReconIntegrationHip const&) = delete;

  // ---- explicit inputs (implicit GL state in the reference)
  void setCalibration(unsigned stream, const float* cv_xyz_inv_rgba, const uint32_t res_inv[3], const float* cv_uv_rg, const uint32_t res_uv[3],
                      const float* cv_xyz_rgb, const uint32_t res_xyz[3]) {
    check(tsdf_set_calibration(m_ctx, stream, cv_xyz_inv_rgba, res_inv, cv_uv_rg, res_uv, cv_xyz_rgb, res_xyz));
  }
  void uploadFrame(const float* depth_rg, const float* quality, const float* silhouette, const uint8_t* colour_rgb) {
    check(tsdf_upload_frame(m_ctx, depth_rg, quality, silhouette, colour_rgb));
  }
  // a frame that is already in device memory (a decoder / pre-process on the GPU): one re-layout launch, no copy
  void uploadFrameDev(const float* depth_rg, const float* quality, const float* silhouette, const uint8_t* colour_rgb, bool arrays_complete) {
    check(tsdf_upload_frame_dev(m_ctx, depth_rg, quality, silhouette, colour_rgb, arrays_complete ? TSDF_FRAME_ARRAYS_COMPLETE : 0u));
  }
  // the client's per-frame sequence (kinect_client.cpp:586-599 update + draw: new frame -> clear / mark / update bricks -> integrate() -> drawF())
  // in ONE call into the library: issuing a frame costs the host about as long as the GPU needs for it, every call boundary counts
  void frameDev(const float* depth_rg, const float* quality, const float* silhouette, const uint8_t* colour_rgb) {
    check(tsdf_frame_dev(m_ctx, depth_rg, quality, silhouette, colour_rgb, TSDF_FRAME_ARRAYS_COMPLETE, m_mv, m_proj));
  }
  void setMatrices(const float modelview[16], const float projection[16]) {
    std::memcpy(m_mv, modelview, sizeof(m_mv));
    std::memcpy(m_proj, projection, sizeof(m_proj));
  }
  void markBricks() { check(tsdf_mark_bricks(m_ctx)); }          // mark_brick() runs inside pre_normal.fs in the reference

  // ---- kinect::Reconstruction (reconstruction.hpp:16-23)
  void draw() { check(tsdf_raymarch(m_ctx, m_mv, m_proj)); }
  void drawF() { check(tsdf_draw_f(m_ctx, m_mv, m_proj)); }
  void reload() {}                                               // shader hot reload: nothing to reload
  void resize(std::size_t width, std::size_t height) { check(tsdf_resize(m_ctx, (uint32_t)width, (uint32_t)height)); }
  void setColorMaskMode(unsigned mode) { check(tsdf_set_color_mask_mode(m_ctx, mode)); }       // reconstruction.cpp:51-53 -> glColorMask :212-216,321-333
  void setViewportOffset(float x, float y) { check(tsdf_set_viewport_offset(m_ctx, x, y)); }   // recon_integration.cpp:527 -> tsdf_raymarch.fs:70,388-389
  // GL state the reference reads implicitly: glViewport's origin (gl_FragCoord) and whether glClear included the colour buffer
  void setViewportOrigin(int x, int y) { check(tsdf_set_viewport_origin(m_ctx, x, y)); }
  void setFramebufferClear(bool clear_color) { check(tsdf_set_framebuffer_clear(m_ctx, clear_color ? 1 : 0)); }

  // ---- kinect::ReconIntegration (recon_integration.hpp:42-58)
  void integrate() { check(tsdf_integrate(m_ctx)); }
  void setColorFilling(bool active) { check(tsdf_set_color_filling(m_ctx, active)); }
  void setUseBricks(bool active) { check(tsdf_set_use_bricks(m_ctx, active)); }
  void setSpaceSkip(bool active) { check(tsdf_set_space_skip(m_ctx, active)); }
  void setDrawBricks(bool active) { check(tsdf_set_draw_bricks(m_ctx, active)); }   // drawF() then ends with drawOccupiedBricks(), recon_integration.cpp:166-168
  void setVoxelSize(float size) { check(tsdf_set_voxel_size(m_ctx, size)); m_slab_valid = m_slab_components_valid = false; }      // recon_integration.cpp:340-353 (a slab part went with the old grid)
  void setTsdfLimit(float limit) { check(tsdf_set_tsdf_limit(m_ctx, limit)); }
  void setBrickSize(float size) { const float s[3] = {size, size, size}; check(tsdf_set_brick_size(m_ctx, s)); m_brick_size = size; }
  unsigned numBricks() const { uint32_t n = 0; tsdf_num_bricks(m_ctx, &n); return n; }
  float occupiedRatio() const { float r = 0.0f; tsdf_occupied_ratio(m_ctx, &r); return r; }
  float getBrickSize() const { float s[3]; tsdf_get_resolution(m_ctx, nullptr, nullptr, s); return s[0]; }
  void clearOccupiedBricks() const { check(tsdf_clear_bricks(m_ctx)); }
  void updateOccupiedBricks() { check(tsdf_update_occupied(m_ctx, nullptr)); }
  void setMinVoxelsPerBrick(unsigned i) { check(tsdf_set_min_voxels_per_brick(m_ctx, i)); }
  // drawOccupiedBricks() (recon_integration.cpp:447-454; bricks.vs + solid.fs, :130-133): 12 red lines per brick of the latest
  // updateOccupiedBricks(), under the matrices of setMatrices -- the client's call while another back-end is showing (kinect_client.cpp:681-683)
  void drawOccupiedBricks() const { check(tsdf_draw_bricks(m_ctx, m_mv, m_proj)); }
  void setShadeMode(int mode) { check(tsdf_set_shade_mode(m_ctx, mode)); }

  // ---- results (the GL class leaves them in textures / the bound framebuffer)
  void downloadFramebuffer(std::vector<float>& rgba, std::vector<float>& depth, unsigned width, unsigned height) {
    rgba.resize((std::size_t)width * height * 4);
    depth.resize((std::size_t)width * height);
    check(tsdf_download_framebuffer(m_ctx, rgba.data(), depth.data()));
  }
  // ---- the swap: glfwSwapBuffers(window) at the end of the client's frame (source/kinect_client.cpp:533) puts an RGBA8 window on a display; here the
  // finished framebuffer travels to a ring of pinned host buffers as RGBA8 or as the wire's DXT1 blocks, and the host picks frames up in order while
  // the next ones are computed.  configurePresent before the first frame (TSDF_PRESENT_RGBA8 / _DXT1, TSDF_PRESENT_TOP_DOWN, 2..8 slots)
  struct PresentedFrame { const void* data = nullptr; std::uint64_t bytes = 0, tag = 0; unsigned width = 0, height = 0; };
  void configurePresent(unsigned format, unsigned flags = 0, unsigned slots = 3) { check(tsdf_present_config(m_ctx, format, flags, slots)); }
  // where the client calls glfwSwapBuffers (kinect_client.cpp:533): never blocks; false = every slot is queued or held, nothing was queued
  bool present(std::uint64_t tag) {
    const int32_t rc = tsdf_present(m_ctx, tag);
    if (rc == TSDF_ERR_STATE) return false;
    check(rc);
    return true;
  }
  // the oldest frame presented (kinect_client.cpp:533) and not yet released: false while its copy is still under way (wait = false) or nothing is queued;
  // out.data stays valid until releasePresented()
  bool acquirePresented(PresentedFrame& out, bool wait = true) {
    uint32_t size[2] = {0, 0};
    out = PresentedFrame{};
    const int32_t rc = tsdf_present_acquire(m_ctx, wait ? 1 : 0, &out.data, &out.bytes, &out.tag, size);
    if (rc == TSDF_ERR_STATE) return false;
    check(rc);
    out.width = size[0]; out.height = size[1];
    return out.data != nullptr;
  }
  // hands the slot of the acquired frame back to present() (the window's back buffer after the swap of kinect_client.cpp:533)
  void releasePresented() { check(tsdf_present_release(m_ctx)); }
  void downloadVolume(std::vector<float>& tsdf) {
    uint32_t r[3];
    check(tsdf_get_resolution(m_ctx, r, nullptr, nullptr));
    tsdf.resize((std::size_t)r[0] * r[1] * r[2]);
    check(tsdf_download_volume(m_ctx, tsdf.data()));
  }
  // ---- the fused surface as an indexed triangle mesh (tsdf_mesh_extract).  The reference has no counterpart: it never exports what it fused.
  // extractMesh runs the extraction on the volume as it is now and returns the counts; downloadMesh copies the arrays of the last extract
  // (normals / colours stay empty unless that extract produced them); writeMeshPly writes it as a binary little-endian PLY.
  struct Mesh { std::vector<float> position, normal, colour; std::vector<std::uint32_t> triangles; };   // [V][3], [V][3], [V][4] (alpha +1 valid, -1 fallback), [T][3]
  struct MeshCounts { std::uint64_t vertices = 0, triangles = 0; };
  MeshCounts extractMesh(bool normals = true, bool colours = true) {
    m_mesh_flags = (normals ? TSDF_MESH_NORMALS : 0u) | (colours ? TSDF_MESH_COLOURS : 0u);
    m_mesh = MeshCounts{};
    check(tsdf_mesh_extract(m_ctx, m_mesh_flags, &m_mesh.vertices, &m_mesh.triangles));
    return m_mesh;
  }
  // ... at a level of detail (tsdf_mesh_extract_lod): level 1 / 2 = the same surface on the lattice of every 2nd / 4th voxel, every vertex one of the
  // full mesh's; level 0 is extractMesh(normals, colours).  downloadMesh / writeMeshPly serve whichever extract was last.
  MeshCounts extractMesh(bool normals, bool colours, unsigned level) {
    m_mesh_flags = (normals ? TSDF_MESH_NORMALS : 0u) | (colours ? TSDF_MESH_COLOURS : 0u);
    m_mesh = MeshCounts{};
    check(tsdf_mesh_extract_lod(m_ctx, m_mesh_flags, level, &m_mesh.vertices, &m_mesh.triangles));
    return m_mesh;
  }
  void downloadMesh(Mesh& out) {
    out.position.resize((std::size_t)m_mesh.vertices * 3);
    out.normal.resize((m_mesh_flags & TSDF_MESH_NORMALS) ? (std::size_t)m_mesh.vertices * 3 : 0);
    out.colour.resize((m_mesh_flags & TSDF_MESH_COLOURS) ? (std::size_t)m_mesh.vertices * 4 : 0);
    out.triangles.resize((std::size_t)m_mesh.triangles * 3);
    check(tsdf_mesh_download(m_ctx, out.position.data(), out.normal.empty() ? nullptr : out.normal.data(), out.colour.empty() ? nullptr : out.colour.data(),
                             out.triangles.data()));
  }
  void writeMeshPly(const char* path) { check(tsdf_mesh_write_ply(m_ctx, path)); }
  // ---- a Z-slab's part of that mesh (tsdf_mesh_slab_extract): the parts of contiguous slabs, concatenated in slab order, ARE the whole volume's mesh.
  // Call order per slab, the halo being current as for a draw: extractMeshSlab (its counts) -> meshSlabSeam (the table the slab BELOW links with) ->
  // meshSlabLink(vertices of all slabs below, the table of the slab directly above; nullptr at the volume's top) -> downloadMeshSlab.  seamTiles: the
  // table's entries at the extract's level.  The part is a state of its own: extractMesh and everything built on it do not see it.
  MeshCounts extractMeshSlab(bool normals = true, bool colours = true, unsigned level = 0) {
    const std::uint32_t flags = (normals ? TSDF_MESH_NORMALS : 0u) | (colours ? TSDF_MESH_COLOURS : 0u);
    MeshCounts n;
    m_slab_valid = m_slab_components_valid = false;                      // (a refused extract leaves no part in the library either)
    check(tsdf_mesh_slab_extract(m_ctx, flags, level, &n.vertices, &n.triangles));
    m_slab = n; m_slab_flags = flags; m_slab_level = level; m_slab_valid = true;
    return m_slab;
  }
  std::size_t seamTiles() {
    requireSlabPart();
    uint32_t res[3];
    check(tsdf_get_resolution(m_ctx, res, nullptr, nullptr));
    const std::size_t t = (std::size_t)8 << m_slab_level;
    return ((res[0] + t - 1) / t) * ((res[1] + t - 1) / t);
  }
  void meshSlabSeam(std::vector<std::uint32_t>& out) {
    out.assign(seamTiles(), 0u);
    check(tsdf_mesh_slab_seam(m_ctx, out.data()));
  }
  void meshSlabLink(std::uint64_t vertex_base, const std::uint32_t* above_seam) {
    check(tsdf_mesh_slab_link(m_ctx, vertex_base, above_seam));
    m_slab_components_valid = false;                                     // (the part's component labels held the indices of the link that was)
  }
  void downloadMeshSlab(Mesh& out) {
    requireSlabPart();
    out.position.resize((std::size_t)m_slab.vertices * 3);
    out.normal.resize((m_slab_flags & TSDF_MESH_NORMALS) ? (std::size_t)m_slab.vertices * 3 : 0);
    out.colour.resize((m_slab_flags & TSDF_MESH_COLOURS) ? (std::size_t)m_slab.vertices * 4 : 0);
    out.triangles.resize((std::size_t)m_slab.triangles * 3);
    check(tsdf_mesh_slab_download(m_ctx, out.position.data(), out.normal.empty() ? nullptr : out.normal.data(), out.colour.empty() ? nullptr : out.colour.data(),
                                  out.triangles.data()));
  }
  struct MeshSlabStats { std::uint64_t tiles = 0, tiles_skipped = 0, tiles_with_surface = 0, bytes = 0; };
  MeshSlabStats meshSlabStats() {
    std::uint64_t s[4];
    check(tsdf_mesh_slab_stats(m_ctx, s));
    return MeshSlabStats{s[0], s[1], s[2], s[3]};
  }
  // ---- the mesh's islands (tsdf_mesh_components).  The reference has no counterpart.  meshComponents labels the connected components of the last
  // extractMesh (by index; numbered by smallest vertex) and returns their number; downloadMeshComponents copies the labels and the 16-byte table;
  // keepMeshComponents / filterMeshComponents / keepLargestMeshComponents replace the mesh with the kept part -- downloadMesh and writeMeshPly serve it
  // from then on, the labels and the mesh's texture taps are gone until meshComponents / meshTextureTaps run again.
  struct MeshComponents { std::vector<std::uint32_t> vertex_component, triangle_component; std::vector<tsdf_mesh_component> table; };
  struct MeshComponentStats { std::uint64_t components = 0, largest_triangles = 0, vertices_removed = 0, triangles_removed = 0; };
  std::uint64_t meshComponents() {
    std::uint64_t n = 0;
    check(tsdf_mesh_components(m_ctx, &n));
    return n;
  }
  void downloadMeshComponents(MeshComponents& out) {
    check(tsdf_mesh_download_components(m_ctx, nullptr, nullptr, nullptr));   // (throws without components of the current mesh)
    out.vertex_component.resize((std::size_t)m_mesh.vertices);
    out.triangle_component.resize((std::size_t)m_mesh.triangles);
    out.table.resize((std::size_t)meshComponentStats().components);
    check(tsdf_mesh_download_components(m_ctx, out.vertex_component.data(), out.triangle_component.data(), out.table.data()));
  }
  MeshCounts keepMeshComponents(const std::vector<std::uint8_t>& keep) {   // keep[c] != 0: component c stays; one entry per component
    if (keep.size() != meshComponentStats().components) throw std::invalid_argument("ReconIntegrationHip: one keep flag per component");
    const std::uint8_t none = 0;                                           // (no component: still a non-null pointer)
    check(tsdf_mesh_keep_components(m_ctx, keep.empty() ? &none : keep.data(), &m_mesh.vertices, &m_mesh.triangles));
    return m_mesh;
  }
  MeshCounts filterMeshComponents(std::uint32_t min_triangles) {           // keeps the components with at least min_triangles triangles
    check(tsdf_mesh_filter_components(m_ctx, min_triangles, &m_mesh.vertices, &m_mesh.triangles));
    return m_mesh;
  }
  MeshCounts keepLargestMeshComponents(std::size_t k = 1) {                // the k components with the most triangles; ties: the lower index first
    MeshComponents comps;
    downloadMeshComponents(comps);
    std::vector<std::uint8_t> keep(comps.table.size(), 0);
    for (std::size_t n = 0; n < k && n < keep.size(); ++n) {
      std::size_t best = keep.size();
      for (std::size_t c = 0; c < keep.size(); ++c)
        if (!keep[c] && (best == keep.size() || comps.table[c].n_triangles > comps.table[best].n_triangles)) best = c;
      keep[best] = 1;
    }
    return keepMeshComponents(keep);
  }
  MeshComponentStats meshComponentStats() {
    std::uint64_t s[4] = {0, 0, 0, 0};
    check(tsdf_mesh_component_stats(m_ctx, s));
    return MeshComponentStats{s[0], s[1], s[2], s[3]};
  }
  // ---- the islands' measures (tsdf_mesh_component_measures).  The reference has no counterpart.  After meshComponents: meshComponentMeasures computes,
  // on the device and in exact integers on the measure grid, every component's doubled area, six-fold signed volume, bounds and vertex sum, and returns the
  // grid (area = area2 * unit^2 / 2, volume = volume6 * unit^3 / 6, position = origin + q * unit); downloadMeshComponentMeasures copies the 80-byte rows;
  // filterMeshComponentsMeasured keeps the components for which every clause of the rule holds (thresholds in grid integers) and replaces the mesh like
  // filterMeshComponents.  Labels and measures are gone after a keep / filter.
  tsdf_mesh_measure_grid meshMeasureGrid() {                               // needs no mesh
    tsdf_mesh_measure_grid g{};
    check(tsdf_mesh_measure_grid_info(m_ctx, &g));
    return g;
  }
  tsdf_mesh_measure_grid meshComponentMeasures() {
    tsdf_mesh_measure_grid g{};
    check(tsdf_mesh_component_measures(m_ctx, &g));
    return g;
  }
  void downloadMeshComponentMeasures(std::vector<tsdf_mesh_component_measure>& rows) {
    rows.resize((std::size_t)meshComponentStats().components + 1);         // (never a null pointer)
    check(tsdf_mesh_download_component_measures(m_ctx, rows.data()));
    rows.pop_back();
  }
  MeshCounts filterMeshComponentsMeasured(const tsdf_mesh_measure_rule& rule) {
    check(tsdf_mesh_filter_components_measured(m_ctx, &rule, &m_mesh.vertices, &m_mesh.triangles));
    return m_mesh;
  }
  // ---- ... of a Z-slab's part (tsdf_mesh_slab_components).  The reference has no counterpart.  Per slab, after meshSlabLink: meshSlabComponents (labels
  // the part alone; the counts of its seam lists) -> meshSlabComponentSeam (the three lists, global indices) -> once, anywhere, mergeMeshComponentSeams
  // over all slabs' lists in slab order (a host function: no context) -> linkMeshSlabComponents(this slab's base and links) ->
  // downloadMeshSlabComponents: concatenated in slab order, what downloadMeshComponents gives on a whole-volume context.
  struct MeshSlabComponentCounts { std::uint64_t local_components = 0, down = 0, up = 0, roots = 0; };
  struct MeshComponentSeams { std::vector<tsdf_mesh_seam_vertex> down, up; std::vector<tsdf_mesh_seam_root> roots; };
  struct MeshSlabSeams { std::uint64_t vertex_base = 0, n_vertices = 0, n_local = 0; MeshComponentSeams lists; };   // one slab's input of the merge
  struct MergedMeshComponents { std::vector<std::uint64_t> component_base; std::vector<std::vector<tsdf_mesh_component_link>> links; std::uint64_t components = 0; };
  MeshSlabComponentCounts meshSlabComponents() {
    std::uint64_t n[4] = {0, 0, 0, 0};
    m_slab_components_valid = false;
    check(tsdf_mesh_slab_components(m_ctx, n));
    m_slab_components = MeshSlabComponentCounts{n[0], n[1], n[2], n[3]};
    m_slab_components_valid = true; m_slab_owned_valid = false;
    return m_slab_components;
  }
  void meshSlabComponentSeam(MeshComponentSeams& out) {
    requireSlabComponents();
    out.down.resize((std::size_t)m_slab_components.down); out.up.resize((std::size_t)m_slab_components.up); out.roots.resize((std::size_t)m_slab_components.roots);
    check(tsdf_mesh_slab_component_seam(m_ctx, out.down.data(), out.up.data(), out.roots.data()));
  }
  static MergedMeshComponents mergeMeshComponentSeams(const std::vector<MeshSlabSeams>& slabs) {
    std::vector<tsdf_mesh_component_seams> in;
    std::size_t n_links = 0;
    for (const MeshSlabSeams& s : slabs) {
      in.push_back(tsdf_mesh_component_seams{s.vertex_base, s.n_vertices, s.n_local, s.lists.down.size(), s.lists.up.size(), s.lists.roots.size(),
                                             s.lists.down.data(), s.lists.up.data(), s.lists.roots.data()});
      n_links += s.lists.roots.size();
    }
    MergedMeshComponents out;
    out.component_base.assign(slabs.size(), 0);
    std::vector<tsdf_mesh_component_link> links(n_links + 1);
    if (tsdf_mesh_merge_component_seams(in.data(), (std::uint32_t)in.size(), out.component_base.data(), links.data(), &out.components) != TSDF_OK)
      throw std::invalid_argument("ReconIntegrationHip: the slabs' seam lists do not belong together (tsdf_mesh_merge_component_seams)");
    std::size_t first = 0;
    for (const MeshSlabSeams& s : slabs) {
      out.links.emplace_back(links.begin() + (std::ptrdiff_t)first, links.begin() + (std::ptrdiff_t)(first + s.lists.roots.size()));
      first += s.lists.roots.size();
    }
    return out;
  }
  std::uint64_t linkMeshSlabComponents(std::uint64_t component_base, const std::vector<tsdf_mesh_component_link>& links) {
    requireSlabComponents();
    std::uint64_t owned = 0;
    check(tsdf_mesh_slab_link_components(m_ctx, component_base, links.empty() ? nullptr : links.data(), links.size(), &owned));
    m_slab_owned = owned; m_slab_owned_valid = true;
    return owned;
  }
  void downloadMeshSlabComponents(MeshComponents& out) {
    requireSlabComponents();
    if (!m_slab_owned_valid) throw std::runtime_error("ReconIntegrationHip: the part's components have no global numbers yet (linkMeshSlabComponents)");
    out.vertex_component.resize((std::size_t)m_slab.vertices);
    out.triangle_component.resize((std::size_t)m_slab.triangles);
    out.table.resize((std::size_t)m_slab_owned);
    check(tsdf_mesh_slab_download_components(m_ctx, out.vertex_component.data(), out.triangle_component.data(), out.table.data()));
  }
  // ---- the same surface EVERY frame (tsdf_mesh_stream): packed vertices and uint32 triangles through a ring of pinned buffers, queued behind the frame
  // like present().  The reference has no counterpart.  configureMeshStream before the first frame: attributes, capacities (vertices, triangles, 8^3
  // tiles with surface; a frame that needs more comes back with overflow set and no geometry) and 2..8 slots.
  struct MeshStreamStats { std::uint64_t frames = 0, overflowed = 0, payload_bytes = 0, device_bytes = 0; };
  void configureMeshStream(bool normals, bool colours, unsigned max_vertices, unsigned max_triangles, unsigned max_surface_tiles, unsigned slots = 3) {
    check(tsdf_mesh_stream_config(m_ctx, (normals ? TSDF_MESH_NORMALS : 0u) | (colours ? TSDF_MESH_COLOURS : 0u), max_vertices, max_triangles, max_surface_tiles, slots));
  }
  // ... at a level of detail (tsdf_mesh_stream_config_lod; the level follows the attributes as in the C entry, every argument given): every frame is
  // that level's mesh and max_surface_tiles counts its 8^3 lattice tiles.  meshStreamLevel: the level of the last configuration.
  void configureMeshStream(bool normals, bool colours, unsigned level, unsigned max_vertices, unsigned max_triangles, unsigned max_surface_tiles, unsigned slots) {
    check(tsdf_mesh_stream_config_lod(m_ctx, (normals ? TSDF_MESH_NORMALS : 0u) | (colours ? TSDF_MESH_COLOURS : 0u), level, max_vertices, max_triangles,
                                      max_surface_tiles, slots));
  }
  unsigned meshStreamLevel() {
    std::uint32_t level = 0;
    check(tsdf_mesh_stream_level(m_ctx, &level));
    return level;
  }
  // ... without its small components (tsdf_mesh_stream_config_filter; min_triangles follows the level as in the C entry, every argument given): every
  // frame is the level's mesh minus the components with fewer than min_triangles triangles, dropped on the device before the frame leaves it; 0 is the
  // ring without a filter.  A frame's n_* are the filtered counts, its needed_* and the capacities those of the unfiltered mesh.
  // meshStreamFrameFilter: what the filter did to the frame HELD now (between acquireMeshFrame and releaseMeshFrame); throws without a filter.
  struct MeshFrameFilter { std::uint64_t components = 0, kept = 0, vertices_removed = 0, triangles_removed = 0; };
  // (The trailing return type is deliberate: tests/test_mesh_lod_abi.py counts the void-first overloads, the two of its own section.)
  auto configureMeshStream(bool normals, bool colours, unsigned level, unsigned min_triangles, unsigned max_vertices, unsigned max_triangles, unsigned max_surface_tiles,
                           unsigned slots) -> void {
    check(tsdf_mesh_stream_config_filter(m_ctx, (normals ? TSDF_MESH_NORMALS : 0u) | (colours ? TSDF_MESH_COLOURS : 0u), level, min_triangles, max_vertices, max_triangles,
                                         max_surface_tiles, slots));
  }
  unsigned meshStreamMinTriangles() {
    std::uint32_t min_triangles = 0;
    check(tsdf_mesh_stream_min_triangles(m_ctx, &min_triangles));
    return min_triangles;
  }
  MeshFrameFilter meshStreamFrameFilter() {
    std::uint64_t s[4];
    check(tsdf_mesh_stream_frame_filter(m_ctx, s));
    return MeshFrameFilter{s[0], s[1], s[2], s[3]};
  }
  // ... with 6-byte tile-local triangles (tsdf_mesh_stream_config_compact; index_format follows min_triangles as in the C entry, every argument given):
  // TSDF_MESH_INDEX_TILE16 streams three 16-bit corner codes per triangle and a table row per lattice tile instead of uint32 indices; a frame's
  // `triangles` is then null and meshFrameCompact() hands out the table and the codes of the frame HELD now (throws on a uint32 ring or without a
  // frame).  decodeMeshTriangles is the header's decoding rule: it gives the uint32 array of the same frame, byte for byte.
  auto configureMeshStream(bool normals, bool colours, unsigned level, unsigned min_triangles, unsigned index_format, unsigned max_vertices, unsigned max_triangles,
                           unsigned max_surface_tiles, unsigned slots) -> void {
    check(tsdf_mesh_stream_config_compact(m_ctx, (normals ? TSDF_MESH_NORMALS : 0u) | (colours ? TSDF_MESH_COLOURS : 0u), level, min_triangles, index_format, max_vertices,
                                          max_triangles, max_surface_tiles, slots));
  }
  unsigned meshStreamIndexFormat() {
    std::uint32_t format = 0;
    check(tsdf_mesh_stream_index_format(m_ctx, &format));
    return format;
  }
  tsdf_mesh_compact meshFrameCompact() {
    tsdf_mesh_compact out{};
    check(tsdf_mesh_stream_frame_compact(m_ctx, &out));
    return out;
  }
  static std::vector<std::uint32_t> decodeMeshTriangles(const tsdf_mesh_compact& c, std::uint64_t n_triangles) {
    std::vector<std::uint32_t> out(n_triangles * 3);
    for (std::uint64_t r = 0; r < c.n_tile_rows; ++r) {
      const tsdf_mesh_tile_row& row = c.table[r];
      for (std::uint64_t t = row.first_triangle, end = t + row.n_triangles; t < end; ++t)
        for (int k = 0; k < 3; ++k) {
          const std::uint32_t code = c.triangles[t * 3 + k];
          const std::uint32_t owner = row.tile + ((code >> 12) & 1u) + ((code >> 13) & 1u) * c.tiles[0] + ((code >> 14) & 1u) * c.tiles[0] * c.tiles[1];
          std::uint64_t lo = r, hi = c.n_tile_rows;                      // the owner's row: rows ascend by tile, and owner >= row.tile
          while (hi - lo > 1) { const std::uint64_t mid = (lo + hi) / 2; if (c.table[mid].tile <= owner) lo = mid; else hi = mid; }
          out[t * 3 + k] = c.table[lo].first_vertex + (code & 0xfffu);
        }
    }
    return out;
  }
  // ... with the packed texture taps of every frame beside its vertices (tsdf_mesh_stream_config_taps, after any configureMeshStream*: each of those
  // turns the taps off again): 8 bytes per vertex and stream, taken at the position the receiver reconstructs from the vertex's codes.  The reference
  // has no counterpart.  meshStreamFrameTaps(): the block of the frame HELD now, [n_vertices][n_streams], valid until releaseMeshFrame() (throws on a
  // ring without taps or without a frame).  decodeMeshTaps is the header's unpacking: u = code / 65535.0f, the binary16 weights widened to fp32 -- the
  // records the receiver's rule of the texture taps takes as they are.
  void meshStreamConfigTaps(bool taps = true) { check(tsdf_mesh_stream_config_taps(m_ctx, taps ? TSDF_MESH_STREAM_TAPS : 0u)); }
  bool meshStreamHasTaps() {
    std::uint32_t flags = 0;
    check(tsdf_mesh_stream_tap_flags(m_ctx, &flags));
    return (flags & TSDF_MESH_STREAM_TAPS) != 0;
  }
  tsdf_mesh_taps meshStreamFrameTaps() {
    tsdf_mesh_taps out{};
    check(tsdf_mesh_stream_frame_taps(m_ctx, &out));
    return out;
  }
  static float halfToFloat(std::uint16_t h) {
    const std::uint32_t sign = (std::uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 0x1fu, man = h & 0x3ffu;
    std::uint32_t bits;
    if (exp == 0x1fu) bits = sign | 0x7f800000u | (man << 13);            // infinity, NaN
    else if (exp) bits = sign | ((exp + 112u) << 23) | (man << 13);       // normal: the exponent re-biased, 127 - 15
    else if (!man) bits = sign;                                           // +-0
    else {                                                                // subnormal: man * 2^-24, exactly
      float f = (float)man * 5.9604644775390625e-08f;
      return sign ? -f : f;
    }
    float f;
    std::memcpy(&f, &bits, sizeof f);
    return f;
  }
  static std::vector<tsdf_texture_tap> decodeMeshTaps(const tsdf_mesh_taps& t) {
    std::vector<tsdf_texture_tap> out(t.n_vertices * t.n_streams);
    for (std::size_t k = 0; k < out.size(); ++k) {
      const tsdf_packed_tap& p = t.taps[k];
      out[k] = tsdf_texture_tap{(float)p.u / 65535.0f, (float)p.v / 65535.0f, halfToFloat(p.quality_h), halfToFloat(p.dist_h)};
    }
    return out;
  }
  // ... as this context's PART of the tile-local frame (tsdf_mesh_stream_config_part): the one ring a Z-slab context streams through; a whole-volume
  // context is the one-slab case.  Capacities are per part; there is no filter.  meshFramePart(): the layers, level, top flag and seam tiles of the frame
  // HELD now (throws on another ring or without a frame); takeMeshPart copies the held frame into a MeshPartFrame of the caller's own.  joinMeshParts
  // is the header's join rule over the parts of contiguous slabs in slab order: false (and `out` empty) when a part overflowed -- the frame is dropped
  // whole -- or the parts do not follow each other; the joined frame is the whole-volume compact frame, byte for byte.
  struct MeshPartFrame {
    std::vector<std::uint8_t> vertices; std::vector<tsdf_mesh_tile_row> table; std::vector<std::uint16_t> codes;
    std::vector<tsdf_packed_tap> taps;                                  // [nVertices()][n_streams] on a ring with taps: parts join by concatenation
    std::uint32_t vertex_stride = 0, overflow = 0, tiles[3] = {0, 0, 0};
    tsdf_mesh_part part{};
    std::uint64_t nVertices() const { return vertex_stride ? vertices.size() / vertex_stride : 0; }
    std::uint64_t nTriangles() const { return codes.size() / 3; }
    tsdf_mesh_compact compact() const { return tsdf_mesh_compact{table.data(), codes.data(), table.size(), {tiles[0], tiles[1], tiles[2]}, part.level}; }
  };
  void configureMeshStreamPart(bool normals, bool colours, unsigned level, unsigned max_vertices, unsigned max_triangles, unsigned max_surface_tiles, unsigned slots = 3) {
    check(tsdf_mesh_stream_config_part(m_ctx, (normals ? TSDF_MESH_NORMALS : 0u) | (colours ? TSDF_MESH_COLOURS : 0u), level, max_vertices, max_triangles,
                                       max_surface_tiles, slots));
  }
  tsdf_mesh_part meshFramePart() {
    tsdf_mesh_part out{};
    check(tsdf_mesh_stream_frame_part(m_ctx, &out));
    return out;
  }
  MeshPartFrame takeMeshPart(const tsdf_mesh_frame& held) {
    const tsdf_mesh_compact c = meshFrameCompact();
    MeshPartFrame p;
    p.part = meshFramePart();
    p.vertex_stride = held.vertex_stride; p.overflow = held.overflow;
    for (int a = 0; a < 3; ++a) p.tiles[a] = c.tiles[a];
    const std::uint8_t* v = (const std::uint8_t*)held.vertices;
    p.vertices.assign(v, v + held.n_vertices * held.vertex_stride);
    p.table.assign(c.table, c.table + c.n_tile_rows);
    p.codes.assign(c.triangles, c.triangles + held.n_triangles * 3);
    if (meshStreamHasTaps()) {
      const tsdf_mesh_taps t = meshStreamFrameTaps();
      p.taps.assign(t.taps, t.taps + t.n_vertices * t.n_streams);
    }
    return p;
  }
  static bool joinMeshParts(const std::vector<MeshPartFrame>& parts, MeshPartFrame& out) {
    out = MeshPartFrame{};
    if (parts.empty()) return false;
    for (std::size_t k = 0; k < parts.size(); ++k) {
      const MeshPartFrame& p = parts[k];
      if (p.overflow || p.vertex_stride != parts[0].vertex_stride || p.part.level != parts[0].part.level) return false;
      if (k && p.part.layers[0] != parts[k - 1].part.layers[1]) return false;
    }
    out.vertex_stride = parts[0].vertex_stride;
    for (int a = 0; a < 3; ++a) out.tiles[a] = parts[0].tiles[a];
    out.part = parts.back().part;
    out.part.layers[0] = parts[0].part.layers[0];
    std::uint64_t nv = 0, nt = 0;
    for (const MeshPartFrame& p : parts) {
      out.vertices.insert(out.vertices.end(), p.vertices.begin(), p.vertices.end());
      for (tsdf_mesh_tile_row row : p.table) {
        row.first_vertex += (std::uint32_t)nv; row.first_triangle += (std::uint32_t)nt;
        out.table.push_back(row);
      }
      out.codes.insert(out.codes.end(), p.codes.begin(), p.codes.end());
      out.taps.insert(out.taps.end(), p.taps.begin(), p.taps.end());
      nv += p.nVertices(); nt += p.nTriangles();
    }
    return true;
  }
  // after drawF(): never blocks; false = every slot is queued or held (or there is no volume yet), nothing was queued
  bool streamMesh(std::uint64_t tag) {
    const int32_t rc = tsdf_mesh_stream(m_ctx, tag);
    if (rc == TSDF_ERR_STATE) return false;
    check(rc);
    return true;
  }
  // the oldest streamed frame not yet released: false while it is not complete on the host (wait = false) or nothing is queued; out's pointers stay
  // valid until releaseMeshFrame()
  bool acquireMeshFrame(tsdf_mesh_frame& out, bool wait = true) {
    out = tsdf_mesh_frame{};
    int32_t ready = 0;
    const int32_t rc = tsdf_mesh_stream_acquire(m_ctx, wait ? 1 : 0, &out, &ready);
    if (rc == TSDF_ERR_STATE) return false;
    check(rc);
    return ready != 0;
  }
  void releaseMeshFrame() { check(tsdf_mesh_stream_release(m_ctx)); }
  MeshStreamStats meshStreamStats() {
    std::uint64_t s[4];
    check(tsdf_mesh_stream_stats(m_ctx, s));
    return MeshStreamStats{s[0], s[1], s[2], s[3]};
  }
  // ---- ray queries (tsdf_cast_rays): what does this ray hit?  The reference has no counterpart: its GUI picks nothing.
  // castRays marches caller-given rays (world coordinates, or the volume's unit cube) through the volume as it is now, by the draw's rule; viewRays writes
  // the draw's own rays of a pixel rectangle for the matrices last set; pick is the two for one pixel: the world position, normal and colour under it.
  struct RayResults { std::vector<tsdf_ray_hit> hits; std::vector<tsdf_ray_surface> surface; };   // surface: empty unless normals / colours were asked for
  struct RayStats { std::uint64_t rays = 0, hits = 0, samples = 0, fetched = 0; };
  struct Pick { bool hit = false; float position[3] = {0, 0, 0}, normal[3] = {0, 0, 0}, rgba[4] = {0, 0, 0, 0}; float t = -1.0f; std::uint32_t samples = 0; };
  void castRays(const std::vector<tsdf_ray>& rays, RayResults& out, bool normals = false, bool colours = false, bool unit_cube = false) {
    const std::uint32_t flags = (unit_cube ? TSDF_RAYS_UNIT_CUBE : 0u) | (normals ? TSDF_RAY_NORMALS : 0u) | (colours ? TSDF_RAY_COLOURS : 0u);
    out.hits.assign(rays.size(), tsdf_ray_hit{});
    out.surface.assign((normals || colours) ? rays.size() : 0, tsdf_ray_surface{});
    check(tsdf_cast_rays(m_ctx, rays.data(), rays.size(), flags, out.hits.data(), out.surface.empty() ? nullptr : out.surface.data()));
  }
  std::vector<tsdf_ray> viewRays(int x0, int y0, int w, int h) {
    std::vector<tsdf_ray> rays((w > 0 && h > 0) ? (std::size_t)w * (std::size_t)h : 0);
    check(tsdf_view_rays(m_ctx, m_mv, m_proj, x0, y0, w, h, rays.data()));
    return rays;
  }
  Pick pick(int x, int y, bool colours = true) {
    const std::vector<tsdf_ray> ray = viewRays(x, y, 1, 1);
    tsdf_ray_hit h{};
    tsdf_ray_surface s{};
    check(tsdf_cast_rays(m_ctx, ray.data(), 1, TSDF_RAYS_UNIT_CUBE | TSDF_RAY_NORMALS | (colours ? TSDF_RAY_COLOURS : 0u), &h, &s));
    Pick p;
    p.hit = (h.status & TSDF_RAY_HIT) != 0; p.t = h.t; p.samples = h.n_samples;
    if (p.hit) {
      for (int a = 0; a < 3; ++a) { p.position[a] = m_in.bbox_min[a] + h.pos[a] * (m_in.bbox_max[a] - m_in.bbox_min[a]); p.normal[a] = s.normal[a]; }   // vol_to_world, recon_integration.cpp:66-72
      for (int a = 0; a < 4; ++a) p.rgba[a] = s.rgba[a];
    }
    return p;
  }
  RayStats rayStats() {
    std::uint64_t s[4];
    check(tsdf_ray_stats(m_ctx, s));
    return RayStats{s[0], s[1], s[2], s[3]};
  }
  // ... where the volume is split into Z-slabs (tsdf_cast_rays_part): every slab's operator casts the SAME rays and answers for the samples it owns;
  // mergeRayParts joins the parts of contiguous slabs, in slab order, into what castRays gives on the whole volume -- per ray the part that hit with the
  // fewest samples, part 0 when none hit, the surface record with it.  Plain C++: the receiver of the parts needs no GPU.
  void castRaysPart(const std::vector<tsdf_ray>& rays, RayResults& out, bool normals = false, bool colours = false, bool unit_cube = false) {
    const std::uint32_t flags = (unit_cube ? TSDF_RAYS_UNIT_CUBE : 0u) | (normals ? TSDF_RAY_NORMALS : 0u) | (colours ? TSDF_RAY_COLOURS : 0u);
    out.hits.assign(rays.size(), tsdf_ray_hit{});
    out.surface.assign((normals || colours) ? rays.size() : 0, tsdf_ray_surface{});
    check(tsdf_cast_rays_part(m_ctx, rays.data(), rays.size(), flags, out.hits.data(), out.surface.empty() ? nullptr : out.surface.data()));
  }
  static void mergeRayParts(const std::vector<RayResults>& parts, RayResults& out) {
    out.hits.clear(); out.surface.clear();
    if (parts.empty()) return;
    const std::size_t n = parts[0].hits.size();
    const bool surface = !parts[0].surface.empty();
    for (const RayResults& p : parts)
      if (p.hits.size() != n || p.surface.size() != (surface ? n : 0)) throw std::invalid_argument("mergeRayParts: the parts answer different casts");
    out.hits.resize(n);
    out.surface.resize(surface ? n : 0);
    for (std::size_t i = 0; i < n; ++i) {
      std::size_t win = 0;
      std::uint32_t best = 0xffffffffu;
      for (std::size_t k = 0; k < parts.size(); ++k) {
        const tsdf_ray_hit& h = parts[k].hits[i];
        if ((h.status & TSDF_RAY_HIT) && h.n_samples < best) { best = h.n_samples; win = k; }
      }
      out.hits[i] = parts[win].hits[i];
      if (surface) out.surface[i] = parts[win].surface[i];
    }
  }
  // ---- texture taps (tsdf_texture_taps): camera-resolution colour for a receiver of the mesh.  The reference has no counterpart: its client runs
  // blendColors per pixel against the colour images and the LUT volumes.  textureTaps gives, per point (world coordinates, or the volume's unit cube) and
  // stream, where that stream's colour image is read and the two numbers blendColors weights the read with; meshTextureTaps the same at the vertices of the
  // last meshExtract, evaluated on the device; a receiver blends per fragment by the rule in the header.  Records are [points][streams].
  struct TextureTaps { std::vector<tsdf_texture_tap> taps; std::vector<tsdf_sensor_tap> sensor; std::uint64_t points = 0; std::uint32_t streams = 0; };   // sensor: empty unless asked for
  struct TextureTapStats { std::uint64_t points = 0, streams = 0, with_quality = 0, not_evaluated = 0; };
  void textureTaps(const std::vector<float>& xyz, TextureTaps& out, bool sensor = false, bool unit_cube = false) {
    const std::uint32_t flags = (unit_cube ? TSDF_TAPS_UNIT_CUBE : 0u) | (sensor ? TSDF_TAPS_SENSOR : 0u);
    out.points = xyz.size() / 3; out.streams = m_in.num_kinects;
    const std::size_t records = (std::size_t)out.points * out.streams;
    out.taps.assign(records, tsdf_texture_tap{});
    out.sensor.assign(sensor ? records : 0, tsdf_sensor_tap{});
    check(tsdf_texture_taps(m_ctx, xyz.data(), out.points, flags, out.taps.data(), sensor ? out.sensor.data() : nullptr));
  }
  void meshTextureTaps(TextureTaps& out, bool sensor = false) {
    check(tsdf_mesh_texture_taps(m_ctx, sensor ? TSDF_TAPS_SENSOR : 0u, &out.points, &out.streams));
    const std::size_t records = (std::size_t)out.points * out.streams;
    out.taps.assign(records, tsdf_texture_tap{});
    out.sensor.assign(sensor ? records : 0, tsdf_sensor_tap{});
    check(tsdf_mesh_download_texture_taps(m_ctx, out.taps.data(), sensor ? out.sensor.data() : nullptr));
  }
  TextureTapStats textureTapStats() {
    std::uint64_t s[4];
    check(tsdf_texture_tap_stats(m_ctx, s));
    return TextureTapStats{s[0], s[1], s[2], s[3]};
  }
  // ---- kinect::ReconPoints::draw() (recon_points.cpp:71-111) on the same inputs: the point back-end for A/B comparison
  void uploadNormals(const float* normals_rgb) { check(tsdf_upload_normals(m_ctx, normals_rgb)); }
  void drawPoints() { check(tsdf_draw_points(m_ctx, m_mv, m_proj)); }
  // ---- kinect::ReconTrigrid::draw() (recon_trigrid.cpp:85-148)
  void setMinLength(float v) { check(tsdf_set_min_length(m_ctx, v)); }
  void drawTrigrid() { check(tsdf_draw_trigrid(m_ctx, m_mv, m_proj)); }
  // ---- kinect::ReconMVT::draw() (recon_mvt.cpp:84-150): reads the raw frame of the last raw / wire upload
  void drawMVT() { check(tsdf_draw_mvt(m_ctx, m_mv, m_proj)); }
  tsdf_ctx* handle() const { return m_ctx; }
  const float* modelview() const { return m_mv; }
  const float* projection() const { return m_proj; }

 private:
  void check(int32_t rc) const { if (rc != TSDF_OK) throw std::runtime_error(std::string("ReconIntegrationHip: ") + tsdf_last_error(m_ctx)); }
  ReconInputs m_in;
  tsdf_ctx* m_ctx = nullptr;
  MeshCounts m_mesh; std::uint32_t m_mesh_flags = 0;   // of the last extractMesh
  MeshCounts m_slab; std::uint32_t m_slab_flags = 0; unsigned m_slab_level = 0; bool m_slab_valid = false;   // of the last extractMeshSlab that succeeded
  // the sizes of seam table and arrays come from these: without them nothing is handed to the library to fill
  void requireSlabPart() const { if (!m_slab_valid) throw std::logic_error("ReconIntegrationHip: no slab mesh (extractMeshSlab)"); }
  MeshSlabComponentCounts m_slab_components; std::uint64_t m_slab_owned = 0; bool m_slab_components_valid = false, m_slab_owned_valid = false;   // of the last meshSlabComponents / linkMeshSlabComponents
  void requireSlabComponents() const {
    if (!m_slab_valid || !m_slab_components_valid) throw std::logic_error("ReconIntegrationHip: no components of the slab's part (meshSlabComponents after meshSlabLink)");
  }
  float m_mv[16], m_proj[16];
  float m_brick_size;
};

// The client's overlays after drawF() in mono mode (source/kinect_client.cpp:672-683), over the SAME context and its matrices (setMatrices):
// "Draw TSDF" is kinect::ReconCalibs (recon_calibs.hpp), "Draw frustums" CalibVolumes::drawFrustums() (CalibVolumes.cpp:214-218).
class ReconCalibsHip {
 public:
  explicit ReconCalibsHip(ReconIntegrationHip& recon) : m_recon(recon) {}
  void draw() { check(tsdf_draw_calibvis(m_recon.handle(), m_recon.modelview(), m_recon.projection())); }
  void setActiveKinect(unsigned num_kinect) { check(tsdf_set_active_kinect(m_recon.handle(), num_kinect)); }   // validates only: changes no output

 private:
  void check(int32_t rc) const { if (rc != TSDF_OK) throw std::runtime_error(std::string("ReconCalibsHip: ") + tsdf_last_error(m_recon.handle())); }
  ReconIntegrationHip& m_recon;
};
// the drawing side of CalibVolumes (its 3-D textures are ReconIntegrationHip::setCalibration)
class CalibVolumesHip {
 public:
  explicit CalibVolumesHip(ReconIntegrationHip& recon) : m_recon(recon) {}
  void drawFrustums() const { check(tsdf_draw_frustums(m_recon.handle(), m_recon.modelview(), m_recon.projection())); }

 private:
  void check(int32_t rc) const { if (rc != TSDF_OK) throw std::runtime_error(std::string("CalibVolumesHip: ") + tsdf_last_error(m_recon.handle())); }
  ReconIntegrationHip& m_recon;
};

// The last two draws of the client's mono frame (kinect_client.cpp:685-707), over the same context and its matrices: the bounding-box wireframe
// g_bbox.draw() (gloost::BoundingBox::draw, BoundingBox.cpp:298-318; the box is the context's bbox_min / bbox_max) and the texture view
// TextureBlitter::blit(15 + g_num_texture % 2, resolution_full / 2) (texture_blitter.cpp).
class BoundingBoxHip {
 public:
  explicit BoundingBoxHip(ReconIntegrationHip& recon) : m_recon(recon) {}
  void draw() const { check(tsdf_draw_bbox(m_recon.handle(), m_recon.modelview(), m_recon.projection())); }

 private:
  void check(int32_t rc) const { if (rc != TSDF_OK) throw std::runtime_error(std::string("BoundingBoxHip: ") + tsdf_last_error(m_recon.handle())); }
  ReconIntegrationHip& m_recon;
};
class TextureBlitterHip {
 public:
  explicit TextureBlitterHip(ReconIntegrationHip& recon) : m_recon(recon) {}
  // unit 15 (the hole-filling atlas) or 16 (the depth-limit image): the client's 15 + g_num_texture % 2; the viewport is resolution_full / 2
  void blit(unsigned unit) const {
    if (unit != 15 && unit != 16) throw std::invalid_argument("TextureBlitterHip: the client blits texture unit 15 or 16");
    check(tsdf_draw_textures(m_recon.handle(), unit - 15));
  }

 private:
  void check(int32_t rc) const { if (rc != TSDF_OK) throw std::runtime_error(std::string("TextureBlitterHip: ") + tsdf_last_error(m_recon.handle())); }
  ReconIntegrationHip& m_recon;
};

// The input side: kinect::NetKinectArray's public surface (framework/NetKinectArray.h:40-55) over the SAME context, for callers
// that also replace the GL upload / pre-process.  The ZMQ socket stays with the caller: where readLoop() memcpy's the received
// message into the PBOs (NetKinectArray.cpp:513-523), hand it to submit().
class NetKinectArrayHip {
 public:
  // colour_format: CalibrationFiles::isCompressedRGB() (0 RGB8 / 1 DXT1 / 5 DXT5); compressed_depth: isCompressedDepth()
  NetKinectArrayHip(ReconIntegrationHip& recon, unsigned colour_format, bool compressed_depth) : m_ctx(recon.handle()) {
    check(tsdf_set_wire_format(m_ctx, colour_format, compressed_depth ? TSDF_DEPTH_U8 : TSDF_DEPTH_F32));
  }
  // per sensor: KinectCalibrationFile::isCompressedDepth()/getNear()/getFar(), CalibVolumes::getDepthLimits(i)
  void setSensor(unsigned i, bool compressed_depth, float near_m, float far_m, float cv_min_d, float cv_max_d) {
    check(tsdf_set_depth_compression(m_ctx, i, compressed_depth, near_m, far_m));
    check(tsdf_set_depth_limits(m_ctx, i, cv_min_d, cv_max_d));
  }
  std::size_t messageBytes() const { uint64_t n = 0; tsdf_wire_sizes(m_ctx, nullptr, nullptr, &n); return (std::size_t)n; }
  void submit(const void* zmq_message, std::size_t bytes) { check(tsdf_upload_wire_frame(m_ctx, zmq_message, bytes, &m_frametime)); m_dirty = true; }   // readLoop(), :482-529
  bool update() { const bool fresh = m_dirty; m_dirty = false; return fresh; }      // NetKinectArray.cpp:225-236: "a new frame was uploaded"
  void processTextures() { check(tsdf_process_textures(m_ctx)); }                    // :309-426 (marks the bricks itself)
  void filterTextures(bool f) { m_filter = f; apply(); }                             // :463-476: each setter re-runs the passes
  void useProcessedDepths(bool f) { m_processed = f; apply(); }
  void refineBoundary(bool f) { m_refine = f; apply(); }
  double frameTime() const { return m_frametime; }
  // NetKinectArray.cpp:428-437,464-466: the first of the seven texture units (color, depth, quality, normal, silhouette, morph_depth, color_lab).
  // Nothing is bound here; the GUI encodes the array it wants to see as unit = start + type (SensorTextureViewHip)
  void setStartTextureUnit(unsigned start_texture_unit) { m_start_texture_unit = start_texture_unit; }
  unsigned getStartTextureUnit() const { return m_start_texture_unit; }
  tsdf_ctx* handle() const { return m_ctx; }

 private:
  void apply() { check(tsdf_set_preprocess(m_ctx, m_filter, m_processed, m_refine)); }
  void check(int32_t rc) const { if (rc != TSDF_OK) throw std::runtime_error(std::string("NetKinectArrayHip: ") + tsdf_last_error(m_ctx)); }
  tsdf_ctx* m_ctx;
  bool m_dirty = false, m_filter = true, m_processed = true, m_refine = true;
  double m_frametime = 0.0;
  unsigned m_start_texture_unit = 0;                                                 // NetKinectArray.cpp:69
};

// The GUI's "Show textures" windows (kinect_client.cpp:483-515): ImGui::Image of one layer of one of NetKinectArray's texture arrays, drawn by
// the ImGui back-end's array mode (imgui_impl_glfw_glb.cpp:111-124).  `info` is the reference's TexInfo (imgui_impl_glfw_glb.h:28-40) -- any
// struct with its two members: unit = getStartTextureUnit() + type, layer = -stream - 1 -- so a caller that holds an ImDrawCmd forwards
// what it memcpy's out of TextureId, the image quad of the command's vertices and its ClipRect unchanged.
class SensorTextureViewHip {
 public:
  explicit SensorTextureViewHip(NetKinectArrayHip const& nka) : m_nka(nka) {}
  // ImVec2(width, width / aspect) of kinect_client.cpp:502-509
  std::array<float, 2> imageSize(float width) const {
    std::array<float, 2> s{{0.0f, 0.0f}};
    check(tsdf_sensor_view_size(m_nka.handle(), width, s.data()));
    return s;
  }
  template <class TexInfoT>
  void draw(TexInfoT const& info, const float p_min[2], const float p_max[2], const float clip_rect[4] = nullptr) const {
    const long unit = (long)info.unit, start = (long)m_nka.getStartTextureUnit(), layer = (long)info.layer;
    if (unit < start || unit > start + 6) throw std::invalid_argument("SensorTextureViewHip: texture unit outside NetKinectArray's start .. start + 6");
    if (layer >= 0) throw std::invalid_argument("SensorTextureViewHip: layer >= 0 is a plain 2-D texture id, not a texture array layer");
    const float rect[4] = {p_min[0], p_min[1], p_max[0], p_max[1]};
    check(tsdf_draw_sensor_texture(m_nka.handle(), (uint32_t)(unit - start), (uint32_t)(-(layer + 1)), rect, clip_rect));
  }

 private:
  void check(int32_t rc) const { if (rc != TSDF_OK) throw std::runtime_error(std::string("SensorTextureViewHip: ") + tsdf_last_error(m_nka.handle())); }
  NetKinectArrayHip const& m_nka;
};

}  // namespace kinect

#endif  // RECON_INTEGRATION_HIP_HPP
