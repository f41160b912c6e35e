// Stand-alone host program for tests/test_mesh_slab_component_reference.py: runs csrc/mesh_cc_seams.hpp -- the merge of the slabs' seam lists and the
// check of the links a slab is handed -- on cases read from a file, under the host sanitizers (the test compiles it with -fsanitize=address,undefined
// and runs it directly).
// in:  uint32 cases; per case uint32 slabs; per slab six uint64 {vertex_base, n_vertices, n_local, n_down, n_up, n_roots}, then the down, up and root
//      records as the library lays them out.
// out: per case int32 result of merge_component_seams; when 0: uint64 components, uint64 component_base[slabs], the links; and one int32 per slab,
//      component_links_check of the slab's own links (0) -- a case that is refused writes its result alone.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mesh_cc_seams.hpp"

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

template <typename T>
static bool read_all(std::FILE* f, std::vector<T>& v, uint64_t n) { v.resize((size_t)n); return n == 0 || std::fread(v.data(), sizeof(T), (size_t)n, f) == n; }

int main(int argc, char** argv) {
  using namespace rr;
  static_assert(sizeof(tsdf_mesh_seam_vertex) == 8 && sizeof(tsdf_mesh_seam_root) == 16 && sizeof(tsdf_mesh_component_link) == 32, "the records' sizes");
  CHECK(argc == 3);
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  CHECK(in && out);
  uint32_t cases = 0;
  CHECK(std::fread(&cases, 4, 1, in) == 1);
  for (uint32_t c = 0; c < cases; ++c) {
    uint32_t n_slabs = 0;
    CHECK(std::fread(&n_slabs, 4, 1, in) == 1);
    std::vector<tsdf_mesh_component_seams> slabs(n_slabs);
    std::vector<std::vector<tsdf_mesh_seam_vertex>> down(n_slabs), up(n_slabs);
    std::vector<std::vector<tsdf_mesh_seam_root>> roots(n_slabs);
    uint64_t n_links = 0;
    for (uint32_t k = 0; k < n_slabs; ++k) {
      uint64_t h[6];
      CHECK(std::fread(h, 8, 6, in) == 6);
      CHECK(read_all(in, down[k], h[3]) && read_all(in, up[k], h[4]) && read_all(in, roots[k], h[5]));
      slabs[k] = tsdf_mesh_component_seams{h[0], h[1], h[2], h[3], h[4], h[5], down[k].data(), up[k].data(), roots[k].data()};
      n_links += h[5];
    }
    // nothing is written by a refused merge: the outputs keep their fill
    const tsdf_mesh_component_link fill{7u, 7u, 7u, 7u, 7u, 7u, 7u, 7u};
    std::vector<tsdf_mesh_component_link> links((size_t)n_links + 1, fill);
    std::vector<uint64_t> base(n_slabs + 1u, 77u);
    uint64_t components = 777u;
    const int32_t rc = merge_component_seams(slabs.data(), n_slabs, base.data(), links.data(), &components);
    CHECK(std::fwrite(&rc, 4, 1, out) == 1);
    CHECK(links[(size_t)n_links].root == 7u && base[n_slabs] == 77u);
    if (rc) {
      for (const tsdf_mesh_component_link& l : links) CHECK(l.root == 7u && l.component == 7u);
      for (uint64_t b : base) CHECK(b == 77u);
      CHECK(components == 777u);
      continue;
    }
    CHECK(std::fwrite(&components, 8, 1, out) == 1);
    CHECK(n_slabs == 0 || std::fwrite(base.data(), 8, n_slabs, out) == n_slabs);
    CHECK(n_links == 0 || std::fwrite(links.data(), sizeof(links[0]), (size_t)n_links, out) == n_links);
    uint64_t first = 0;
    for (uint32_t k = 0; k < n_slabs; ++k) {
      const tsdf_mesh_component_link* mine = links.data() + first;
      const uint64_t n = slabs[k].n_roots;
      const int32_t ok = component_links_check(roots[k].data(), n, slabs[k].vertex_base, mine, n);
      CHECK(std::fwrite(&ok, 4, 1, out) == 1);
      // ... and the check refuses what must not reach a scatter
      CHECK(component_links_check(roots[k].data(), n, slabs[k].vertex_base, mine, n + 1) == 1);
      if (n) {
        std::vector<tsdf_mesh_component_link> bad(mine, mine + n);
        bad[n - 1].root += 1u;
        CHECK(component_links_check(roots[k].data(), n, slabs[k].vertex_base, bad.data(), n) == 2);
        bad[n - 1] = mine[n - 1]; bad[n - 1].final_root = bad[n - 1].root + 1u;
        CHECK(component_links_check(roots[k].data(), n, slabs[k].vertex_base, bad.data(), n) == 3);
        if (bad[n - 1].root > slabs[k].vertex_base && seam_find(roots[k].data(), n, bad[n - 1].root - 1u) < 0) {   // an own vertex that is no exported root
          bad[n - 1].final_root = bad[n - 1].root - 1u;
          CHECK(component_links_check(roots[k].data(), n, slabs[k].vertex_base, bad.data(), n) == 4);
        }
      }
      first += n;
    }
  }
  CHECK(std::fclose(out) == 0);
  std::fclose(in);
  std::puts("mesh cc seams ok");
  return 0;
}
