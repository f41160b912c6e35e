// Stand-alone host program for tests/test_mesh_measure_reference.py: runs csrc/mesh_measure.hpp -- the quantisation, the packing, a triangle's exact
// doubled area and six-fold volume, and the split and join of the volume sum -- on data read from a file, under the host sanitizers (the test compiles it
// with -fsanitize=address,undefined -fno-sanitize-recover=all and runs it directly).
// in:  float bbox_min[3]; double scale; uint32 V, T, R; float position[V][3]; uint32 triangle[T][3]; uint64 raw[R][3] (triangles given as packed words).
// out: uint64 packed[V]; per triangle of the mesh, then per raw triangle: uint64 a2, int64 v6; then per group (mesh, raw) the sum of v6 through the split:
//      uint64 volume6_lo, int64 volume6_hi.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mesh_measure.hpp"

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

template <typename T>
static bool read_all(std::FILE* f, std::vector<T>& v, size_t n) { v.resize(n); return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n; }

struct Sum { uint64_t lo = 0; int64_t hi = 0; };
static bool emit(std::FILE* out, uint64_t w0, uint64_t w1, uint64_t w2, Sum& sum) {
  const rr::MeasureTriangle m = rr::measure_triangle(w0, w1, w2);
  sum.lo += rr::measure_v6_lo(m.v6);
  sum.hi += rr::measure_v6_hi(m.v6);
  return std::fwrite(&m.a2, 8, 1, out) == 1 && std::fwrite(&m.v6, 8, 1, out) == 1;
}

int main(int argc, char** argv) {
  using namespace rr;
  CHECK(argc == 3);
  std::FILE* in = std::fopen(argv[1], "rb");
  std::FILE* out = std::fopen(argv[2], "wb");
  CHECK(in && out);
  float bbox_min[3];
  double scale = 0;
  uint32_t n[3];
  CHECK(std::fread(bbox_min, 4, 3, in) == 3 && std::fread(&scale, 8, 1, in) == 1 && std::fread(n, 4, 3, in) == 3);
  std::vector<float> pos;
  std::vector<uint32_t> tri;
  std::vector<uint64_t> raw;
  CHECK(read_all(in, pos, (size_t)n[0] * 3) && read_all(in, tri, (size_t)n[1] * 3) && read_all(in, raw, (size_t)n[2] * 3));
  std::vector<uint64_t> packed(n[0]);
  for (uint32_t v = 0; v < n[0]; ++v) {
    uint32_t q[3];
    for (int a = 0; a < 3; ++a) q[a] = measure_quantise(pos[(size_t)v * 3 + a], bbox_min[a], scale);
    packed[v] = measure_pack(q[0], q[1], q[2]);
    int64_t back[3];
    measure_unpack(packed[v], back);
    CHECK(back[0] == (int64_t)q[0] && back[1] == (int64_t)q[1] && back[2] == (int64_t)q[2]);
  }
  CHECK(n[0] == 0 || std::fwrite(packed.data(), 8, n[0], out) == n[0]);
  Sum mesh, hand;
  for (uint32_t t = 0; t < n[1]; ++t) {
    const uint32_t* i = &tri[(size_t)t * 3];
    CHECK(i[0] < n[0] && i[1] < n[0] && i[2] < n[0]);
    CHECK(emit(out, packed[i[0]], packed[i[1]], packed[i[2]], mesh));
  }
  for (uint32_t t = 0; t < n[2]; ++t) CHECK(emit(out, raw[(size_t)t * 3], raw[(size_t)t * 3 + 1], raw[(size_t)t * 3 + 2], hand));
  for (const Sum& s : {mesh, hand}) {
    uint64_t lo; int64_t hi;
    measure_v6_join(s.lo, s.hi, &lo, &hi);
    CHECK(std::fwrite(&lo, 8, 1, out) == 1 && std::fwrite(&hi, 8, 1, out) == 1);
  }
  CHECK(std::fclose(out) == 0);
  std::fclose(in);
  std::puts("mesh measure ok");
  return 0;
}
