"""CPU: which lattice tile layers a Z-slab's part ring owns, the alignment rule and the record slots (rgbd-recon_amd/csrc/result_paths.hpp:
MeshPartLayers, HIP-free) as a stand-alone program with its own main, built with the host address and undefined-behaviour sanitizers, against
mesh_slab_reference.slab_layers for every slab of the GPU tests' grids and of the 512^3 x 8 configuration."""
import os
import subprocess

import mesh_slab_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbd-recon_amd", "csrc")

MAIN = r'''
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "result_paths.hpp"
using namespace rr;

// argv: res_z level z0 z1  ->  "layer0 layer1 top aligned seam_tiles record_slots" for a 5 x 3 lattice-tile layer and 100 owned slots
int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const int res_z = std::atoi(argv[1]), level = std::atoi(argv[2]), z0 = std::atoi(argv[3]), z1 = std::atoi(argv[4]);
  const int storage_ntz = (res_z + 7) / 8, cr = (res_z + (1 << level) - 1) >> level, lattice_ntz = (cr + 7) / 8;
  const MeshPartLayers p = MeshPartLayers::of(z0 / 8, (z1 + 7) / 8, storage_ntz, level, lattice_ntz);
  std::printf("%d %d %d %d %llu %llu\n", p.layer0, p.layer1, (int)p.top, (int)p.aligned, (unsigned long long)p.seam_tiles(15), (unsigned long long)p.record_slots(100, 15));
  return kMeshPartRecordBytes == 64 ? 0 : 1;
}
'''


def test_part_layers_under_the_host_sanitizers(tmp_path):
    src = tmp_path / "mesh_part_layers_main.cpp"
    src.write_text(MAIN)
    exe = str(tmp_path / "mesh_part_layers_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, str(src), "-o", exe])
    cases = [(32, 0, 0, 16), (32, 0, 16, 32), (32, 0, 8, 16), (28, 0, 8, 24), (28, 0, 24, 28), (64, 1, 0, 32), (64, 1, 32, 64), (64, 2, 0, 32), (64, 2, 32, 64),
             (64, 1, 0, 16), (64, 1, 16, 64), (64, 1, 0, 24), (64, 2, 0, 24), (64, 2, 0, 16), (64, 1, 24, 64), (35, 0, 0, 35), (35, 1, 0, 35), (35, 2, 0, 35)]
    cases += [(512, level, 64 * k, 64 * (k + 1)) for level in (0, 1, 2) for k in range(8)]
    walked = 0
    for res_z, level, z0, z1 in cases:
        p = subprocess.run([exe] + [str(x) for x in (res_z, level, z0, z1)], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        l0, l1, top, aligned, seam, slots = (int(x) for x in p.stdout.split())
        try:
            want = S.slab_layers((res_z, 8, 8), level, z0, z1)
        except ValueError:
            want = None
        assert bool(aligned) == (want is not None), (res_z, level, z0, z1)
        assert top == (z1 == res_z) and seam == (0 if top else 15) and slots == 100 + seam
        if want is not None:
            assert (l0, l1) == want, (res_z, level, z0, z1)
            walked += 1
    assert walked >= 30 and walked < len(cases)                           # both verdicts occur
