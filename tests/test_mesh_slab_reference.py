"""CPU: the numpy restatement of the mesh extraction on Z-slab contexts (tests/mesh_slab_reference.py) against the whole-volume references, and the
slab driver's collective (SlabDriver.extract_mesh) over gloo with stand-in backends that serve reference parts."""
import os
import socket
from importlib import import_module

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import mesh_lod_reference as L
import mesh_reference as M
import mesh_slab_reference as S

BBOX = ((-1.0, 0.0, -1.0), (1.0, 2.2, 1.0))
LIMIT = 0.05
# (rx, ry, rz), level, slabs: the GPU test's cases (tests/test_gpu_mesh_slab.py)
CASES = [((32, 32, 32), 0, [(0, 16), (16, 32)]),
         ((32, 32, 32), 0, [(0, 8), (8, 16), (16, 24), (24, 32)]),
         ((20, 12, 28), 0, [(0, 8), (8, 24), (24, 28)]),
         ((24, 20, 64), 1, [(0, 32), (32, 64)]),
         ((24, 20, 64), 2, [(0, 32), (32, 64)]),
         ((24, 20, 64), 1, [(0, 16), (16, 64)]),
         ((16, 16, 16), 0, [(0, 16)])]
SEED = 20261019


def _case(res, level, slabs):
    vol = S.crafted_volume(res, slabs, SEED, LIMIT)
    ref, parts = S.split(vol, LIMIT, *BBOX, level, slabs)
    return vol, ref, parts


@pytest.mark.parametrize("res,level,slabs", CASES)
def test_ranges_tile_the_whole_mesh(res, level, slabs):
    vol, ref, parts = _case(res, level, slabs)
    whole = L.extract_lod(vol, LIMIT, *BBOX, level)
    assert ref["position"].tobytes() == whole["position"].tobytes() and ref["triangles"].tobytes() == whole["triangles"].tobytes()
    assert len(whole["position"]) > 100 and len(whole["triangles"]) > 100
    assert parts[0]["vertices"][0] == 0 and parts[0]["triangles"][0] == 0
    assert parts[-1]["vertices"][1] == len(whole["position"]) and parts[-1]["triangles"][1] == len(whole["triangles"])
    for a, b in zip(parts, parts[1:]):
        assert a["vertices"][1] == b["vertices"][0] and a["triangles"][1] == b["triangles"][0]
    for p in parts:
        (v0, v1), (t0, t1) = p["vertices"], p["triangles"]
        tri = whole["triangles"][t0:t1].astype(np.int64)
        # a part's triangles index its own vertices and, at most, those of the first layer of the slab above
        assert tri.size == 0 or (tri.min() >= v0)
        if p is parts[-1]:
            assert tri.size == 0 or tri.max() < v1
    # every seam is crossed: a case that joined without looking above would not pass
    for p in parts[:-1]:
        assert S.crosses_seam(ref, p) > 0


@pytest.mark.parametrize("res,level,slabs", CASES)
def test_seam_tables_are_the_reference_tile_bases(res, level, slabs):
    vol, ref, parts = _case(res, level, slabs)
    s = 1 << level
    ntx, nty, _ = ref["lattice_tiles"]
    lat = ref["voxel"] // s
    for p in parts:
        l0 = p["layers"][0]
        assert p["seam"].shape == (nty, ntx) and p["seam"].dtype == np.uint32
        for ty in range(nty):
            for tx in range(ntx):
                # vertices of the slab in front of this tile: lower tiles of the same layer (the layer is the slab's first)
                before = (lat[:, 2] >> 3 == l0) & (((lat[:, 1] >> 3) * ntx + (lat[:, 0] >> 3)) < ty * ntx + tx)
                assert int(p["seam"][ty, tx]) == int(before.sum())


@pytest.mark.parametrize("res,level,slabs", CASES)
def test_linked_parts_concatenate_to_the_whole_triangle_array(res, level, slabs):
    vol, ref, parts = _case(res, level, slabs)
    out = []
    for k, p in enumerate(parts):
        above = parts[k + 1]["seam"] if k + 1 < len(parts) else None
        out.append(S.link(S.unlinked(ref, p), p["vertices"][0], above))
    assert np.concatenate(out).tobytes() == ref["triangles"].tobytes()
    # linking again with another base shifts every index by the difference
    u = S.unlinked(ref, parts[0])
    above = parts[1]["seam"] if len(parts) > 1 else None
    assert (S.link(u, 1000, above).astype(np.int64) - S.link(u, 0, above).astype(np.int64) == 1000).all()


def test_misaligned_slab_is_refused():
    with pytest.raises(ValueError):
        S.slab_layers((64, 20, 24), 1, 0, 24)
    assert S.slab_layers((64, 20, 24), 0, 0, 24) == (0, 3)
    assert S.slab_layers((28, 12, 20), 0, 24, 28) == (3, 4)


# ---- SlabDriver.extract_mesh over gloo: stand-in backends that hold a reference part the way a context holds it before the link
class FakeMeshSlab:
    def __init__(self, res, ref, part):
        self.res = res
        self.ref, self.part = ref, part
        self.u = None
        self.tri = None

    def extract_mesh_slab(self, normals=True, colours=True, level=0):
        self.u = S.unlinked(self.ref, self.part)
        (v0, v1), (t0, t1) = self.part["vertices"], self.part["triangles"]
        return v1 - v0, t1 - t0

    def mesh_slab_seam(self):
        return self.part["seam"].copy()

    def mesh_slab_link(self, vertex_base, above_seam=None):
        self.tri = S.link(self.u, vertex_base, above_seam)

    def mesh_slab_download(self, normals=True, colours=True, triangles=True):
        v0, v1 = self.part["vertices"]
        return dict(position=self.ref["position"][v0:v1].copy(), triangles=self.tri)


GLOO_CASE = ((20, 12, 28), 0, [(0, 8), (8, 28)])


def _mesh_worker(rank, world, port, q, dedicated):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mgpu = import_module("rgbd-recon_amd.multigpu")
        res, level, slabs = GLOO_CASE
        if dedicated:                                                    # rank 0 owns no slab: the workers split the volume
            slabs = [(0, 16), (16, 28)]
        vol, ref, parts = _case(res, level, slabs)
        part = parts[max(rank - 1, 0)] if dedicated else parts[rank]
        drv = mgpu.SlabDriver(FakeMeshSlab(res, ref, part), rank, world, "cpu", view=(8, 4), halo="recompute",
                              compositor="dedicated" if dedicated else "shared")
        got = drv.extract_mesh(normals=False, colours=False, level=level)
        ok = True
        if dedicated and rank == 0:
            ok &= got["vertex_base"] == 0 and len(got["part"]["position"]) == 0 and got["counts"][0].tolist() == [0, 0]
        else:
            ok &= got["vertex_base"] == part["vertices"][0]
            ok &= got["part"]["position"].tobytes() == ref["position"][part["vertices"][0]:part["vertices"][1]].tobytes()
        if rank == 0:
            ok &= got["mesh"]["position"].tobytes() == ref["position"].tobytes()
            ok &= got["mesh"]["triangles"].tobytes() == ref["triangles"].tobytes() and got["mesh"]["triangles"].dtype == np.uint32
        else:
            ok &= "mesh" not in got
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.timeout(900)
@pytest.mark.parametrize("world,dedicated", [(2, False), (3, True)])
def test_slab_driver_extract_mesh_gloo(world, dedicated):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_mesh_worker, args=(r, world, port, q, dedicated)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
        assert p.exitcode == 0
    got = dict(q.get(timeout=5) for _ in range(world))
    assert got == {r: True for r in range(world)}


def test_one_device_fallback_joins_reference_parts():
    mgpu = import_module("rgbd-recon_amd.multigpu")
    res, level, slabs = CASES[2]
    vol, ref, parts = _case(res, level, slabs)
    out = mgpu.mesh_slabs_on_one_device([FakeMeshSlab(res, ref, p) for p in parts], normals=False, colours=False, level=level)
    assert out["position"].tobytes() == ref["position"].tobytes() and out["triangles"].tobytes() == ref["triangles"].tobytes()
    assert out["counts"] == [(p["vertices"][1] - p["vertices"][0], p["triangles"][1] - p["triangles"][0]) for p in parts]
