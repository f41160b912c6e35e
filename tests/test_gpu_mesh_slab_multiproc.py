"""-m gpu: SlabDriver.extract_mesh with real contexts in separate processes, all on the one GPU of the box, over gloo (the pattern of
tests/test_gpu_multiproc.py): a dedicated compositor and two slabs with exchanged halos.  After a frame every rank extracts its part, the counts and
the seam tables are all-gathered, and rank 0 holds the whole mesh: the bytes an unpartitioned context extracts."""
import os
import socket
import time
from importlib import import_module

import pytest

pytestmark = pytest.mark.gpu

KW = dict(res=(64, 64, 64), brick_size=[2.0 / 8, 2.2 / 8, 2.0 / 8], limit=0.04, view=(160, 90))


def _worker(rank, world, port, q, level):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist
    import rgbd_recon_amd as rr
    mgpu = import_module("rgbd-recon_amd.multigpu")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        scene = rr.scene.make_scene(n_streams=4, width=160, height=120, lut_res=32, inv_res=32)
        mv, pr = rr.scene.default_view(*KW["view"])
        hip = rr.ReconIntegrationHip(scene, slab=mgpu.worker_slab_range(KW["res"][2], rank, world), **KW)
        drv = mgpu.SlabDriver(hip, rank, world, "cuda:0", view=KW["view"], halo="exchange", composite="dense", compositor="dedicated")
        drv.frame(mv, pr)                                                # integrates and exchanges the halos
        drv.finish()
        got = drv.extract_mesh(normals=True, colours=True, level=level)
        ok = int(got["counts"][0, 0]) == 0 and int(got["vertex_base"]) == int(got["counts"][:rank, 0].sum())
        ok &= len(got["part"]["position"]) == int(got["counts"][rank, 0]) and len(got["part"]["triangles"]) == int(got["counts"][rank, 1])
        if rank == 0:
            whole = rr.ReconIntegrationHip(scene, **KW)
            whole.clearOccupiedBricks(); whole.markBricks(); whole.updateOccupiedBricks(); whole.integrate()
            want = whole.extract_mesh(normals=True, colours=True, level=level)
            ok &= len(want["position"]) > 200 and bool((got["counts"][1:, 0] > 0).all())      # both slabs hold surface
            for k in ("position", "normal", "colour", "triangles"):
                ok &= got["mesh"][k].dtype == want[k].dtype and got["mesh"][k].tobytes() == want[k].tobytes()
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("level", [0, 1])
def test_slab_driver_extract_mesh_equals_the_whole_volume(level):
    import torch                     # first import on a fresh box takes minutes: pay it here, not in all children at once
    import torch.multiprocessing as mp
    assert torch.cuda.is_available()
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 3, port, q, level)) for r in range(3)]
    for p in procs:
        p.start()
    deadline = time.monotonic() + 300                                    # one deadline for all ranks
    while time.monotonic() < deadline and all(p.exitcode in (None, 0) for p in procs) and any(p.exitcode is None for p in procs):
        next(p for p in procs if p.exitcode is None).join(0.2)           # (ends early when a rank has failed: the others then wait in a collective)
    codes = [p.exitcode for p in procs]
    for p in procs:
        if p.is_alive():                                                 # a rank that raised leaves the others waiting in a collective
            p.terminate()
    assert codes == [0, 0, 0]
    assert dict(q.get(timeout=5) for _ in range(3)) == {0: True, 1: True, 2: True}
