"""CPU: the numpy restatement of the streamed slab parts (tests/mesh_part_reference.py): the joined parts against mesh_compact_reference.encode of the
whole mesh, byte for byte, on the crafted cases of tests/test_gpu_mesh_slab.py."""
import functools

import numpy as np
import pytest

import mesh_compact_reference as MC
import mesh_pack_reference as P
import mesh_part_reference as MP
import mesh_slab_reference as S

BBOX = ((-1.0, 0.0, -1.0), (1.0, 2.2, 1.0))
LIMIT = 0.05
SEED = 20261019
# (rx, ry, rz), level, slabs: the six crafted cases of tests/test_gpu_mesh_slab.py -- 1-layer slabs and a partial top among them
CASES = [((32, 32, 32), 0, [(0, 16), (16, 32)]),
         ((32, 32, 32), 0, [(0, 8), (8, 16), (16, 24), (24, 32)]),
         ((20, 12, 28), 0, [(0, 8), (8, 24), (24, 28)]),
         ((24, 20, 64), 1, [(0, 32), (32, 64)]),
         ((24, 20, 64), 2, [(0, 32), (32, 64)]),
         ((24, 20, 64), 1, [(0, 16), (16, 64)])]


@functools.lru_cache(maxsize=None)
def _case(k):
    res, level, slabs = CASES[k]
    vol = S.crafted_volume(res, slabs, SEED, LIMIT)
    ref, parts = MP.parts(vol, LIMIT, *BBOX, level, slabs)
    return vol, ref, parts, MC.encode(ref, level, vol.shape)


@pytest.mark.parametrize("k", range(len(CASES)))
def test_joined_parts_are_the_whole_compact_frame(k):
    vol, ref, parts, (table, codes, tiles) = _case(k)
    v, t, c = MP.join(parts)
    assert len(codes) > 100 and len(table) > 1
    assert v.dtype == np.uint16 and v.tobytes() == P.pack(ref["unit"]).tobytes()
    assert t.dtype == MC.ROW and t.tobytes() == table.tobytes()
    assert c.dtype == np.uint16 and c.tobytes() == codes.tobytes()
    assert MC.decode(t, c, tiles).tobytes() == ref["triangles"].tobytes()
    per_layer = tiles[0] * tiles[1]
    for p in parts:                                                      # rows: owned tiles only, ids of the whole grid, bases part-local
        l0, l1 = p["layers"]
        assert ((p["table"]["tile"] >= l0 * per_layer) & (p["table"]["tile"] < l1 * per_layer)).all()
        assert not len(p["table"]) or (p["table"]["first_vertex"][0] == 0 and p["table"]["first_triangle"][0] == 0)
        assert p["table"]["n_triangles"].sum() == len(p["codes"]) and p["top"] == (p is parts[-1])


@pytest.mark.parametrize("k", range(len(CASES)))
def test_every_seam_is_crossed_by_a_code_with_bit_14(k):
    """not vacuous: below the top a part has codes with dz = 1 whose owner row lies in the next part, and it names rows it does not hold"""
    _, _, parts, _ = _case(k)
    for p in parts[:-1]:
        assert MP.seam_codes(p) > 0 and p["seam_tiles"] > 0
    assert MP.seam_codes(parts[-1]) == 0 and parts[-1]["seam_tiles"] == 0
    # only the top part decodes alone: a lower part's own table does not hold the rows its dz = 1 codes name (part 0's indices are the whole frame's)
    _, ref, _, _ = _case(k)
    low = parts[0]
    alone = MC.decode(low["table"], low["codes"], low["tiles"])
    assert (alone != ref["triangles"][:len(alone)]).any()
    top = parts[-1]
    first = sum(len(p["vertices"]) for p in parts[:-1])
    assert (MC.decode(top["table"], top["codes"], top["tiles"]).astype(np.int64) + first == ref["triangles"][len(ref["triangles"]) - len(top["codes"]):]).all()


@pytest.mark.parametrize("res,level", [((32, 32, 32), 0), ((20, 12, 28), 0), ((24, 20, 64), 1), ((24, 20, 64), 2)])
def test_the_one_slab_case_is_the_whole_frame(res, level):
    slabs = [(0, res[2])]
    vol = S.crafted_volume(res, [(0, 8)], SEED, LIMIT)                    # (specials planted around plane 8)
    ref, parts = MP.parts(vol, LIMIT, *BBOX, level, slabs)
    table, codes, tiles = MC.encode(ref, level, vol.shape)
    (p,) = parts
    assert p["top"] and p["layers"] == (0, tiles[2]) and p["seam_tiles"] == 0
    assert p["table"].tobytes() == table.tobytes() and p["codes"].tobytes() == codes.tobytes() and p["vertices"].tobytes() == P.pack(ref["unit"]).tobytes()
    v, t, c = MP.join(parts)
    assert t.tobytes() == table.tobytes() and c.tobytes() == codes.tobytes()


def empty_slab_volume():
    """(32, 32, 32) in four slabs, the third without a vertex: planes 16 .. 24 are outside everywhere"""
    slabs = [(0, 8), (8, 16), (16, 24), (24, 32)]
    vol = S.crafted_volume((32, 32, 32), slabs, SEED, LIMIT)
    vol[16:25] = -LIMIT
    return vol, slabs


def test_a_part_without_a_vertex_joins_cleanly():
    vol, slabs = empty_slab_volume()
    ref, parts = MP.parts(vol, LIMIT, *BBOX, 0, slabs)
    table, codes, tiles = MC.encode(ref, 0, vol.shape)
    assert len(parts[2]["vertices"]) == 0 and len(parts[2]["table"]) == 0 and len(parts[2]["codes"]) == 0
    assert all(len(parts[k]["vertices"]) > 0 for k in (0, 1, 3))
    v, t, c = MP.join(parts)
    assert t.tobytes() == table.tobytes() and c.tobytes() == codes.tobytes() and v.tobytes() == P.pack(ref["unit"]).tobytes()
    assert MP.payload_bytes(parts[2], 8) == 0


def test_join_refuses_an_overflowed_part_and_a_gap():
    _, _, parts, _ = _case(1)
    with pytest.raises(ValueError):
        MP.join([parts[0], dict(parts[1], overflow=4), parts[2], parts[3]])
    with pytest.raises(ValueError):
        MP.join([parts[0], parts[2]])
    with pytest.raises(ValueError):
        MP.join([])


def test_packed_attributes_are_sliced_with_the_vertices():
    res, level, slabs = CASES[2]
    vol = S.crafted_volume(res, slabs, SEED, LIMIT)
    ref, _ = S.split(vol, LIMIT, *BBOX, level, slabs)
    rng = np.random.default_rng(3)
    nrm = rng.normal(size=(len(ref["unit"]), 3)).astype(np.float32)
    _, parts = MP.parts(vol, LIMIT, *BBOX, level, slabs, normal=nrm)
    v, _, _ = MP.join(parts)
    assert v.shape[1] == 16 and v.tobytes() == P.pack(ref["unit"], nrm, None).tobytes()
    assert sum(MP.payload_bytes(p, 16) for p in parts) >= len(v) * 16


# ---- the slab driver over gloo, with stand-in backends that serve reference parts
class FakePartRing:
    """what SlabDriver.stream_mesh and mesh_parts_on_one_device use of a backend whose ring streams parts"""
    def __init__(self, res, part):
        self.res, self.part, self.queued = res, part, []

    def mesh_stream(self, tag=0):
        self.queued.append(tag)

    def mesh_stream_take(self, wait=True):
        p = self.part
        info = dict(n_vertices=len(p["vertices"]), n_triangles=len(p["codes"]), needed_vertices=len(p["vertices"]), needed_triangles=len(p["codes"]),
                    needed_tiles=len(p["table"]), tag=self.queued.pop(0), overflow=p["overflow"], vertex_stride=8, flags=0,
                    compact=dict(table=p["table"].copy(), tiles=p["tiles"], level=p["level"]),
                    part=dict(layers=p["layers"], level=p["level"], top=p["top"], seam_tiles=p["seam_tiles"]))
        return p["vertices"].copy(), p["codes"].copy(), info


def _same_as_whole(frame, ref, whole):
    table, codes, tiles = whole
    v, c, info = frame
    return (v.tobytes() == P.pack(ref["unit"]).tobytes() and c.tobytes() == codes.tobytes() and info["compact"]["table"].tobytes() == table.tobytes() and
            info["compact"]["tiles"] == tiles and (info["n_vertices"], info["n_triangles"]) == (len(v), len(c)))


def test_one_device_fallback_joins_reference_parts():
    from importlib import import_module
    mgpu = import_module("rgbd-recon_amd.multigpu")
    vol, ref, parts, whole = _case(2)
    backends = [FakePartRing(CASES[2][0], p) for p in parts]
    got, frame = mgpu.mesh_parts_on_one_device(backends, tag=5)
    assert [g[2]["tag"] for g in got] == [5, 5, 5] and _same_as_whole(frame, ref, whole)
    backends[1].part = dict(parts[1], overflow=1)
    assert mgpu.mesh_parts_on_one_device(backends)[1] is None             # dropped whole


def _stream_worker(rank, world, port, q, dedicated):
    import os
    from importlib import import_module
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mgpu = import_module("rgbd-recon_amd.multigpu")
        res, level, slabs = (20, 12, 28), 0, [(0, 8), (8, 28)]
        vol = S.crafted_volume(res, slabs, SEED, LIMIT)
        ref, parts = MP.parts(vol, LIMIT, *BBOX, level, slabs)
        part = parts[max(rank - 1, 0)] if dedicated else parts[rank]
        drv = mgpu.SlabDriver(FakePartRing(res, part), rank, world, "cpu", view=(8, 4), halo="recompute", compositor="dedicated" if dedicated else "shared")
        got = drv.stream_mesh(tag=9)
        ok = (got["part"] is None) if (dedicated and rank == 0) else (got["part"][2]["tag"] == 9 and got["part"][0].tobytes() == part["vertices"].tobytes())
        if rank == 0:
            ok &= _same_as_whole(got["frame"], ref, MC.encode(ref, level, vol.shape))
        else:
            ok &= "frame" not in got
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("world,dedicated", [(2, False), (3, True)])
def test_slab_driver_stream_mesh_gloo(world, dedicated):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_stream_worker, args=(r, world, port, q, dedicated)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
        assert p.exitcode == 0
    got = dict(q.get(timeout=5) for _ in range(world))
    assert got == {r: True for r in range(world)}
