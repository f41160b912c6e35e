"""CPU: the numpy restatement of the mesh components on Z-slab contexts (tests/mesh_slab_component_reference.py) against the whole reference mesh's
components; the library's host merge (tsdf_mesh_merge_component_seams: it needs no device) against its numpy twin and against the reference's merge,
byte for byte, through ctypes and as a stand-alone program under the host sanitizers; malformed lists; the figures that keep the GPU cases from
passing trivially; the slab driver's collective over gloo with stand-in backends; drop_mesh_components against mesh_component_reference.keep."""
import ctypes as C
import functools
import os
import socket
import struct
import subprocess
from importlib import import_module

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import mesh_component_reference as K
import mesh_slab_component_reference as R
import mesh_slab_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbd-recon_amd", "csrc")
BBOX, LIMIT, CASES = R.BBOX, R.LIMIT, R.CASES                            # kind, (rx, ry, rz), level, slabs: shared with tests/test_gpu_mesh_slab_components.py
IDS = ["%s-%dx%dx%d-L%d-%dslabs" % (k, *r, l, len(s)) for k, r, l, s in CASES]


@functools.lru_cache(maxsize=None)
def _case(i):
    kind, res, level, slabs = CASES[i]
    vol = R.case_volume(kind, res, slabs, LIMIT)
    ref, parts = S.split(vol, LIMIT, *BBOX, level, slabs)
    return ref, parts, R.components_of_parts(ref, parts, level)


def _lists(run):
    return [{k: lab[k] for k in ("vertex_base", "n_vertices", "n_local", "down", "up", "roots")} for lab in run["labs"]]


def _same_merge(a, b):
    assert a["component_base"] == b["component_base"] and a["n_components"] == b["n_components"]
    assert len(a["links"]) == len(b["links"])
    for x, y in zip(a["links"], b["links"]):
        assert x.dtype.itemsize == y.dtype.itemsize == 32 and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_joined_parts_equal_the_whole_mesh_components(i):
    ref, parts, run = _case(i)
    want = K.components(ref["triangles"], len(ref["position"]))
    assert len(want[2]) >= 1 and len(ref["triangles"]) > 100
    for got, w in zip(run["joined"], want):
        assert got.dtype == w.dtype and got.tobytes() == w.tobytes()
    # a part's rows are those of the representatives it owns, and its numbers continue those of the slabs below
    at = 0
    for k, (p, r) in enumerate(zip(parts, run["results"])):
        assert run["merged"]["component_base"][k] == at
        assert ((r[2]["first_vertex"] >= p["vertices"][0]) & (r[2]["first_vertex"] < p["vertices"][1])).all()
        at += len(r[2])
    assert at == run["merged"]["n_components"] == len(want[2])
    # the lists are sorted, and every triangle of every part has an own vertex
    for lab, p in zip(run["labs"], parts):
        for name, key in (("down", "vertex"), ("up", "vertex"), ("roots", "root")):
            assert (np.diff(lab[name][key].astype(np.int64)) > 0).all(), name
        tri = lab["triangles"]
        assert ((tri >= p["vertices"][0]) & (tri < p["vertices"][1])).any(axis=1).all()
        assert (lab["up"]["vertex"] >= p["vertices"][1]).all() and (lab["up"]["root"] < p["vertices"][1]).all()
    assert len(run["labs"][0]["down"]) == 0                               # slab_z0 == 0: nothing below


# what the issue's author measured: the cases are not vacuous
FIGURES = {0: dict(components=4, spanning3=4, local=[6, 8, 8, 6], removed=[2, 8, 8, 6], own_slab=2),
           1: dict(components=4, spanning=4, own_slab=2),
           2: dict(components=4, spanning=4, own_slab=2),
           3: dict(components=1227, spanning=229, spanning3=3, own_slab=34, up_records=2343),
           6: dict(components=165, spanning=8),
           7: dict(components=23, spanning=3),
           8: dict(components=4)}


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_cases_are_not_vacuous(i):
    kind, res, level, slabs = CASES[i]
    ref, parts, run = _case(i)
    f = R.figures(ref, parts, run)
    print(IDS[i], f)
    for key, value in FIGURES.get(i, {}).items():
        assert f[key] == value, (key, f[key], value)
    assert all(n >= 1 for n in f["per_seam"])                             # at least one component spans every seam
    if kind == "columns":
        assert f["own_slab"] >= 1                                         # roots merged into a root of their OWN slab: joined only through another slab
    if len(slabs) == 4:
        assert f["spanning3"] >= 1
    if len(slabs) > 1:
        assert f["up_records"] > 0 and sum(f["removed"]) > 0


def test_columns_are_lost_at_level_2():
    vol = R.columns_volume((24, 20, 64), LIMIT)
    ref, parts = S.split(vol, LIMIT, *BBOX, 2, [(0, 32), (32, 64)])
    assert len(K.components(ref["triangles"], len(ref["position"]))[2]) == 1   # two voxels thick: the 4-voxel lattice does not resolve them


# ---- the merge: reference, numpy twin, library
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_library_merge_equals_the_numpy_twin_and_the_reference(rr, i):
    ref, parts, run = _case(i)
    lists = _lists(run)
    twin = rr.merge_mesh_component_seams(lists)
    native = rr.merge_mesh_component_seams(lists, native=True)
    _same_merge(twin, native)
    _same_merge(twin, dict(run["merged"], links=[np.ascontiguousarray(l) for l in run["merged"]["links"]]))
    assert R.LINK == rr.MESH_COMPONENT_LINK_DTYPE and R.SEAM_ROOT == rr.MESH_SEAM_ROOT_DTYPE and R.SEAM_VERTEX == rr.MESH_SEAM_VERTEX_DTYPE


def _malformed(lists):
    """(what is wrong, the lists) for every refusal the header names"""
    def copy():
        return [dict(s, down=s["down"].copy(), up=s["up"].copy(), roots=s["roots"].copy()) for s in lists]
    out = []
    c = copy(); c[1]["down"] = c[1]["down"][c[1]["down"]["vertex"] != c[0]["up"]["vertex"][0]]; out.append(("an up record without its down record", c))
    c = copy(); c[-1]["up"] = c[0]["up"][:1].copy(); out.append(("an up record above the last slab", c))
    for name in ("down", "up", "roots"):
        k = 1 if name == "down" else 0
        c = copy(); c[k][name][[0, 1]] = c[k][name][[1, 0]]; out.append(("unsorted " + name, c))
    c = copy(); c[0]["up"] = np.concatenate([c[0]["up"][:1], c[0]["up"]]); out.append(("a repeated up record", c))
    c = copy(); c[1]["roots"]["root"][0] = c[0]["roots"]["root"][0]; out.append(("a root outside its slab (below)", c))
    c = copy(); c[0]["roots"]["root"][-1] = c[1]["vertex_base"]; out.append(("a root outside its slab (above)", c))
    c = copy(); c[0]["roots"]["rank"][-1] = c[0]["n_local"]; out.append(("a rank that is no local component", c))
    c = copy(); c[0]["up"]["root"][0] = c[0]["vertex_base"] + c[0]["n_vertices"] - 1; out.append(("a seam record whose root has no root record", c))
    c = copy(); c[1]["vertex_base"] -= 1; out.append(("slabs that overlap", c))
    return out


def test_malformed_lists_are_refused_and_nothing_is_written(rr):
    lists = _lists(_case(0)[2])
    assert len(lists[0]["up"]) > 2 and len(lists[1]["down"]) > 2 and len(lists[0]["roots"]) > 1
    assert lists[0]["vertex_base"] + lists[0]["n_vertices"] - 1 not in lists[0]["roots"]["root"]
    lib = rr.load_library()
    n_links = sum(len(s["roots"]) for s in lists)
    for what, bad in _malformed(lists):
        with pytest.raises(ValueError):
            rr.merge_mesh_component_seams(bad)
        with pytest.raises(rr.TsdfError) as e:
            rr.merge_mesh_component_seams(bad, native=True)
        assert e.value.code == -1, what
        arr, keep = rr.component_seams_struct(bad)
        base, links, n = np.full(len(bad), 77, np.uint64), np.full(n_links * 8, 7, np.uint32), C.c_uint64(777)
        rc = lib.tsdf_mesh_merge_component_seams(arr, C.c_uint32(len(bad)), base.ctypes.data_as(C.c_void_p), links.ctypes.data_as(C.c_void_p), C.byref(n))
        assert rc == -1 and (base == 77).all() and (links == 7).all() and n.value == 777, what
    # NULL arrays; no slab at all is the empty mesh
    arr, keep = rr.component_seams_struct(lists)
    assert lib.tsdf_mesh_merge_component_seams(None, C.c_uint32(4), None, None, None) == -1
    assert lib.tsdf_mesh_merge_component_seams(arr, C.c_uint32(len(lists)), None, None, None) == -1
    n = C.c_uint64(5)
    assert lib.tsdf_mesh_merge_component_seams(None, C.c_uint32(0), None, None, C.byref(n)) == 0 and n.value == 0
    assert rr.merge_mesh_component_seams([]) == dict(component_base=[], links=[], n_components=0)


def _pack_case(lists):
    out = [struct.pack("<I", len(lists))]
    for s in lists:
        out.append(struct.pack("<6Q", s["vertex_base"], s["n_vertices"], s["n_local"], len(s["down"]), len(s["up"]), len(s["roots"])))
        out += [np.ascontiguousarray(s[k]).tobytes() for k in ("down", "up", "roots")]
    return b"".join(out)


def test_merge_header_under_the_host_sanitizers(rr, tmp_path):
    """tests/cpp/mesh_cc_seams_main.cpp, compiled with the host sanitizers and run directly: the links of two cases equal the numpy twin's, a
    malformed case is refused with nothing written"""
    exe = str(tmp_path / "mesh_cc_seams_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "mesh_cc_seams_main.cpp"), "-o", exe])
    good = [_lists(_case(0)[2]), _lists(_case(3)[2])]
    bad = _malformed(good[0])[0][1]
    (tmp_path / "in.bin").write_bytes(struct.pack("<I", 3) + _pack_case(good[0]) + _pack_case(bad) + _pack_case(good[1]))
    p = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert p.returncode == 0 and "mesh cc seams ok" in p.stdout, p.stdout + p.stderr
    want = b""
    for lists in (good[0], None, good[1]):
        if lists is None:
            want += struct.pack("<i", 6)                                  # (mesh_cc_seams.hpp: an up record without its down record)
            continue
        m = rr.merge_mesh_component_seams(lists)
        want += struct.pack("<iQ", 0, m["n_components"]) + struct.pack("<%dQ" % len(lists), *m["component_base"]) + b"".join(l.tobytes() for l in m["links"])
        want += struct.pack("<%di" % len(lists), *([0] * len(lists)))
    assert (tmp_path / "out.bin").read_bytes() == want


# ---- drop_mesh_components: the joined mesh without some components, by tsdf_mesh_keep_components' rule
def test_drop_mesh_components_equals_the_reference_keep(rr):
    ref, parts, run = _case(3)
    mesh = dict(position=ref["position"], triangles=ref["triangles"])
    vc, tc, table = run["joined"]
    rng = np.random.default_rng(5)
    for keep in (table["n_triangles"] >= 20, rng.random(len(table)) < 0.5, np.zeros(len(table), bool), np.ones(len(table), bool)):
        got, want = rr.drop_mesh_components(mesh, vc, tc, keep), K.keep(mesh, keep)
        assert sorted(got) == sorted(want)
        for k in want:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k
    assert 0 < len(rr.drop_mesh_components(mesh, vc, tc, table["n_triangles"] >= 20)["position"]) < len(mesh["position"])


# ---- SlabDriver.mesh_components over gloo: stand-in backends that serve reference parts
class FakeComponentSlab:
    def __init__(self, res, ref, part, level):
        self.res, self.ref, self.part, self.level = res, ref, part, level
        self.u = self.tri = self.lab = self.result = None

    def extract_mesh_slab(self, normals=True, colours=True, level=0):
        self.u = S.unlinked(self.ref, self.part)
        (v0, v1), (t0, t1) = self.part["vertices"], self.part["triangles"]
        return v1 - v0, t1 - t0

    def mesh_slab_seam(self):
        return self.part["seam"].copy()

    def mesh_slab_link(self, vertex_base, above_seam=None):
        self.tri = S.link(self.u, vertex_base, above_seam)
        assert vertex_base == self.part["vertices"][0]

    def mesh_slab_download(self, normals=True, colours=True, triangles=True):
        v0, v1 = self.part["vertices"]
        return dict(position=self.ref["position"][v0:v1].copy(), triangles=self.tri)

    def mesh_slab_components(self):
        assert self.tri is not None
        self.lab = R.label_part(self.ref, self.part, self.level)
        return dict(local_components=self.lab["n_local"], down=len(self.lab["down"]), up=len(self.lab["up"]), roots=len(self.lab["roots"]))

    def mesh_slab_component_seam(self):
        return {k: self.lab[k].copy() for k in ("down", "up", "roots")}

    def mesh_slab_link_components(self, component_base, links):
        self.result = R.link(self.lab, component_base, links)
        return len(self.result[2])

    def mesh_slab_download_components(self):
        return dict(zip(("vertex_component", "triangle_component", "table"), self.result))


GLOO_CASE = ("columns", (24, 20, 28), 0)


def _gloo_parts(dedicated):
    kind, res, level = GLOO_CASE
    slabs = [(0, 16), (16, 28)] if dedicated else [(0, 8), (8, 28)]
    vol = R.case_volume(kind, res, slabs, LIMIT)
    ref, parts = S.split(vol, LIMIT, *BBOX, level, slabs)
    return res, level, ref, parts


def _worker(rank, world, port, q, dedicated):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mgpu = import_module("rgbd-recon_amd.multigpu")
        res, level, ref, parts = _gloo_parts(dedicated)
        part = parts[max(rank - 1, 0)] if dedicated else parts[rank]
        drv = mgpu.SlabDriver(FakeComponentSlab(res, ref, part, level), rank, world, "cpu", view=(8, 4), halo="recompute",
                              compositor="dedicated" if dedicated else "shared")
        drv.extract_mesh(normals=False, colours=False, level=level)
        got = drv.mesh_components()
        want = K.components(ref["triangles"], len(ref["position"]))
        ok = got["n_components"] == len(want[2]) == 4
        if dedicated and rank == 0:
            ok &= len(got["part"]["vertex_component"]) == 0 and len(got["part"]["table"]) == 0 and got["component_base"] == 0
        else:
            v0, v1 = part["vertices"]
            ok &= got["part"]["vertex_component"].tobytes() == want[0][v0:v1].tobytes()
        if rank == 0:
            c = got["components"]
            ok &= all(c[k].tobytes() == w.tobytes() and c[k].dtype == w.dtype for k, w in zip(("vertex_component", "triangle_component", "table"), want))
        else:
            ok &= "components" not in got
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
def test_slab_driver_mesh_components_gloo(world, dedicated):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, dedicated)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
        assert p.exitcode == 0
    got = dict(q.get(timeout=5) for _ in range(world))
    assert got == {r: True for r in range(world)}


def test_driver_refuses_components_before_an_extract():
    mgpu = import_module("rgbd-recon_amd.multigpu")
    res, level, ref, parts = _gloo_parts(False)
    drv = mgpu.SlabDriver(FakeComponentSlab(res, ref, parts[0], level), 0, 1, "cpu", view=(8, 4), halo="recompute")
    with pytest.raises(RuntimeError):
        drv.mesh_components()


def test_one_device_helper_joins_reference_parts():
    mgpu = import_module("rgbd-recon_amd.multigpu")
    kind, res, level, slabs = CASES[2]
    ref, parts, run = _case(2)
    backends = [FakeComponentSlab(res, ref, p, level) for p in parts]
    mgpu.mesh_slabs_on_one_device(backends, normals=False, colours=False, level=level)
    for native in (False, True):
        out = mgpu.mesh_components_on_one_device(backends, native=native)
        for k, w in zip(("vertex_component", "triangle_component", "table"), run["joined"]):
            assert out[k].tobytes() == w.tobytes() and out[k].dtype == w.dtype
        assert out["n_components"] == 4
