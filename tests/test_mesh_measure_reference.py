"""CPU: tests/mesh_measure_reference.py -- the signs and the order of the nested shells' volumes, the integer measures against float64 sums over the
fp32 positions inside a bound derived per component, the wide (> 64-bit) path on a coarse lattice, csrc/mesh_measure.hpp under the host sanitizers
against Python integers, and the three records' layout in C, ctypes and numpy."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import mesh_component_reference as K
import mesh_measure_reference as R
import mesh_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbd-recon_amd", "csrc")
BBOX = (np.array([-1.0, 0.0, -1.0], np.float32), np.array([1.0, 2.2, 1.0], np.float32))   # the default box: E = 2.2 m


@pytest.fixture(scope="module")
def grid():
    return R.grid(*BBOX)


@pytest.fixture(scope="module")
def cases(grid):
    """name -> (mesh, vertex_component, triangle_component, table, rows), computed once"""
    vols = dict(A=K.speckle_volume(), B=K.random_volume(), C=K.snakes_volume(), D=K.shells_volume(), S=R.random_small_volume())
    out = {}
    for name, vol in vols.items():
        mesh = M.extract(vol, K.LIMIT, *BBOX)
        vc, tc, table = K.components(mesh["triangles"], len(mesh["position"]))
        out[name] = (mesh, vc, tc, table, R.measures(mesh, vc, tc, len(table), grid))
    return out


def test_grid_is_isotropic_and_2_to_the_20_units_along_the_longest_edge(grid):
    assert grid["bits"] == 20 and grid["origin"].dtype == np.float32 and grid["origin"].tolist() == [-1.0, 0.0, -1.0]
    e = float(np.float32(2.2) - np.float32(0.0))
    assert grid["scale"] == 1048576.0 / e and grid["unit"] == 1.0 / grid["scale"]
    assert 2.0e-6 < grid["unit"] < 2.2e-6                                 # about 2.1 um
    q = R.quantise(np.array([[-1.0, 0.0, -1.0], [1.0, 2.2, 1.0], [np.nan, -5.0, 9.0], [np.inf, -np.inf, 0.0]], np.float32), grid)
    assert q[0].tolist() == [0, 0, 0] and q[1][1] == R.QMAX and q[1][0] == q[1][2] == round(2.0 * grid["scale"])
    assert q[2].tolist() == [0, 0, R.QMAX] and q[3][:2].tolist() == [R.QMAX, 0]
    assert (R.unpack(R.pack(q)) == q).all() and R.pack(q).dtype == np.uint64
    # half-way cases go to even: a grid of 2^19 units per metre, positions (k + 0.5) / 2^19
    g2 = dict(scale=524288.0, unit=1.0 / 524288.0, origin=np.zeros(3, np.float32), bits=20)
    half = (np.arange(6, dtype=np.float64)[:, None] + 0.5) / 524288.0 * np.ones(3)
    assert R.quantise(half.astype(np.float32), g2)[:, 0].tolist() == [0, 2, 2, 4, 4, 6]


def test_shells_have_the_signs_of_matter_void_matter(cases, grid):
    """(a) D: a ball inside a hollow shell.  Normals point into empty space: the shell's outer surface and the ball enclose matter (positive), the
    cavity's wall encloses a void (negative); |volume6| is ordered outer > cavity > ball."""
    _, _, _, table, rows = cases["D"]
    vol = R.volume6(rows)
    si = R.si(rows, grid)
    print("D: volumes", si["volume"].tolist(), "m^3, areas", si["area"].tolist(), "m^2")
    assert len(table) == 3 and vol[0] > 0 and vol[1] < 0 and vol[2] > 0
    assert abs(vol[0]) > abs(vol[1]) > abs(vol[2])
    assert rows["area2"][0] > rows["area2"][1] > rows["area2"][2] > 0
    assert (rows["reserved"] == 0).all() and (rows["q_min"] <= rows["q_max"]).all()
    # the three surfaces are concentric: nested bounds, one centroid
    assert (rows["q_min"][0] < rows["q_min"][1]).all() and (rows["q_min"][1] < rows["q_min"][2]).all()
    assert (rows["q_max"][0] > rows["q_max"][1]).all() and (rows["q_max"][1] > rows["q_max"][2]).all()
    centre = rows["sum_q"] / table["n_vertices"][:, None] * grid["unit"] + grid["origin"]
    assert np.abs(centre - [0.0, 1.1, 0.0]).max() < 0.02


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_integer_measures_agree_with_float64_sums_inside_the_derived_bound(cases, grid, name):
    """(b) The float64 side: P = (p - origin) * scale unrounded, area = sum |e1 x e2| / 2, volume6 = sum det(P0, P1, P2), in grid units.  The bound, per
    triangle and summed per component: rounding moves every vertex by at most d = sqrt(3) / 2 units, so
      area:  d * perimeter / 2 + 2 d^2, plus 1/2 for rounding the doubled area down to a whole unit^2;
      det:   d (|b x c| + |a x c| + |a x b|) + d^2 (|a| + |b| + |c|) + d^3.
    To both comes the float64 side's own rounding, 64 eps times the magnitudes that are summed (a few operations per term, each of relative error eps)."""
    mesh, vc, tc, table, rows = cases[name]
    P = (mesh["position"].astype(np.float64) - grid["origin"].astype(np.float64)) * grid["scale"]
    a, b, c = (P[mesh["triangles"][:, k]] for k in range(3))
    d, eps = math.sqrt(3.0) / 2.0, np.finfo(np.float64).eps
    norm = lambda x: np.sqrt((x * x).sum(axis=1))
    cross = np.cross(b - a, c - a)
    area = norm(cross) / 2.0
    perimeter = norm(b - a) + norm(c - b) + norm(a - c)
    area_bound = d * perimeter / 2.0 + 2.0 * d * d + 0.5 + 64.0 * eps * (norm(b - a) * norm(c - a) + area)
    bc, ac, ab = np.cross(b, c), np.cross(a, c), np.cross(a, b)
    det = (a * bc).sum(axis=1)
    det_bound = d * (norm(bc) + norm(ac) + norm(ab)) + d * d * (norm(a) + norm(b) + norm(c)) + d ** 3 + 64.0 * eps * norm(a) * norm(b) * norm(c)
    n = len(table)
    sums = [np.bincount(tc, weights=w, minlength=n) for w in (area, area_bound, det, det_bound)]
    vol = R.volume6(rows)
    worst = 0.0
    for comp in range(n):
        got_area, got_vol = int(rows["area2"][comp]) / 2.0, float(vol[comp])
        assert abs(got_area - sums[0][comp]) <= sums[1][comp], (name, comp, got_area, sums[0][comp], sums[1][comp])
        assert abs(got_vol - sums[2][comp]) <= sums[3][comp], (name, comp, got_vol, sums[2][comp], sums[3][comp])
        if sums[0][comp] > 0:
            worst = max(worst, abs(got_area - sums[0][comp]) / sums[0][comp])
    print(name, "worst relative area error", worst, "of", n, "components")
    assert worst < 1e-3                                                   # (the bound is the check; this only says the bound is not vacuous)


def test_the_coarse_lattice_needs_more_than_64_bits(cases, grid):
    """(c) On the 4 x 4 x 4 volume in the default box a triangle's |e1 x e2|^2 passes 2^64: the two-limb path is exercised, not assumed"""
    mesh = cases["S"][0]
    n2, a2, _ = R.triangle_measures(R.quantise(mesh["position"], grid), mesh["triangles"])
    print("4 x 4 x 4:", len(n2), "triangles, largest n2 has", max(n2).bit_length(), "bits")
    assert max(n2) >= 1 << 64 and max(n2) < 1 << 88
    assert all(a * a <= n < (a + 1) * (a + 1) for a, n in zip(a2, n2))


def _hand_made():
    """packed triangles [R, 3] uint64 that strain the arithmetic.  The header's bounds (n2 < 2^88, |v6| < 2^63) are generous: with coordinates in
    [0, 2^20] the corners of the cube give the largest values there are, n2 = 3 * 2^80 and v6 = +-2^61; _beyond_the_grid goes nearer the bounds."""
    m = R.QMAX
    corners = [(x, y, z) for x in (0, m) for y in (0, m) for z in (0, m)]
    tris = [(p, q, r) for p in corners for q in corners for r in corners]          # the largest n2 and |v6| the grid allows, and every degenerate form
    for a, b in ((m, m), (m - 1, m - 3), (3, 5), (1, 1), (m, 1), (65536, 65537)):
        tris.append(((0, 0, 0), (a, 0, 0), (0, b, 0)))                     # n2 = (a b)^2: a perfect square, up to 2^80
        tris.append(((7, 9, 11), (7 + a, 9, 11), (7, 9, 11 + b)))
    for s in (1, 2, 3, 1000, 46341, 65536, m - 1, m):
        tris.append(((0, 0, 1), (s, 0, 0), (0, s, 0)))                     # e1 x e2 = (s, s, s^2): n2 = (s^2 + 1)^2 - 1, one below a square
    tris.append(((5, 5, 5), (5, 5, 5), (5, 5, 5)))                         # a point
    tris.append(((1, 2, 3), (2, 4, 6), (3, 6, 9)))                         # collinear
    rng = np.random.default_rng(5)
    tris += [tuple(map(tuple, t)) for t in rng.integers(0, m + 1, (1500, 3, 3)).tolist()]
    tris += _beyond_the_grid()
    q = np.array(tris, np.int64)
    return R.pack(q.reshape(-1, 3)).reshape(-1, 3)


def _beyond_the_grid():
    """Raw packed words hold 21 bits a coordinate, up to w = 2^21 - 1: twice what a clamped vertex has.  No mesh gives such a word; the arithmetic is held
    to its stated bounds with them all the same: n2 = 3 w^4, just under 2^86, and v6 = +-w^3, just under 2^63.  The corners of that cube, minus the
    triples whose determinant -- or a partial sum of it, in measure_det's order -- leaves 64 bits (2 w^3 does)."""
    w = (1 << 21) - 1
    corners = [(x, y, z) for x in (0, w) for y in (0, w) for z in (0, w)]
    fits = lambda v: -(1 << 63) <= v < 1 << 63
    out = []
    for p in corners:
        for q in corners:
            for r in corners:
                c = (q[1] * r[2] - q[2] * r[1], q[2] * r[0] - q[0] * r[2], q[0] * r[1] - q[1] * r[0])
                if fits(p[0] * c[0] + p[1] * c[1]) and fits(p[0] * c[0] + p[1] * c[1] + p[2] * c[2]):
                    out.append((p, q, r))
    out.append(((0, 0, 0), (w, 0, 0), (0, w, 0)))                          # n2 = (w^2)^2, a perfect square under 2^84
    out.append(((0, 0, 1), (w, 0, 0), (0, w, 0)))                          # n2 = (w^2 + 1)^2 - 1
    return out


def _run_program(exe, tmp_path, tag, g, position, triangles, raw):
    position, triangles = np.ascontiguousarray(position, np.float32).reshape(-1, 3), np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    blob = g["origin"].astype("<f4").tobytes() + struct.pack("<d", g["scale"]) + struct.pack("<III", len(position), len(triangles), len(raw))
    (tmp_path / f"{tag}.in").write_bytes(blob + position.tobytes() + triangles.tobytes() + np.ascontiguousarray(raw, np.uint64).tobytes())
    p = subprocess.run([exe, str(tmp_path / f"{tag}.in"), str(tmp_path / f"{tag}.out")], capture_output=True, text=True)
    assert p.returncode == 0 and "mesh measure ok" in p.stdout, p.stdout + p.stderr
    out = (tmp_path / f"{tag}.out").read_bytes()
    nv, nt, nr = len(position), len(triangles), len(raw)
    assert len(out) == 8 * nv + 16 * (nt + nr) + 32
    packed = np.frombuffer(out, "<u8", nv)
    per = np.frombuffer(out, np.dtype([("a2", "<u8"), ("v6", "<i8")]), nt + nr, 8 * nv)
    sums = np.frombuffer(out, np.dtype([("lo", "<u8"), ("hi", "<i8")]), 2, 8 * nv + 16 * (nt + nr))
    return packed, per[:nt], per[nt:], sums


def _same(per, a2, v6, total):
    assert per["a2"].tolist() == a2 and per["v6"].tolist() == v6
    assert int(total["hi"]) * (1 << 64) + int(total["lo"]) == sum(v6)


def test_the_header_under_the_host_sanitizers_equals_python_integers(cases, grid, tmp_path):
    """(d) tests/cpp/mesh_measure_main.cpp, compiled with the host sanitizers and run directly"""
    exe = str(tmp_path / "mesh_measure_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "mesh_measure_main.cpp"), "-o", exe])
    raw = _hand_made()
    n2, a2, v6 = R.triangle_measures(R.unpack(raw.reshape(-1)), np.arange(raw.size).reshape(-1, 3))
    print("hand-made:", len(raw), "triangles, n2 up to", max(n2).bit_length(), "bits, |v6| up to", max(abs(v) for v in v6).bit_length(), "bits")
    w = (1 << 21) - 1
    assert max(n2) == 3 * w ** 4 > 1 << 85 and max(v6) == w ** 3 > 1 << 62 and min(v6) == -w ** 3 and 0 in n2
    assert 3 << 80 in n2 and 2 << 60 in v6 and -(2 << 60) in v6         # ... and the largest a clamped grid gives
    assert any(math.isqrt(n) ** 2 == n and n > 1 << 83 for n in n2) and any(math.isqrt(n + 1) ** 2 == n + 1 and n > 1 << 83 for n in n2)
    assert any(math.isqrt(n) ** 2 == n and 1 << 79 < n < 1 << 81 for n in n2) and any(math.isqrt(n + 1) ** 2 == n + 1 and 1 << 79 < n < 1 << 81 for n in n2)
    # the coarse lattice's mesh (the wide path on extracted data) with a few vertices no extract produces, and the speckle
    mesh = cases["S"][0]
    odd = np.array([[np.nan, 0.5, 0.5], [np.inf, -np.inf, 0.0], [-3.0, 9.0, 0.99999994], [1.0, 2.2, 1.0], [-1.0, 0.0, -1.0]], np.float32)
    position = np.concatenate([mesh["position"], odd])
    nv = len(mesh["position"])
    triangles = np.concatenate([mesh["triangles"], np.array([[nv, nv + 1, nv + 2], [nv + 3, nv + 4, 0], [nv + 2, 1, nv + 3]], np.uint32)])
    packed, per, hand, sums = _run_program(exe, tmp_path, "small", grid, position, triangles, raw)
    q = R.quantise(position, grid)
    assert packed.tobytes() == R.pack(q).tobytes()
    _same(per, *R.triangle_measures(q, triangles)[1:], sums[0])
    _same(hand, a2, v6, sums[1])
    mesh = cases["A"][0]
    packed, per, _, sums = _run_program(exe, tmp_path, "speckle", grid, mesh["position"], mesh["triangles"], raw[:0])
    q = R.quantise(mesh["position"], grid)
    assert packed.tobytes() == R.pack(q).tobytes()
    _same(per, *R.triangle_measures(q, mesh["triangles"])[1:], sums[0])
    # half-way cases, to even
    g2 = dict(scale=524288.0, unit=1.0 / 524288.0, origin=np.zeros(3, np.float32), bits=20)
    half = ((np.arange(300, dtype=np.float64)[:, None] + 0.5) / 524288.0 * np.ones(3)).astype(np.float32)
    packed, _, _, _ = _run_program(exe, tmp_path, "half", g2, half, np.zeros((0, 3), np.uint32), raw[:0])
    assert packed.tobytes() == R.pack(R.quantise(half, g2)).tobytes() and (R.unpack(packed)[:, 0] % 2 == 0).all()


class _Measure(C.Structure):
    _fields_ = [("q_min", C.c_uint32 * 3), ("q_max", C.c_uint32 * 3), ("area2", C.c_uint64), ("volume6_lo", C.c_uint64), ("volume6_hi", C.c_int64),
                ("sum_q", C.c_uint64 * 3), ("reserved", C.c_uint64)]


class _Grid(C.Structure):
    _fields_ = [("unit", C.c_double), ("origin", C.c_float * 3), ("bits", C.c_uint32)]


class _Rule(C.Structure):
    _fields_ = [("min_triangles", C.c_uint32), ("min_extent", C.c_uint32), ("min_area2", C.c_uint64), ("min_abs_volume6", C.c_uint64), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


def test_the_three_records_have_one_layout_in_c_ctypes_and_numpy(rr, tmp_path):
    """(e) 80 / 24 / 32 bytes, the same offsets everywhere"""
    recs = [("tsdf_mesh_component_measure", _Measure, (rr.MESH_COMPONENT_MEASURE_DTYPE, R.ROW), 80),
            ("tsdf_mesh_measure_grid", _Grid, (rr.MESH_MEASURE_GRID_DTYPE, R.GRID), 24), ("tsdf_mesh_measure_rule", _Rule, (rr.MESH_MEASURE_RULE_DTYPE, R.RULE), 32)]
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "rgbd_recon_hip.h"', 'int main(void) {']
    for cname, ct, _, size in recs:
        lines.append(f'  _Static_assert(sizeof({cname}) == {size}, "{size} bytes");')
        lines.append(f'  printf("%zu", sizeof({cname}));')
        for field, _ in ct._fields_:
            lines.append(f'  printf(" %zu", offsetof({cname}, {field}));')
        lines.append('  printf("\\n");')
    lines += ['  return 0;', '}', '']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [[int(v) for v in line.split()] for line in subprocess.check_output([exe], text=True).splitlines()]
    assert [g[0] for g in got] == [80, 24, 32]
    assert got[0][1:] == [0, 12, 24, 32, 40, 48, 72]
    for (cname, ct, dtypes, size), line in zip(recs, got):
        names = [f for f, _ in ct._fields_]
        assert C.sizeof(ct) == size and [getattr(ct, f).offset for f in names] == line[1:], cname
        for dt in dtypes:
            assert dt.itemsize == size and list(dt.names) == names and [dt.fields[f][1] for f in names] == line[1:], cname
    assert rr.MESH_RULE_POSITIVE_VOLUME == R.RULE_POSITIVE_VOLUME == 1
    assert "#define TSDF_MESH_RULE_POSITIVE_VOLUME 1u" in open(rr.HEADER_PATH).read()


def test_keep_flags_follow_every_clause(cases, grid):
    """the rule on A and D: an area threshold is not a triangle threshold; a void has no positive volume; an all-zero rule keeps everything"""
    _, _, _, table, rows = cases["A"]
    zero = dict(min_triangles=0, min_extent=0, min_area2=0, min_abs_volume6=0, flags=0, reserved=0)
    assert R.keep_flags(rows, table, zero).all()
    by_area = R.keep_flags(rows, table, dict(zero, min_area2=math.ceil(2 * 0.05 / grid["unit"] ** 2)))
    by_count = R.keep_flags(rows, table, dict(zero, min_triangles=100))
    print("A: kept by area", int(by_area.sum()), "by count", int(by_count.sum()), "of", len(table))
    assert 0 < by_count.sum() < by_area.sum() < len(table) and (by_count == (table["n_triangles"] >= 100)).all()
    assert (by_area == (rows["area2"] * grid["unit"] ** 2 / 2 >= 0.05 - 1e-9)).all()
    extent = (rows["q_max"].astype(np.int64) - rows["q_min"]).max(axis=1)
    assert (R.keep_flags(rows, table, dict(zero, min_extent=int(np.median(extent)))) == (extent >= int(np.median(extent)))).all()
    _, _, _, table, rows = cases["D"]
    assert R.keep_flags(rows, table, dict(zero, flags=R.RULE_POSITIVE_VOLUME)).tolist() == [True, False, True]
    vol = [abs(v) for v in R.volume6(rows)]
    assert R.keep_flags(rows, table, dict(zero, min_abs_volume6=vol[1])).tolist() == [True, True, False]
    assert R.keep_flags(rows, table, dict(zero, min_abs_volume6=vol[1] + 1)).tolist() == [True, False, False]
