"""-m gpu: integrate, the brick depth limits, the march launches and the shading against the float64 reference of
tests/main_path_reference.py -- arithmetic that shares no code, no precision and no formulation with the kernels or the oracle.

Every comparison holds the kernel AND the oracle to the reference on the same inputs, under the one acceptance rule of
tests/main_path_cases.py (its head holds the measured tolerances, margin bounds and excluded shares): a failure says which of the two
disagrees, where, and how close the reference itself was to deciding otherwise.  tests/test_main_path_reference.py is the half of this
that runs without a GPU.  All contexts go through the C ABI (rr.ReconIntegrationHip).
"""
import numpy as np
import pytest

import main_path_cases as C
from helpers import lut_box_class
from oracle.oracle import OracleRecon

pytestmark = pytest.mark.gpu


def pair(rr):
    return lambda scene, **kw: {"kernel": rr.ReconIntegrationHip(scene, **kw), "oracle": OracleRecon(scene, **kw)}


# RR_K1_FORM caps the integrate kernel's choice when a context is created (tests/test_gpu_coverage.py): the form that then runs at the LUT
# box class of (INT_RES, inverse LUT 24) = 1, and at class 2 (inverse LUT 16), where the separable record form exists
FORMS_CLASS1 = {"3": "lds_direct", "2": "lds_direct", "1": "lds_direct", "0": "generic"}     # (the cache and the separable passes need class 2)
FORMS_CLASS2 = {"3": "cached", "2": "record"}


def _form_env(monkeypatch, form):
    monkeypatch.setenv("RR_K1_FORM", form)
    if form == "3":
        monkeypatch.setenv("RR_PROJ_CACHE_MB", "64")           # the opt-in projection cache: k_integrate_cached


@pytest.mark.parametrize("use_bricks", [True, False], ids=["culled", "dense"])
@pytest.mark.parametrize("form", ["3", "2", "1", "0"])
def test_main_path_integrate_every_form(rr, form, use_bricks, monkeypatch):
    assert lut_box_class(C.INT_RES, (24,) * 3)[1] == 1
    _form_env(monkeypatch, form)
    _, objs = C.integrate_case(pair(rr), "base", use_bricks)
    f = objs["kernel"].integrate_form()
    assert f["form"] == FORMS_CLASS1[form] and f["culled"] == use_bricks


@pytest.mark.parametrize("use_bricks", [True, False], ids=["culled", "dense"])
@pytest.mark.parametrize("form", ["3", "2"])
def test_main_path_integrate_separable_forms(rr, form, use_bricks, monkeypatch):
    """the same shape under an inverse LUT of 16^3: class 2, the only class at which the record form and the projection cache run"""
    assert lut_box_class(C.INT_RES, (16,) * 3)[1] == 2
    _form_env(monkeypatch, form)
    _, objs = C.integrate_case(pair(rr), "class2", use_bricks)
    assert objs["kernel"].integrate_form()["form"] == FORMS_CLASS2[form]


@pytest.mark.parametrize("use_bricks", [True, False], ids=["culled", "dense"])
def test_main_path_integrate_class_0_runs_the_generic_kernel(rr, use_bricks):
    assert lut_box_class(C.INT_RES, (C.CLASS0_INV_RES,) * 3)[1] == 0
    _, objs = C.integrate_case(pair(rr), "class0", use_bricks)
    assert objs["kernel"].integrate_form()["form"] == "generic"


def test_main_path_integrate_second_frame_resets_emptied_tiles(rr):
    """a second frame with the objects elsewhere: tiles that held a surface and are empty now must hold -limit again"""
    first = C.integrate_reference("base")[0]
    second = C.integrate_reference("moved")[0]
    emptied = (np.abs(first) < C.F32_LIMIT) & (second == -C.F32_LIMIT)
    assert emptied.sum() > 500
    C.integrate_case(pair(rr), "base", True, moved=True)


@pytest.mark.parametrize("eye", ["far", "grazing", "in_brick", "axis"])
def test_main_path_depth_limits_eyes(rr, eye):
    C.peel_case(pair(rr), eye=eye)


@pytest.mark.parametrize("counters", ["ten_eleven", "last_row", "wrap"])
def test_main_path_depth_limits_hand_set_counters(rr, counters):
    C.peel_case(pair(rr), counters=counters)


def march_set(rr, monkeypatch):
    """gather march (RR_MARCH_BOX=0), the default box march and the two-box form (2), read when a context is created, and the oracle"""
    def make(scene, **kw):
        out = {}
        for name, env in (("kernel gather", "0"), ("kernel box", None), ("kernel box2", "2")):
            if env is None:
                monkeypatch.delenv("RR_MARCH_BOX", raising=False)
            else:
                monkeypatch.setenv("RR_MARCH_BOX", env)
            out[name] = rr.ReconIntegrationHip(scene, **kw)
        monkeypatch.delenv("RR_MARCH_BOX", raising=False)
        out["oracle"] = OracleRecon(scene, **kw)
        return out
    return make


@pytest.mark.parametrize("skip", [False, True], ids=["dense", "skipSpace"])
@pytest.mark.parametrize("kind", ["sphere", "slab"])
@pytest.mark.parametrize("res", C.MARCH_RES, ids=lambda r: "x".join(map(str, r)))
def test_main_path_march(rr, res, kind, skip, monkeypatch):
    C.march_case(march_set(rr, monkeypatch), kind, res, skip)


@pytest.mark.parametrize("mode", [0, 2, 3])
def test_main_path_shade(rr, mode):
    C.shade_case(pair(rr), mode)
