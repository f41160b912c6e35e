"""-m gpu: the point, triangle-grid and MVT draws against the float64 reference of tests/backend_reference.py -- rasterisation written from
the reference's host code and shaders, sharing no formulation with the kernels, the oracle or tests/mvt_reference.py.

Every comparison holds the kernel AND the oracle (for MVT, the fp32 restatement of tests/mvt_reference.py) to the reference on the same
inputs, under the acceptance rule of tests/backend_cases.py, whose head holds the measured tolerances, margin bounds and excluded shares:
a failure says which of the two disagrees, where, and how close the reference itself was to deciding otherwise.
tests/test_backend_reference.py is the half of this that runs without a GPU.  All contexts go through the C ABI (rr.ReconIntegrationHip).
"""
import pytest

import backend_cases as C
from oracle.oracle import OracleRecon

pytestmark = pytest.mark.gpu


def pair(rr):
    def make(scene, mvt=False, **kw):
        return {"kernel": rr.ReconIntegrationHip(scene, **kw), "oracle": (C.MvtRestatement if mvt else OracleRecon)(scene, **kw)}
    return make


@pytest.mark.parametrize("name", list(C.TRIGRID_CASES))
def test_backend_trigrid(rr, name):
    C.trigrid_case(pair(rr), name)


@pytest.mark.parametrize("name", list(C.POINTS_CASES))
def test_backend_points(rr, name):
    C.points_case(pair(rr), name)


@pytest.mark.parametrize("name", list(C.MVT_CASES))
def test_backend_mvt(rr, name):
    C.mvt_case(pair(rr), name)


def test_backend_pixel_centres_on_an_edge(rr):
    """an exact grid: vertices and edges through pixel centres, in fp32 and float64 alike; inside the mesh such a centre is covered, by whichever triangle"""
    C.exact_case(pair(rr))
