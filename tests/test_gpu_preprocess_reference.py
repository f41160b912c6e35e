"""-m gpu: the pre-processing kernels (k_pre_morph, k_pre_filter, k_pre_boundary, k_pre_normal, k_pre_quality, and k_pre_lab through
preprocessed(lab=True)) AND the oracle against the float64 reference of tests/preprocess_reference.py -- arithmetic that shares no code, no
precision, no tiling and no reading of the shaders with either.

Every pass is judged alone: the reference of pass k is fed the candidate's own product of pass k - 1.  The acceptance rule is compare() of
tests/main_path_cases.py; tests/preprocess_reference_cases.py holds the cases, the measured tolerances and margin bounds and what each pass
excludes.  A failure says whether the kernel, the oracle or both disagree, where, and how close the reference itself was to deciding
otherwise.  tests/test_preprocess_reference.py is the half that runs without a GPU (and the only one that runs `sensor`).

The range cells k_pre_quality writes beside the quality image have no download; tests/test_gpu_preprocess_shapes.py::test_raw_path_volume_is_exact
stays their only judge."""
import pytest

import preprocess_reference_cases as C
from oracle.oracle import OracleRecon

pytestmark = pytest.mark.gpu


def pair(rr):
    return lambda scene, **kw: {"kernel": rr.ReconIntegrationHip(scene, **kw), "oracle": OracleRecon(scene, **kw)}


@pytest.mark.parametrize("case", C.GPU_CASES, ids=C.case_id)
def test_passes_match_the_reference(rr, case):
    """tiny x the two flag sets, odd x all eight, edge_depths, compressed twice, saturated -- each as built and under the mirrored calibration"""
    res = C.run_case(pair(rr), *case)
    assert len(res) == 4
