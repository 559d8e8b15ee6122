"""CPU-side tests of the output stage (NA_BatchEnableOutputStage / SetStreamGain / GetStreamGain / Handover / HandoverRemaining): the
binding list, the header, db_to_gain, and what the calls do where there is no device.  Everything that runs is in
tests/test_gpu_handover.py."""
import math
import os
import re

import pytest

import na_oracle as O

STAGE = ["NA_BatchEnableOutputStage", "NA_BatchSetStreamGain", "NA_BatchGetStreamGain", "NA_BatchHandover", "NA_BatchHandoverRemaining"]


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    return neuralaudio_amd


def test_the_output_stage_is_bound_declared_and_exported(na):
    """The five calls are public: in capi.NA_SYMBOLS, declared outside the header's test-build block (so
    test_release_library_exports_the_documented_surface_and_nothing_else holds the release library to them) and exported by the
    library the tests load; Batch has methods of the same names."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    header = open(os.path.join(O.ROOT, "include", "neuralaudio_amd.h")).read()
    public = header.split("#ifndef NA_RELEASE")[0]
    declared = set(re.findall(r"NA_EXTERN[^;(]*?\b(NA_[A-Za-z0-9]+)\(", public))
    for name in STAGE:
        assert name in capi.NA_SYMBOLS and name in declared, name
        getattr(lib, name)
    for method in ("EnableOutputStage", "SetStreamGain", "GetStreamGain", "Handover", "HandoverRemaining"):
        assert callable(getattr(na.Batch, method))
    # the contract is in the header comment: the two formulas, word for word
    assert "g_a + (g_b - g_a) * ((min(k, R-1) + 1) / R)" in header and "w = (min(k, N-1) + 1) / N" in header
    assert "(1 - w) * (g_from * y_from) + w * (g_to * y_to)" in header


def test_db_to_gain(na):
    assert "db_to_gain" in na.__all__
    assert na.db_to_gain(0.0) == 1.0
    assert abs(na.db_to_gain(-6.0206) - 0.5) < 1e-6
    assert na.db_to_gain(float("-inf")) == 0.0
    assert abs(na.db_to_gain(20.0) - 10.0) < 1e-12 and abs(na.db_to_gain(-20.0) - 0.1) < 1e-12
    assert math.isclose(na.db_to_gain(6.0) * na.db_to_gain(-6.0), 1.0, rel_tol=1e-12)


def test_without_a_batch_the_calls_fail_loudly(na):
    """The stage lives in a batch and a batch needs a device: on the batch that does not exist every call fails
    with the library's "no HIP device" error instead of crashing."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    assert lib.NA_BatchEnableOutputStage(None) != 0
    assert "no HIP device" in capi.last_error()
    assert lib.NA_BatchSetStreamGain(None, 0, 0.5, 64) != 0
    assert "no HIP device" in capi.last_error()
    assert lib.NA_BatchHandover(None, 0, 1, 1.0, 64) != 0
    assert "no HIP device" in capi.last_error()
    assert lib.NA_BatchGetStreamGain(None, 0) < 0
    assert "no HIP device" in capi.last_error()
    assert lib.NA_BatchHandoverRemaining(None, 0) < 0
    assert "no HIP device" in capi.last_error()
