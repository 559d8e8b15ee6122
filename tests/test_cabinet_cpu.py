"""CPU-side tests of the cabinet stage (NA_BatchEnableCabinetStage / GetCabinetInfo / LoadIR / UnloadIR / SetStreamIR / GetStreamIR /
StreamIRFadeRemaining): the binding list, the header, what the calls do where there is no device, and the float64 contract the GPU
tests check against (tests/cabinet_cases.py) on a case worked out by hand.  Everything that runs on the device is in
tests/test_gpu_cabinet.py."""
import os
import re

import numpy as np
import pytest

import cabinet_cases as K
import na_oracle as O

STAGE = ["NA_BatchEnableCabinetStage", "NA_BatchGetCabinetInfo", "NA_BatchLoadIR", "NA_BatchUnloadIR", "NA_BatchSetStreamIR",
         "NA_BatchGetStreamIR", "NA_BatchStreamIRFadeRemaining"]
HOOKS = ["NA_DebugRunCabinetStage", "NA_DebugCabinetLaunches"]


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    return neuralaudio_amd


def test_the_cabinet_stage_is_bound_declared_and_exported(na):
    """The seven calls are public: in capi.NA_SYMBOLS, declared outside the header's test-build block (so
    test_release_library_exports_the_documented_surface_and_nothing_else holds the release library to them) and exported by the
    library the tests load; the two hooks are declared inside that block; Batch has the methods."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    header = open(os.path.join(O.ROOT, "include", "neuralaudio_amd.h")).read()
    public, hooks = header.split("#ifndef NA_RELEASE")[0], header.split("#ifndef NA_RELEASE")[1]
    declared = set(re.findall(r"NA_EXTERN[^;(]*?\b(NA_[A-Za-z0-9]+)\(", public))
    debug = set(re.findall(r"NA_EXTERN[^;(]*?\b(NA_[A-Za-z0-9]+)\(", hooks))
    for name in STAGE:
        assert name in capi.NA_SYMBOLS and name in declared, name
        getattr(lib, name)
    for name in HOOKS:
        assert name in capi.NA_SYMBOLS and name in debug and name not in declared, name
        getattr(lib, name)
    for method in ("EnableCabinetStage", "CabinetInfo", "LoadIR", "UnloadIR", "SetStreamIR", "GetStreamIR", "IRFadeRemaining"):
        assert callable(getattr(na.Batch, method))
    assert "typedef struct NA_CabinetInfo { int maxTaps, ringSamples, pieceSamples, numIRs; long long deviceBytes; } NA_CabinetInfo;" in public
    # the contract is in the header comment: the two formulas, word for word
    assert "c_h[t] = sum over k in [0, K) of h[k] * y[t - k]" in public
    assert "(1 - w) * c_A[t] + w * c_B[t]" in public and "w = (min(k, N-1) + 1) / N" in public
    assert "c_dry[t] = y[t]" in public
    fields = [name for name, _ in capi.NA_CabinetInfo._fields_]
    assert fields == ["maxTaps", "ringSamples", "pieceSamples", "numIRs", "deviceBytes"]


def test_without_a_batch_the_calls_fail_loudly(na):
    """The stage lives in a batch and a batch needs a device: on the batch that does not exist every call fails with the library's
    "no HIP device" error instead of crashing."""
    import ctypes as C
    from neuralaudio_amd import capi
    lib = capi.load_library()
    taps = np.ones(4, np.float32)
    info = capi.NA_CabinetInfo()
    calls = [(lambda: lib.NA_BatchEnableCabinetStage(None, 2048), lambda rc: rc != 0),
             (lambda: lib.NA_BatchGetCabinetInfo(None, C.byref(info)), lambda rc: rc != 0),
             (lambda: lib.NA_BatchLoadIR(None, taps.ctypes.data_as(C.POINTER(C.c_float)), 4), lambda rc: rc < 0),
             (lambda: lib.NA_BatchUnloadIR(None, 0), lambda rc: rc != 0),
             (lambda: lib.NA_BatchSetStreamIR(None, 0, 0, 64), lambda rc: rc != 0),
             (lambda: lib.NA_BatchGetStreamIR(None, 0), lambda rc: rc <= -2),
             (lambda: lib.NA_BatchStreamIRFadeRemaining(None, 0), lambda rc: rc < 0)]
    for call, failed in calls:
        assert failed(call())
        assert "no HIP device" in capi.last_error()


def test_the_float64_contract_on_a_case_worked_out_by_hand():
    """tests/cabinet_cases.py, which the GPU tests check against: a two-tap IR from T0, a fade to a delay, a fade to dry."""
    irs = {"a": np.array([1.0, 0.5], np.float32), "d": np.array([0.0, 1.0], np.float32)}
    c = K.CabContract(2, irs)
    y = np.array([[1, 2, 3, 4], [5, 6, 7, 8]], np.float32)
    e, b, exact = c.step(y)
    assert np.array_equal(e, y) and list(exact) == [True, True] and not np.any(b)
    c.set_ir(0, "a", 0)
    e, b, exact = c.step(y)
    assert list(e[0]) == [1.0, 2.5, 4.0, 5.5] and list(exact) == [False, True]  # y[t] = 0 in front of T0
    assert np.all(b[0] >= 6 * K.U * np.array([1.0, 2.5, 4.0, 5.5])) and np.all(b[0] < 1e-5)
    c.set_ir(0, "d", 2)  # w = 1/2, 1, 1, 1 on the same history
    e, _, _ = c.step(y)
    assert list(e[0]) == [0.5 * (1 + 2.0) + 0.5 * 4, 1.0, 2.0, 3.0] and c.remaining(0) == 0
    c.set_ir(0, None, 4)  # to dry: w = 1/4 .. 1, then the entry is gone
    e, _, exact = c.step(y)
    assert list(e[0]) == [0.75 * 4 + 0.25 * 1, 0.5 * 1 + 0.5 * 2, 0.25 * 2 + 0.75 * 3, 4.0] and c.state[0] is None
    assert list(c.step(y)[2]) == [True, True]
    # the sequential f32 sum agrees with float64 on integers, and the bound holds for it on floats
    rng = np.random.default_rng(1)
    h, x = K.integers(rng, 37, 4), K.integers(rng, 200, 8)
    assert np.array_equal(K.sequential_f32(h, x), K.conv64(h, x))
    h, x = rng.standard_normal(300).astype(np.float32), rng.standard_normal(500).astype(np.float32)
    assert np.all(np.abs(K.sequential_f32(h, x) - K.conv64(h, x)) <= K.conv_bound(h, x))
    w, v = K.weight32(3, np.arange(5))
    assert list(w) == [float(np.float32(1) / np.float32(3)), float(np.float32(2) / np.float32(3)), 1.0, 1.0, 1.0] and v[2] == 0.0
