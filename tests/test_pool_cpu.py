"""CPU-side tests of the stream pool (NA_BatchReserveStreams / NA_BatchActivateStream / NA_BatchParkStream): the binding list, the
header, and what the calls do where there is no device.  Everything that runs is in tests/test_gpu_pool.py."""
import os
import re

import pytest

import na_oracle as O

POOL = ["NA_BatchReserveStreams", "NA_BatchActivateStream", "NA_BatchParkStream", "NA_BatchIsParked", "NA_BatchFindParked", "NA_BatchNumParked"]


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    return neuralaudio_amd


def test_the_pool_is_bound_declared_and_exported(na):
    """The six calls are public: in capi.NA_SYMBOLS, declared outside the header's test-build block (so
    test_release_library_exports_the_documented_surface_and_nothing_else holds the release library to them) and exported by the
    library the tests load.  The resource counter is a test hook: inside the block."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    header = open(os.path.join(O.ROOT, "include", "neuralaudio_amd.h")).read()
    public, hooks = header.split("#ifndef NA_RELEASE")[0], header.split("#ifndef NA_RELEASE")[1].split("#endif /* NA_RELEASE */")[0]
    declared = set(re.findall(r"NA_EXTERN[^;(]*?\b(NA_[A-Za-z0-9]+)\(", public))
    for name in POOL:
        assert name in capi.NA_SYMBOLS and name in declared, name
        getattr(lib, name)
    assert "NA_DebugDeviceResourceCalls" in capi.NA_SYMBOLS and "NA_DebugDeviceResourceCalls" in hooks and "NA_DebugDeviceResourceCalls" not in declared
    assert lib.NA_DebugDeviceResourceCalls() >= 0
    for method in ("ReserveStreams", "ActivateStream", "ParkStream", "IsParked", "FindParked", "NumParked"):
        assert callable(getattr(na.Batch, method))


def test_without_a_batch_the_calls_fail_loudly(na):
    """A pool lives in a batch and a batch needs a device: where there is none NA_BatchCreate fails with the library's "no HIP device"
    error, and every pool call on the batch that does not exist fails (or answers "nothing") instead of crashing."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    m = na.NeuralModelLoader().CreateFromFile(os.path.join(O.MODELS_DIR, "BossLSTM-1x16.nam"), doPrewarm=False)
    assert m is not None
    assert lib.NA_BatchReserveStreams(None, m._h, 4, 1) < 0
    assert "no HIP device" in capi.last_error()
    assert lib.NA_BatchActivateStream(None, 0, 1.0) != 0
    assert "no HIP device" in capi.last_error()
    assert lib.NA_BatchParkStream(None, 0) != 0
    assert "no HIP device" in capi.last_error()
    assert lib.NA_BatchIsParked(None, 0) == 0 and lib.NA_BatchFindParked(None, m._h) == -1 and lib.NA_BatchNumParked(None) == -1
    if na.device_count() > 0:
        return  # (with a device: tests/test_gpu_pool.py)
    with pytest.raises(na.NeuralAudioError, match="no HIP device"):
        na.Batch(0)
