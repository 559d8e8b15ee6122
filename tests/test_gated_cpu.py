"""Gated WaveNet layer arrays (A1 key "gated") without a GPU: loading, the kernel family they are predicted to run on, the refusals, and
the condition that gives the GPU parity bound of tests/test_gpu_gated.py its meaning (tests/gated_cases.py has the contract)."""
import numpy as np
import pytest

import gated_cases as GC
import na_oracle as O
import neuralaudio_amd as na


def _load(c, w=None):
    return na.NeuralModelLoader().CreateFromString(GC.nam_json(c["arrays"], GC.weights(c) if w is None else w), ".nam", doPrewarm=False)


def test_a_gated_two_array_file_loads_and_is_predicted_on_the_frame_family_whatever_the_knob():
    m = _load(GC.CASES[0])
    assert m is not None and m.IsGated() and not m.IsStatic() and m.GetReceptiveFieldSize() == 2 * 2 * sum(GC.LONG)
    info = m.KernelInfo(streams=600)
    assert info["kernel"] == "frame" and info["pack"] == 1 and not info["range_proven"]
    for knobs in ({}, {"NA_WN_KERNEL": "split"}, {"NA_WN_KERNEL": "generic"}):
        k = na.wavenet_kernel(m, streams=600, knobs=knobs)
        assert (k["family"], k["kernel_name"], k["pack"], k["virtual"]) == ("frame", "WaveNetFrameKernel", 1, False), knobs
    assert not _load(GC.case("plain", [16, 8], 3, GC.LONG, 1, gated=[False, False])).IsGated()


@pytest.mark.parametrize("what,case,match", [
    ("the plain weight count under gated: true", None, "Wrong number of weights"),
    ("a 20-channel gated array", GC.case("wide", [20], 3, [1, 2], 1), "layer array 0: gated layers at 20 channels.*at most 16 channels"),
    ("a plain 32-channel array behind a gated one", GC.case("mixed-wide", [8, 32], 3, [1, 2], 1, gated=[True, False]),
     "layer array 0: 32 channels .*in a model with gated layer arrays.*at most 16 channels"),
    ("the kernel size beyond the largest", GC.case("k36", [16], GC.MAX_K16 + 1, [1], 1),
     "layer 0: kernel size 36 at 16 gated channels.*largest kernel size at this width is 35")])
def test_files_the_gated_path_cannot_run_are_refused_at_load(what, case, match):
    w = None
    if case is None:
        case, plain = GC.CASES[0], GC.case("plain", [16, 8], 3, GC.LONG, 1, gated=[False, False])
        w = GC.weights(plain)
    with pytest.raises(na.NeuralAudioError, match=match):
        _load(case, w)


def test_the_largest_gated_kernel_size_loads():
    assert _load(GC.case("k35", [16], GC.MAX_K16, [1], 1)).IsGated()


@pytest.mark.parametrize("case", GC.CASES, ids=[c["name"] for c in GC.CASES])
def test_the_float32_restatement_stays_within_half_the_gpu_bound_of_the_float64_one(case):
    w, x = GC.weights(case), O.signal_noise(GC.SAMPLES, seed=case["seed"])
    y64, y32 = (GC.forward(case["arrays"], w, x, dt, case["std"]) for dt in (np.float64, np.float32))
    assert y32.dtype == np.float32 and O.rms(y64) > 1e-5, O.rms(y64)  # (a silent model cannot pass)
    worst = GC.worst_window(y32.astype(np.float64), y64)
    print("%s: float32 restatement at %.3g of the GPU bound, level %.3g" % (case["name"], worst, O.rms(y64)))
    assert worst < 0.5, worst
