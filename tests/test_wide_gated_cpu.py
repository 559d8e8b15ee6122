"""Gated layer arrays wider than 16 channels on request (NeuralModelLoader.SetWaveNetWideGated) without a GPU: what loads, what is
refused, and which kernel a model is predicted to run on (csrc/wavenet_choice.h WaveNetKernelFor).  tests/test_gpu_wide_gated.py runs
the kernel, on the same cases."""
import math
import os

import pytest

import gated_cases as GC
import na_oracle as O
import neuralaudio_amd as na
import wide_cases as WC

WIDE = [GC.case("32-16", [32, 16], 3, GC.LONG, 31), GC.case("24", [24], 3, GC.LONG, 32), GC.case("17-k2", [17], 2, [1, 70], 33),
        GC.case("64-32", [64, 32], 3, [1, 200], 34), GC.case("64-k1", [64], 1, [1, 1], 35), GC.case("20-k5", [20], 5, [70, 1], 36),
        GC.case("gated-plain", [40, 20], 3, [1, 64], 37, gated=[True, False]), GC.case("plain-gated", [40, 20], 3, [1, 64], 38, gated=[False, True]),
        GC.case("48-leaky", [48], 3, [1, 64], 39, act=O.ACT_LEAKYRELU), GC.case("33-8-stdmath", [33, 8], 3, [1, 64], 40, std=True)]
KNOBS = [{}, {"NA_WN_KERNEL": "split"}, {"NA_WN_KERNEL": "generic"}, {"NA_WN_KERNEL": "frame"}]


def loader(wide=True, exact=False, std=False):
    ld = na.NeuralModelLoader()
    ld.SetWaveNetWideGated(wide)
    ld.SetWaveNetExactF32(exact)
    if std:
        ld.SetWaveNetMathMode(na.EMathMode.StdMath)
    return ld


def load(ld, case, prewarm=False):
    return ld.CreateFromString(GC.nam_json(case["arrays"], GC.weights(case)), ".nam", doPrewarm=prewarm)


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact-f32"])
@pytest.mark.parametrize("case", WIDE, ids=[c["name"] for c in WIDE])
def test_wide_gated_models_load_on_the_wide_f32_family_whatever_the_knobs(case, exact):
    m = load(loader(exact=exact, std=case["std"]), case)
    assert m.IsGated()
    info = m.KernelInfo(1.0, 1)
    assert info["kernel"] == "wide-f32" and math.isinf(info["input_limit"]) and info["pack"] == 1, info
    for knobs in KNOBS:
        k = na.wavenet_kernel(m, streams=600, knobs=knobs)
        assert (k["family"], k["kernel_name"], k["pack"], k["virtual"]) == ("wide-f32", "WaveNetWideF32Kernel", 1, False) and math.isinf(k["input_limit"]), (knobs, k)


@pytest.mark.parametrize("gated", [[True], [False, True]], ids=["gated-80", "plain-80-beside-gated"])
def test_beyond_64_channels_is_refused_with_the_limit(gated):
    c = GC.case("80", [80, 8][:len(gated)], 3, [1, 2], 1, gated=gated)
    with pytest.raises(na.NeuralAudioError, match="layer array 0: 80 channels.*gated.*at most 64 channels"):
        load(loader(), c)


def test_without_the_option_the_same_file_is_refused_and_other_models_are_what_they_were():
    wide = GC.case("wide", [20], 3, [1, 2], 1)
    with pytest.raises(na.NeuralAudioError, match="layer array 0: gated layers at 20 channels.*at most 16 channels"):
        load(loader(wide=False), wide)
    assert na.wavenet_kernel(load(loader(), wide))["family"] == "wide-f32"
    narrow = na.wavenet_kernel(load(loader(), GC.CASES[0]), streams=600, knobs={"NA_WN_KERNEL": "split"})
    assert (narrow["family"], narrow["kernel_name"]) == ("frame", "WaveNetFrameKernel"), narrow
    arrays = WC.chain([32], [([3, 3], [1, 64])])
    text = O.nam_json_wavenet_generic(arrays, O.synth_wavenet_weights(arrays, seed=32))
    plain = [na.wavenet_kernel(ld.CreateFromString(text, ".nam", doPrewarm=False), streams=600) for ld in (loader(), loader(wide=False))]
    assert plain[0] == plain[1] and plain[0]["family"] == "generic", plain
    std = os.path.join(O.MODELS_DIR, "BossWN-standard.nam")
    assert na.wavenet_kernel(loader().CreateFromFile(std, doPrewarm=False), streams=600)["family"] == "f16-split"
