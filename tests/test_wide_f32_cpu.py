"""Exact f32 on request (NeuralModelLoader.SetWaveNetExactF32) without a GPU: what loads, and which kernel family a model is predicted
to run on (csrc/wavenet_choice.h WaveNetKernelFor).  tests/test_gpu_wide_f32.py runs the kernel."""
import math
import os

import pytest

import gated_cases as GC
import na_oracle as O
import neuralaudio_amd as na
import wide_cases as WC


def _loader(exact):
    loader = na.NeuralModelLoader()
    loader.SetWaveNetExactF32(exact)
    return loader


@pytest.mark.parametrize("scaling", list(WC.WEIGHT_SCALINGS))
@pytest.mark.parametrize("name", ["32/8 tanh", "80/72 tanh"])
def test_weights_the_default_loader_refuses_load_on_the_f32_family(name, scaling):
    arrays, w = WC.range_model(name)
    text = O.nam_json_wavenet_generic(arrays, O.scale_wavenet_tensors(arrays, w, WC.WEIGHT_SCALINGS[scaling]))
    m = _loader(True).CreateFromString(text, ".nam", doPrewarm=False)
    info = m.KernelInfo(1.0, 1)
    assert info["kernel"] == "wide-f32" and math.isinf(info["input_limit"]) and info["pack"] == 1, info
    k = na.wavenet_kernel(m)
    assert (k["family"], k["kernel_name"], k["virtual"]) == ("wide-f32", "WaveNetWideF32Kernel", False), k
    with pytest.raises(na.NeuralAudioError, match="wider than 16 channels"):
        _loader(False).CreateFromString(text, ".nam", doPrewarm=False)


@pytest.mark.parametrize("knobs", [{}, {"NA_WN_KERNEL": "split"}, {"NA_WN_KERNEL": "generic"}, {"NA_WN_KERNEL": "frame"}], ids=lambda k: k.get("NA_WN_KERNEL", "auto"))
def test_a_narrow_model_with_the_option_is_predicted_on_the_frame_family_whatever_the_knob(knobs):
    path = os.path.join(O.MODELS_DIR, "BossWN-standard.nam")
    m = _loader(True).CreateFromFile(path, doPrewarm=False)
    k = na.wavenet_kernel(m, streams=600, knobs=knobs)
    assert (k["family"], k["kernel_name"], k["pack"], k["virtual"]) == ("frame", "WaveNetFrameKernel", 1, False) and math.isinf(k["input_limit"]), k
    assert na.wavenet_kernel(_loader(False).CreateFromFile(path, doPrewarm=False), streams=600, knobs={})["family"] == "f16-split"


def test_a_gated_array_wider_than_16_channels_is_still_refused():
    c = GC.case("wide", [20], 3, [1, 2], 1)
    with pytest.raises(na.NeuralAudioError, match="layer array 0: gated layers at 20 channels.*at most 16 channels"):
        _loader(True).CreateFromString(GC.nam_json(c["arrays"], GC.weights(c)), ".nam", doPrewarm=False)
