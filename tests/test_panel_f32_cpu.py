"""Exact f32 beyond 128 channels (NeuralModelLoader.SetWaveNetExactF32, csrc/wavenet_panel_f32_kernels.hip) without a GPU: what loads,
which kernel a model is predicted on, and which instantiation a launch takes.  tests/test_gpu_panel_f32.py runs the kernel."""
import math
import os
import subprocess

import pytest

import na_oracle as O
import neuralaudio_amd as na
import wide_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _text(channels):
    arrays = WC.chain(list(channels), [([3, 2], [1, 70])] * len(channels))
    return O.nam_json_wavenet_generic(arrays, O.synth_wavenet_weights(arrays, seed=sum(channels)))


def _loader(exact):
    loader = na.NeuralModelLoader()
    loader.SetWaveNetExactF32(exact)
    return loader


@pytest.mark.parametrize("knobs", [{}, {"NA_WN_KERNEL": "split"}, {"NA_WN_KERNEL": "generic"}], ids=lambda k: k.get("NA_WN_KERNEL", "auto"))
@pytest.mark.parametrize("channels", [(129,), (160, 80), (193,), (256, 256)], ids=str)
def test_a_model_of_129_to_256_channels_loads_with_the_option_onto_the_panel_kernel(channels, knobs):
    m = _loader(True).CreateFromString(_text(channels), ".nam", doPrewarm=False)
    info = m.KernelInfo(1.0, 1)
    assert info["kernel"] == "wide-f32" and math.isinf(info["input_limit"]) and info["pack"] == 1, info
    k = na.wavenet_kernel(m, knobs=knobs)
    assert (k["family"], k["kernel_name"], k["pack"], k["virtual"]) == ("wide-f32", "WaveNetPanelF32Kernel", 1, False) and math.isinf(k["input_limit"]), k


def test_the_limits_on_both_sides_of_the_new_widths():
    assert na.wavenet_kernel(_loader(True).CreateFromString(_text((128,)), ".nam", doPrewarm=False))["kernel_name"] == "WaveNetWideF32Kernel"
    with pytest.raises(na.NeuralAudioError, match=r"layer array 0: 257 channels.*limit is 256"):
        _loader(True).CreateFromString(_text((257,)), ".nam", doPrewarm=False)
    with pytest.raises(na.NeuralAudioError, match="channels > 128"):
        _loader(False).CreateFromString(_text((129,)), ".nam", doPrewarm=False)


def test_the_launch_choice_at_its_edges(tmp_path):
    exe = tmp_path / "panel_choice_cases"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "neuralaudio_amd", "csrc"),
                    os.path.join(ROOT, "tests", "panel_choice_cases.cpp"), "-o", str(exe)], check=True)
    asked = [(128, 0), (129, 0), (192, 0), (193, 0), (256, 0), (257, 0), (64, 1), (65, 1), (129, 1)]
    out = subprocess.run([str(exe)] + [str(v) for pair in asked for v in pair], capture_output=True, text=True, check=True).stdout.split("\n")
    got = [tuple(int(v) for v in line.split()) for line in out if line]
    # (wide kernel's NB, panel kernel's NB, frames per launch); gated models stay where they were: 64 channels at most
    assert got == [(8, 0, 128), (0, 12, 64), (0, 12, 64), (0, 16, 64), (0, 16, 64), (0, 0, 0), (4, 0, 128), (0, 0, 0), (0, 0, 0)]
