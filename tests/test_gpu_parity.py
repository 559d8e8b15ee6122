"""GPU parity tests proper: the HIP path (through the C ABI) against the CPU oracle on the same inputs.

Tolerance: BASELINE.json's north_star asks for <= 1e-4 RMS against the reference Internal CPU path.
The HIP path computes in FP32 with the same rational tanh/sigmoid, so we hold it to 2e-6 RMS here
(observed ~1e-7: pure f32 summation-order noise).
"""
import os

import numpy as np
import pytest

import na_oracle as O

pytestmark = pytest.mark.gpu

TOL_RMS = 2e-6
NORTH_STAR_TOL = 1e-4


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


@pytest.fixture(scope="module")
def loader(na):
    return na.NeuralModelLoader()


def _model_path(name):
    return os.path.join(O.MODELS_DIR, name)


WAVENET_FILES = [("BossWN-standard.nam", 1.0), ("BossWN-feather.nam", 1.0), ("BossWN-nano.nam", 1.0),
                 ("BossWN-a2.nam", 0.0), ("BossWN-a2.nam", 1.0)]


@pytest.mark.parametrize("name,quality", WAVENET_FILES)
@pytest.mark.parametrize("block", [128, 37])
def test_single_stream_wavenet_matches_oracle(na, loader, name, quality, block):
    loader.SetDefaultQualityScaleFactor(quality)
    m = loader.CreateFromFile(_model_path(name))
    loader.SetDefaultQualityScaleFactor(1.0)
    assert m is not None
    ora = O.oracle_from_file(name, quality=quality)
    n = 8192 if block == 128 else 37 * 40
    x = O.signal_sine(n)
    y = np.concatenate([m.Process(x[i:i + block]) for i in range(0, n, block)])
    yo = ora.process(x)
    err = O.rms(y - yo)
    assert O.rms(yo) > 0.05
    assert err < TOL_RMS, (name, quality, block, err)


@pytest.mark.parametrize("name", ["BossLSTM-1x16.nam", "BossLSTM-2x8.nam", "tw40_blues_deluxe_deerinkstudios.json"])
def test_single_stream_lstm_matches_oracle(na, loader, name):
    m = loader.CreateFromFile(_model_path(name))
    assert m is not None
    ora = O.oracle_from_file(name)
    x = O.signal_sine(4096)
    y = np.concatenate([m.Process(x[i:i + 128]) for i in range(0, x.size, 128)])
    yo = ora.process(x)
    assert O.rms(y - yo) < 5e-6, (name, O.rms(y - yo))


def test_batch_streams_are_independent_and_match_oracle(na, loader):
    """64 Standard streams with different inputs == 64 independent oracle runs (spot-check 4 of them)."""
    m = loader.CreateFromFile(_model_path("BossWN-standard.nam"), doPrewarm=False)
    b = na.Batch(0)
    S, n, blocks = 64, 128, 12
    b.AddStreams(m, S)
    x = np.stack([O.signal_sine(n * blocks, start=977 * s) if s % 2 == 0 else O.signal_noise(n * blocks, 1234 + s)
                  for s in range(S)])
    y = np.concatenate([b.Process(x[:, i * n:(i + 1) * n]) for i in range(blocks)], axis=1)
    for s in (0, 1, 31, 63):
        yo = O.oracle_from_file("BossWN-standard.nam").process(x[s])
        assert O.rms(y[s] - yo) < TOL_RMS, (s, O.rms(y[s] - yo))


def test_keras_gru_file_matches_committed_torch_vectors(na, loader):
    """HIP path vs an INDEPENDENT implementation: tests/golden/gru_torch.npz holds torch.nn.GRU's output for the committed synthetic
    keras GRU model (the reference evaluates GRU with RTNeural, which is absent: parity unpinned)."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gru_torch.npz"))
    m = loader.CreateFromFile(_model_path("synthetic_gru_1x16.json"))
    assert m is not None
    x = g["input"]
    y = np.concatenate([m.Process(x[i:i + 128]) for i in range(0, x.size, 128)])
    assert O.rms(y - g["output"]) < 5e-6


# ------------------------------------------------------------------------------------------------ StdMath policy

def test_keras_lstm_known_answer_vector_through_the_hip_path(na):
    """The reference's ONLY golden output: Utils/Models/tw40_blues_deluxe_deerinkstudios.json carries input_batch -> output_batch
    (exact-math vector: StdMath, zero state, no prewarm).  The HIP path in StdMath mode (the reference's -DLSTM_MATH=StdMath build,
    NeuralAudio/CMakeLists.txt:94-96, Activation.h:20-45) must reproduce it directly -- no oracle in between."""
    j = O.load_json("tw40_blues_deluxe_deerinkstudios.json")
    x = np.asarray(j["input_batch"], np.float32).ravel()
    want = np.asarray(j["output_batch"], np.float32).ravel()
    ld = na.NeuralModelLoader()
    ld.SetLSTMMathMode(na.EMathMode.StdMath)
    m = ld.CreateFromFile(_model_path("tw40_blues_deluxe_deerinkstudios.json"), doPrewarm=False)
    y = np.concatenate([m.Process(x[i:i + 128]) for i in range(0, x.size, 128)])
    err = O.rms(y - want)
    assert O.rms(want) > 0.01
    assert err < 1e-6, err
    # and the default FastMath build of the same file is NOT that vector (4.8e-3 RMS in the oracle): the knob is live
    m2 = na.NeuralModelLoader().CreateFromFile(_model_path("tw40_blues_deluxe_deerinkstudios.json"), doPrewarm=False)
    y2 = np.concatenate([m2.Process(x[i:i + 128]) for i in range(0, x.size, 128)])
    assert O.rms(y2 - want) > 1e-3


@pytest.mark.parametrize("name", ["BossLSTM-1x16.nam", "BossLSTM-2x8.nam", "tw40_blues_deluxe_deerinkstudios.json"])
def test_stdmath_lstm_matches_stdmath_oracle(na, name):
    ld = na.NeuralModelLoader()
    ld.SetLSTMMathMode(na.EMathMode.StdMath)
    m = ld.CreateFromFile(_model_path(name))
    x = O.signal_noise(2048, 5)
    y = np.concatenate([m.Process(x[i:i + 128]) for i in range(0, x.size, 128)])
    yo = O.oracle_from_file(name, math_mode=O.MATH_STD).process(x)
    assert O.rms(y - yo) < 5e-6, (name, O.rms(y - yo))


@pytest.mark.parametrize("name", ["BossWN-standard.nam", "BossWN-nano.nam"])
def test_stdmath_wavenet_matches_stdmath_oracle(na, name):
    ld = na.NeuralModelLoader()
    ld.SetWaveNetMathMode(na.EMathMode.StdMath)
    m = ld.CreateFromFile(_model_path(name))
    x = O.signal_sine(2048)
    y = np.concatenate([m.Process(x[i:i + 128]) for i in range(0, x.size, 128)])
    yo = O.oracle_from_file(name, math_mode=O.MATH_STD).process(x)
    print("%s: StdMath HIP path - StdMath oracle %.3g RMS" % (name, O.rms(y - yo)))
    assert O.rms(y - yo) < TOL_RMS, (name, O.rms(y - yo))  # (measured: Standard 2.6e-7, Nano 2.1e-7; tests/test_gpu_stdmath.py has the rest)
    yf = O.oracle_from_file(name).process(x)
    assert O.rms(yo - yf) > 1e-5  # the two policies differ measurably (6.6e-4 on Standard / sine)


@pytest.mark.parametrize("layers,hidden", [(1, 12), (2, 12), (1, 4), (2, 6), (1, 13), (2, 9), (1, 1), (1, 24), (1, 17), (1, 20), (1, 32)])
@pytest.mark.parametrize("std", [False, True], ids=["fastmath", "stdmath"])
def test_lstm_hidden_sizes_padded_into_the_dpp_layouts_match_oracle(na, layers, hidden, std):
    """Hidden sizes below a lane layout of the LDS-free kernel (8 or 16 units per gate block) run padded: the reference's static 1x12 /
    2x12 (NeuralModel.cpp:33,37) as 16, small ones as 8 (two layers: side by side in the wave halves); one layer of 17 .. 32 units (the
    reference's static 1x24, :35) on the 32-unit layout."""
    ld = na.NeuralModelLoader()
    if std:
        ld.SetLSTMMathMode(na.EMathMode.StdMath)
    w = O.synth_lstm_weights(layers, hidden, seed=300 + 10 * hidden + layers)
    m = ld.CreateFromString(O.nam_json_lstm(layers, hidden, w), ".nam", doPrewarm=True)
    assert m is not None
    x = O.signal_noise(1000, 7)
    want = O.OracleLSTM.from_nam(layers, hidden, w, math_mode=O.MATH_STD if std else O.MATH_FAST).process(x)
    got = np.concatenate([m.Process(x[i:i + 100]) for i in range(0, x.size, 100)])
    assert O.rms(got - want) < 5e-6, (layers, hidden, O.rms(got - want))


@pytest.mark.parametrize("kind,layers,hidden", [("lstm", 1, 16), ("lstm", 2, 8), ("lstm", 1, 24), ("lstm", 2, 12), ("lstm", 1, 32), ("lstm", 2, 5),
                                                ("gru", 1, 24), ("gru", 1, 16), ("gru", 2, 8), ("gru", 1, 32), ("gru", 1, 7)])
def test_recurrent_models_through_tiny_and_ragged_buffers(na, kind, layers, hidden):
    """Every body of the LDS-free recurrent kernel (8 / 16 / 32-unit layouts, the side-by-side two-layer one with its peeled boundary ticks)
    through buffers of 1, 2, 3, 5 ... 129, 300 samples: groups of four, tails, chunking above 128 (InternalModel.h:104-117 is chunk-invariant)."""
    import json
    sizes = [1, 2, 3, 5, 1, 4, 7, 128, 1, 127, 64, 33, 2, 129, 300]
    x = O.signal_noise(sum(sizes), 11)
    if kind == "lstm":
        w = O.synth_lstm_weights(layers, hidden, seed=5 + hidden)
        m = na.NeuralModelLoader().CreateFromString(O.nam_json_lstm(layers, hidden, w), ".nam", doPrewarm=True)
        want = O.OracleLSTM.from_nam(layers, hidden, w).process(x)
    else:
        gj = O.synth_keras_gru(layers, hidden, seed=5 + hidden)
        m = na.NeuralModelLoader().CreateFromString(json.dumps(gj), ".json", doPrewarm=True)
        want = O.OracleGRU(gj).process(x)
    out, pos = [], 0
    for n in sizes:
        out.append(m.Process(x[pos:pos + n]))
        pos += n
    assert O.rms(np.concatenate(out) - want) < 5e-6


# one shape per recurrent kernel that some knob set can reach (lstm_dev.h RecurrentKernelFor): the LDS-free kernel, the shaped one-wave
# instances, the runtime-shaped kernel on one wave and on a workgroup, and -- under NA_LSTM_LANE_KERNEL / NA_LSTM_NO_WAVE_RT, in the forced
# runs of test_gpu_families.py -- LstmBlockKernel<40>, LstmGenericKernel (also with a dense tail) and GruGenericKernel
DISPATCH_SHAPES = [[("lstm", 16)], [("lstm", 24), ("lstm", 24)], [("gru", 20), ("gru", 20)], [("lstm", 16), ("lstm", 16), ("lstm", 16)], [("gru", 86)],
                   [("lstm", 40)], [("lstm", 5)], [("lstm", 8), ("dense", 4, "tanh"), ("dense", 1)]]


@pytest.mark.parametrize("spec", DISPATCH_SHAPES, ids=lambda s: "-".join("%s%d" % (l[0], l[1]) for l in s))
def test_the_kernel_the_decision_names_runs_and_is_right(na, loader, spec):
    """Three streams (the lane = stream kernels mask 61 idle lanes), 72 samples as calls of 65 and 7: NA_BatchStreamKernelName is the
    kernel that RecurrentKernelFor names for the process's own tuning knobs, and the output is the oracle's."""
    import json
    import recurrent_cases as RC
    import ref_np as R
    kind, hidden, layers, tail_layers, tail_width, tail_history = RC.stack_dims(spec)
    want_name = na.recurrent_kernel(kind, hidden, layers, tail_layers, tail_width, tail_history, knobs=None)
    x = np.stack([O.signal_noise(72, 20 + s) for s in range(3)])
    if tail_layers:
        mj = R.synth_keras_stack(spec, seed=77)
        doc, ext, prewarm = json.dumps(mj), ".json", True
        want = np.stack([R.keras_stack_forward(mj, x[s]) for s in range(3)])
    elif kind == "lstm":
        w = O.synth_lstm_weights(layers, hidden, seed=70 + hidden)
        doc, ext, prewarm = O.nam_json_lstm(layers, hidden, w), ".nam", True
        want = np.stack([O.OracleLSTM.from_nam(layers, hidden, w).process(x[s]) for s in range(3)])
    else:
        gj = O.synth_keras_gru(layers, hidden, seed=70 + hidden)
        doc, ext, prewarm = json.dumps(gj), ".json", True
        want = np.stack([O.OracleGRU(gj).process(x[s]) for s in range(3)])
    if want_name == "":
        # no kernel takes the shape under these knobs (GRU 1x86 without the runtime-shaped kernel: beyond GruGenericKernel's LDS): an error, no launch
        m = loader.CreateFromString(doc, ext, doPrewarm=False)
        assert m is not None
        b = na.Batch(0)
        b.AddStreams(m, 3, doPrewarm=False)
        with pytest.raises(na.NeuralAudioError):
            b.Process(x[:, :65])
        return
    m = loader.CreateFromString(doc, ext, doPrewarm=prewarm)
    assert m is not None
    b = na.Batch(0)
    b.AddStreams(m, 3)
    y = np.concatenate([b.Process(x[:, :65]), b.Process(x[:, 65:])], axis=1)
    # the LDS-free kernel reports its four-streams-per-wave flavour where the library's threshold (NA_REC_QUAD_MIN; default 2049 streams)
    # puts the three streams of a one-layer model of up to 16 units on it: the library says what its threshold is
    lib = na.capi.load_library()
    quad_min = lib.NA_DebugSetRecurrentQuadMin(0)
    lib.NA_DebugSetRecurrentQuadMin(quad_min)
    if want_name == "RecurrentDppKernel" and layers == 1 and hidden <= 16 and 0 < quad_min <= 3:
        want_name = "RecurrentQuadKernel"
    assert b.StreamKernelName(0) == want_name and b.StreamKernelName(2) == want_name, (b.StreamKernelName(0), b.StreamKernelName(2), want_name)
    for s in range(3):
        err = O.rms(y[s] - want[s])
        print("%s stream %d: rms error %.3g, bound %.3g" % (want_name, s, err, RC.bound(want[s])))
        assert err <= RC.bound(want[s]), (spec, s, err)


@pytest.mark.parametrize("layers,hidden", [(1, 3), (1, 18), (3, 16), (2, 40), (2, 64), (1, 128), (2, 96), (3, 128)])
def test_runtime_shaped_lstm_matches_oracle(na, loader, layers, hidden):
    """Hidden sizes / layer counts without a shaped kernel run on the runtime-shaped one (LSTMDynamic.h:95-108 accepts any); shapes
    whose weights exceed the LDS (2x64 and up) stream them from L2, up to 128 units."""
    if (os.environ.get("NA_LSTM_NO_WAVE_RT") or os.environ.get("NA_LSTM_LANE_KERNEL")) and (hidden > 64 or layers * hidden > 128):
        pytest.skip("beyond the lane = stream kernel's LDS bound")
    w = O.synth_lstm_weights(layers, hidden, seed=100 + hidden)
    m = loader.CreateFromString(O.nam_json_lstm(layers, hidden, w), ".nam")
    assert m is not None
    x = O.signal_noise(512, 3)
    y = np.concatenate([m.Process(x[i:i + 100]) for i in range(0, x.size, 100)])
    yo = O.OracleLSTM.from_nam(layers, hidden, w).process(x)
    assert O.rms(y - yo) < 5e-6, (layers, hidden, O.rms(y - yo))


@pytest.mark.parametrize("spec", [[("lstm", 8), ("dense", 6, "tanh"), ("dense", 1)], [("gru", 12), ("dense", 5, "relu"), ("dense", 3, "sigmoid"), ("dense", 1)],
                                  [("dense", 8, "tanh"), ("dense", 4, "elu"), ("dense", 1)], [("gru", 8), ("gru", 8), ("dense", 2)],
                                  [("lstm", 16), ("dense", 1, "tanh")], [("lstm", 5), ("lstm", 5), ("dense", 64, "relu"), ("dense", 1)],
                                  # activation / batchnorm / prelu layers (lowered to dense layers at load, model_loader.cpp AppendKerasTailLayer)
                                  [("gru", 8), ("dense", 6), ("batchnorm", 6), ("activation", 6, "tanh"), ("dense", 1)],
                                  [("lstm", 8), ("prelu", 8), ("dense", 4), ("prelu", 4, "scalar"), ("batchnorm", 4, "noaffine"), ("dense", 1)],
                                  [("dense", 8), ("activation", 8, "relu"), ("batchnorm", 8), ("dense", 1)],
                                  # dense layers wider than 64 units (round 4: up to 256)
                                  [("lstm", 8), ("dense", 128, "tanh"), ("dense", 1)], [("dense", 200, "relu"), ("dense", 96, "tanh"), ("dense", 1)],
                                  [("gru", 24), ("dense", 256, "sigmoid"), ("dense", 100), ("prelu", 100), ("dense", 1)],
                                  # conv1d layers (causal, dilated; their input history is stream state) and softmax (round 5)
                                  [("conv1d", 8, 3, 1, "tanh"), ("conv1d", 8, 3, 2, "tanh"), ("conv1d", 4, 2, 4, "relu"), ("dense", 1)],
                                  [("lstm", 8), ("conv1d", 6, 5, 3), ("prelu", 6), ("batchnorm", 6), ("dense", 1, "tanh")],
                                  [("gru", 12), ("conv1d", 16, 4, 64, "elu"), ("dense", 5, "softmax"), ("dense", 1)],
                                  [("conv1d", 4, 12, 1), ("activation", 4, "softmax"), ("conv1d", 1, 2, 100, "sigmoid")],
                                  [("dense", 6, "tanh"), ("conv1d", 3, 3, 170, "tanh"), ("conv1d", 1, 1, 1)],
                                  # softmax in tails WITHOUT a conv1d layer (the per-sample DenseTail; round 6 -- it was evaluated as linear there)
                                  [("lstm", 8), ("dense", 4, "softmax"), ("dense", 1)], [("gru", 8), ("dense", 4, "softmax"), ("dense", 1)],
                                  [("dense", 6, "softmax"), ("dense", 1)], [("gru", 6), ("dense", 5), ("activation", 5, "softmax"), ("dense", 2, "tanh")]],
                         ids=lambda s: "-".join("%s%d%s" % (l[0], l[1], "".join(str(v) for v in l[2:])) for l in s))
def test_generic_keras_stack_matches_numpy_restatement(na, loader, spec):
    """Generic keras stacks: the reference evaluates them with RTNeural, which is an absent submodule -- parity unpinned;
    the checker is tests/ref_np.keras_stack_forward (Keras layer definitions, float64, accurate tanh as the reference's
    FastMathsProvider).  Chunked processing must not matter either."""
    import json
    import ref_np as R
    if (os.environ.get("NA_LSTM_NO_WAVE_RT") or os.environ.get("NA_LSTM_LANE_KERNEL")) and max(l[1] for l in spec if l[0] != "lstm" and l[0] != "gru") > 64:
        pytest.skip("dense layers wider than 64 units are beyond the lane = stream kernels' LDS bound")
    mj = R.synth_keras_stack(spec, seed=40 + len(spec))
    m = loader.CreateFromString(json.dumps(mj), ".json")
    assert m is not None
    x = O.signal_noise(384, 9)
    y = np.concatenate([m.Process(x[i:i + 100]) for i in range(0, x.size, 100)])
    yr = R.keras_stack_forward(mj, x)
    assert O.rms(y - yr) < 5e-6, (spec, O.rms(y - yr))
    m2 = loader.CreateFromString(json.dumps(mj), ".json")
    y2 = m2.Process(x)
    assert np.max(np.abs(y2 - y)) < 1e-6


@pytest.mark.parametrize("channels,head", [(24, 12), (32, 8), (20, 3), (64, 2)])
def test_wavenet_wider_than_16_channels_matches_oracle(na, loader, channels, head):
    """Layer arrays wider than the shaped kernels take run on the runtime-shaped block kernel (the reference's dynamic engine accepts
    any channel count, WaveNetDynamic.h:229-254): parity vs the oracle, chunk invariance, prewarmed start."""
    arrays = [dict(input_size=1, condition_size=1, head_size=head, head_kernel_size=1, head_dilation=1, channels=channels, has_head_bias=False,
                   activation=O.ACT_TANH, kernel_sizes=[3, 3, 2, 3], dilations=[1, 7, 64, 200]),
              dict(input_size=channels, condition_size=1, head_size=1, head_kernel_size=1, head_dilation=1, channels=head, has_head_bias=True,
                   activation=O.ACT_TANH, kernel_sizes=[3, 5], dilations=[3, 40])]
    w = O.synth_wavenet_weights(arrays, seed=channels)
    m = loader.CreateFromString(O.nam_json_wavenet_generic(arrays, w), ".nam")
    assert m is not None
    x = O.signal_noise(700, 5)
    y = np.concatenate([m.Process(x[i:i + 128]) for i in range(0, x.size, 128)])
    yo = O.OracleWaveNet(arrays, w).process(x)
    assert O.rms(y - yo) < 2e-6, (channels, O.rms(y - yo))
    m2 = loader.CreateFromString(O.nam_json_wavenet_generic(arrays, w), ".nam")
    y2 = np.concatenate([m2.Process(x[i:i + 37]) for i in range(0, x.size, 37)])
    assert np.max(np.abs(y2 - y)) < 1e-6


@pytest.mark.parametrize("channels,head,act", [(80, 72, O.ACT_TANH), (100, 50, O.ACT_TANH), (128, 64, O.ACT_TANH), (128, 128, O.ACT_LEAKYRELU), (66, 3, O.ACT_TANH)])
def test_wavenet_of_65_to_128_channels_matches_oracle(na, loader, channels, head, act):
    """WaveNetDynamic.h:229-254 takes any width; layer arrays of 65 .. 128 channels run on WaveNetWideKernel (64 x 64 sub-matrices through
    the matrix pipe, head accumulator in registers): parity vs the oracle with a second array that rechannels from the wide one, chunk
    invariance, a prewarmed start, several streams per batch."""
    arrays = [dict(input_size=1, condition_size=1, head_size=head, head_kernel_size=1, head_dilation=1, channels=channels, has_head_bias=False,
                   activation=act, kernel_sizes=[3, 3, 2, 3], dilations=[1, 7, 64, 200]),
              dict(input_size=channels, condition_size=1, head_size=1, head_kernel_size=1, head_dilation=1, channels=head, has_head_bias=True,
                   activation=act, kernel_sizes=[3, 5], dilations=[3, 40])]
    w = O.synth_wavenet_weights(arrays, seed=channels)
    m = loader.CreateFromString(O.nam_json_wavenet_generic(arrays, w), ".nam")
    assert m is not None
    x = O.signal_noise(700, 5)
    y = np.concatenate([m.Process(x[i:i + 128]) for i in range(0, x.size, 128)])
    yo = O.OracleWaveNet(arrays, w).process(x)
    assert O.rms(yo) > 1e-5 and O.rms(y - yo) < 2e-6 * max(1.0, O.rms(yo)), (channels, O.rms(y - yo), O.rms(yo))
    m2 = loader.CreateFromString(O.nam_json_wavenet_generic(arrays, w), ".nam")
    y2 = np.concatenate([m2.Process(x[i:i + 37]) for i in range(0, x.size, 37)])
    assert np.max(np.abs(y2 - y)) < 1e-6 * max(1.0, float(np.abs(y).max()))
    b = na.Batch(0)
    b.AddStreams(m, 5)
    xs = np.stack([O.signal_noise(256, 70 + s) for s in range(5)])
    ys = np.concatenate([b.Process(xs[:, :128]), b.Process(xs[:, 128:])], axis=1)
    assert b.StreamKernelName(0) == "WaveNetWideKernel"
    for s_ in (0, 4):
        assert O.rms(ys[s_] - O.OracleWaveNet(arrays, w).process(xs[s_])) < 2e-6 * max(1.0, O.rms(yo))
    b.close()


def test_128_channel_wavenet_runs_in_real_time_for_64_streams(na, loader):
    import time
    arrays = [dict(input_size=1, condition_size=1, head_size=1, head_kernel_size=1, head_dilation=1, channels=128, has_head_bias=True,
                   activation=O.ACT_TANH, kernel_sizes=[3] * 10, dilations=[1, 2, 4, 8, 16, 32, 64, 128, 256, 512])]
    m = loader.CreateFromString(O.nam_json_wavenet_generic(arrays, O.synth_wavenet_weights(arrays, seed=1)), ".nam", doPrewarm=False)
    b = na.Batch(0)
    b.AddStreams(m, 64)
    x = np.stack([O.signal_noise(128, 60 + s) for s in range(64)])
    for _ in range(3):
        b.Process(x)
    t0 = time.perf_counter()
    for _ in range(10):
        y = b.Process(x)
    per_block = (time.perf_counter() - t0) / 10
    assert np.all(np.isfinite(y))
    assert per_block < 2.5e-3, per_block  # the block lasts 2.667 ms at 48 kHz
    b.close()


@pytest.mark.parametrize("channels,act", [(24, O.ACT_LEAKYRELU), (40, O.ACT_TANH), (64, O.ACT_LEAKYRELU)])
def test_wide_wavenet_with_a_conv_head_matches_oracle(na, loader, channels, act):
    """A single wide layer array with an A2-style conv head (kernel 16, bias; the head accumulator keeps its own history ring): the
    reference's dynamic engine takes any such shape (WaveNetDynamic.h:67-83 Conv1D, :229-254, :445-468); here it runs on the
    runtime-shaped kernel, whose layer mat-muls are on the matrix pipe."""
    arrays = [dict(input_size=1, condition_size=1, head_size=1, head_kernel_size=16, head_dilation=1, channels=channels, has_head_bias=True,
                   activation=act, kernel_sizes=[6, 3, 15, 2, 6], dilations=[1, 17, 13, 101, 239])]
    w = O.synth_wavenet_weights(arrays, seed=100 + channels)
    m = loader.CreateFromString(O.nam_json_wavenet_generic(arrays, w), ".nam")
    assert m is not None
    x = O.signal_noise(128 * 12 + 50, 6)
    y = np.concatenate([m.Process(x[i:i + 128]) for i in range(0, x.size, 128)])
    yo = O.OracleWaveNet(arrays, w).process(x)
    assert O.rms(yo) > 1e-4 and O.rms(y - yo) < 2e-6 * max(1.0, O.rms(yo)), (channels, O.rms(y - yo), O.rms(yo))
    m2 = loader.CreateFromString(O.nam_json_wavenet_generic(arrays, w), ".nam")
    y2 = np.concatenate([m2.Process(x[i:i + 53]) for i in range(0, x.size, 53)])
    assert np.max(np.abs(y2 - y)) < 2e-6 * max(1.0, float(np.abs(y).max()))


def test_large_recurrent_models_run_in_real_time(na, loader):
    """LSTM 2x64 (197 KB of weights: more than the LDS) took 251 ms per 128-sample block on the lane = stream kernel in round 2 -- not
    real time (a block lasts 2.67 ms at 48 kHz; LSTMDynamic.h:95-108,166-179 runs any size in real time on a CPU).  With the weights
    streamed from L2 the wave kernel must stay under 2 ms for 64 streams; keras GRU 1x64 and LSTM 1x128 likewise."""
    import json
    import time
    if os.environ.get("NA_LSTM_NO_WAVE_RT") or os.environ.get("NA_LSTM_LANE_KERNEL"):
        pytest.skip("forced lane = stream kernels")
    w = O.synth_lstm_weights(2, 64, seed=164)
    models = [loader.CreateFromString(O.nam_json_lstm(2, 64, w), ".nam"), loader.CreateFromString(O.nam_json_lstm(1, 128, O.synth_lstm_weights(1, 128, seed=9)), ".nam"),
              loader.CreateFromString(json.dumps(O.synth_keras_gru(2, 64, seed=75)), ".json")]
    for m in models:
        assert m is not None
        b = na.Batch(0)
        b.AddStreams(m, 64)
        x = np.stack([O.signal_noise(128, 60 + s) for s in range(64)])
        for _ in range(3):
            b.Process(x)
        t0 = time.perf_counter()
        for _ in range(10):
            b.Process(x)
        per_block = (time.perf_counter() - t0) / 10
        assert per_block < 2.5e-3, per_block  # the block lasts 2.667 ms at 48 kHz (measured: 1.5 ms for the 2x64 LSTM, 2.0 for 1x128)
        b.close()


@pytest.mark.parametrize("kind,layers,hidden", [("lstm", 1, 129), ("lstm", 2, 192), ("lstm", 1, 512), ("gru", 1, 160), ("gru", 2, 200), ("lstm", 1, 1024)])
def test_recurrent_layers_wider_than_128_units_match_oracle(na, loader, kind, layers, hidden):
    """LSTMDynamic.h:95-108,166-179 takes any size; here up to 1024 units: from 65 gate rows on a stream is a workgroup of 2 .. 16 waves
    sharing the gate rows (weights streamed from L2), from 129 units on the 1-unit head is evaluated inside the sample loop.
    Ragged buffers, and a row's sum keeps the oracle's term order whatever the wave count."""
    import json
    if os.environ.get("NA_LSTM_NO_WAVE_RT") or os.environ.get("NA_LSTM_LANE_KERNEL"):
        pytest.skip("forced lane = stream kernels")
    if kind == "lstm":
        w = O.synth_lstm_weights(layers, hidden, seed=hidden + layers)
        m = loader.CreateFromString(O.nam_json_lstm(layers, hidden, w), ".nam")
        ora = O.OracleLSTM.from_nam(layers, hidden, w)
    else:
        j = O.synth_keras_gru(layers, hidden, seed=hidden + layers)
        m = loader.CreateFromString(json.dumps(j), ".json")
        ora = O.OracleGRU(j)
    assert m is not None
    x = O.signal_noise(333, 19)
    y = np.concatenate([m.Process(x[i:i + 100]) for i in range(0, x.size, 100)])
    assert np.all(np.isfinite(y))
    want = ora.process(x)
    assert O.rms(y - want) < 5e-6 * max(1.0, O.rms(want))


def test_lstm_1x256_runs_in_real_time_for_64_streams(na, loader):
    """1 MB of gate weights per model, streamed from L2 by four waves per stream: 64 streams x 128 samples inside the 2.67 ms the block lasts."""
    import time
    if os.environ.get("NA_LSTM_NO_WAVE_RT") or os.environ.get("NA_LSTM_LANE_KERNEL"):
        pytest.skip("forced lane = stream kernels")
    m = loader.CreateFromString(O.nam_json_lstm(1, 256, O.synth_lstm_weights(1, 256, seed=4)), ".nam")
    b = na.Batch(0)
    b.AddStreams(m, 64)
    x = np.stack([O.signal_noise(128, 60 + s) for s in range(64)])
    for _ in range(3):
        b.Process(x)
    t0 = time.perf_counter()
    for _ in range(10):
        y = b.Process(x)
    per_block = (time.perf_counter() - t0) / 10
    assert np.all(np.isfinite(y))
    assert per_block < 2.5e-3, per_block
    b.close()


@pytest.mark.parametrize("layers,hidden", [(1, 64), (2, 64), (1, 128)])
def test_large_keras_gru_matches_oracle(na, loader, layers, hidden):
    import json
    if os.environ.get("NA_LSTM_NO_WAVE_RT") or os.environ.get("NA_LSTM_LANE_KERNEL"):
        pytest.skip("forced lane = stream kernels")
    j = O.synth_keras_gru(layers, hidden, seed=31 + hidden)
    m = loader.CreateFromString(json.dumps(j), ".json")
    assert m is not None
    x = O.signal_noise(300, 8)
    y = np.concatenate([m.Process(x[i:i + 100]) for i in range(0, x.size, 100)])
    assert O.rms(y - O.OracleGRU(j).process(x)) < 5e-6


def test_generic_keras_stack_files_match_committed_torch_vectors(na, loader):
    """HIP path vs an INDEPENDENT implementation: tests/golden/keras_stacks_torch.npz holds torch.nn.LSTM / GRU / Linear outputs for three
    committed synthetic keras stacks (RTNeural is absent: parity unpinned)."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keras_stacks_torch.npz"))
    for name in [k for k in g.files if k != "input"]:
        if "conv" in name and (os.environ.get("NA_LSTM_NO_WAVE_RT") or os.environ.get("NA_LSTM_LANE_KERNEL")):
            continue  # (conv1d layers run on the runtime-shaped wave kernel only: forced lane = stream runs of tests/test_gpu_families.py)
        m = loader.CreateFromFile(_model_path("synthetic_stack_%s.json" % name))
        assert m is not None, name
        y = m.Process(g["input"])
        assert O.rms(y - g[name]) < 5e-6, (name, O.rms(y - g[name]))


@pytest.mark.parametrize("amp", [30.0, 1000.0, 10000.0])
def test_hot_inputs_stay_within_tolerance_on_the_f16_split_path(na, loader, amp):
    """The f16-split kernel carries every value as f16 hi + lo parts (22 mantissa bits, f16 exponent range): inputs far outside the audio
    range must still match the f32 oracle -- up to the model's clamp limit (NA_BatchStreamInputLimit: 30 677 for this model, the bound
    under which no split value can overflow; beyond it samples are clamped, tests/test_gpu_spec.py)."""
    m = loader.CreateFromFile(_model_path("BossWN-standard.nam"))
    x = (amp * np.sin(0.01 * np.arange(1024))).astype(np.float32)
    y = m.Process(x)
    yo = O.oracle_from_file("BossWN-standard.nam").process(x)
    assert np.all(np.isfinite(y)) and O.rms(y - yo) < 5e-6 * max(1.0, O.rms(yo)), (amp, O.rms(y - yo))
