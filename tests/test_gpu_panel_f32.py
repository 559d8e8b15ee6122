"""WaveNetPanelF32Kernel (csrc/wavenet_panel_f32_kernels.hip): WaveNets of 129 .. 256 channels in exact f32, for models of a loader with
SetWaveNetExactF32(True) -- against the float64 evaluation (ref_np) at the f32 oracle's own distance from it (_float64_bound).  Every
batch asserts the kernel name before its output is trusted."""
import os

import numpy as np
import pytest

import na_oracle as O
import ref_np
import wide_cases as WC
from test_gpu_wide import BLOCK, _float64_bound, _run, na, num_cus  # noqa: F401 (fixtures)

FORCED = bool(os.environ.get("NA_WN_KERNEL") or os.environ.get("NA_WN_PACK") or os.environ.get("NA_WN_SPEC") or os.environ.get("NA_WN_PAD"))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(FORCED, reason="forced kernel family")]
NAME = "WaveNetPanelF32Kernel"
# K = 1 / 3 / 4; dilations inside the 64-frame block, at its edge (63 / 64 / 65) and in the ring alone (200): the last array has the
# second pair of layers, the arrays in front of it the first four (float64 evaluation and oracle stay within seconds at 256 / 256)
LAYERS, LAST_LAYERS = ([3, 4, 3, 1], [1, 63, 64, 2]), ([3, 3], [65, 200])
SHAPES = [((129, 1), O.ACT_TANH), ((160, 80), O.ACT_TANH), ((193, 17), O.ACT_TANH), ((8, 200, 24), O.ACT_TANH), ((255, 255), O.ACT_LEAKYRELU),
          ((256, 256), O.ACT_TANH)]


@pytest.fixture(scope="module")
def loaders(na):
    exact, default, exact_std = na.NeuralModelLoader(), na.NeuralModelLoader(), na.NeuralModelLoader()
    exact.SetWaveNetExactF32(True)
    exact_std.SetWaveNetExactF32(True)
    exact_std.SetWaveNetMathMode(na.EMathMode.StdMath)
    return {"exact": exact, "default": default, "exact-std": exact_std}


def _batch(na, models_and_counts):
    b = na.Batch(0)
    for m, count in models_and_counts:
        b.AddStreams(m, count)
    return b


def _load(loader, arrays, w):
    return loader.CreateFromString(O.nam_json_wavenet_generic(arrays, w), ".nam")


def _follows_float64(y, arrays, w, x, what, math_mode=O.MATH_FAST):
    """_float64_bound with the f32 oracle as the yardstick, and the ratio g / o it leaves room under (DESIGN.md 2.5 quotes the worst)"""
    yo = O.OracleWaveNet(arrays, w, math_mode=math_mode).process(x)
    y64 = ref_np.wavenet_forward(arrays, w, x, tanh=np.tanh if math_mode == O.MATH_STD else ref_np.fast_tanh)[0]
    assert np.all(np.isfinite(yo)) and O.rms(yo) > 0
    _float64_bound(y, yo, y64, what)
    print("%s: g / o = %.3f" % (what, O.rms(y - y64) / max(O.rms(yo - y64), 1e-300)))


@pytest.mark.parametrize("channels,act", SHAPES, ids=["-".join(map(str, c)) for c, _ in SHAPES])
def test_shapes_follow_float64_whatever_the_call_sizes(na, loaders, channels, act):
    arrays = WC.chain(list(channels), [LAYERS] * (len(channels) - 1) + [LAST_LAYERS], act)
    w = O.synth_wavenet_weights(arrays, seed=sum(channels))
    m = _load(loaders["exact"], arrays, w)
    x = O.signal_noise(300 + 37 * 16, seed=sum(channels))
    ys = []
    for sizes in ([BLOCK] * 8, [1] * 300 + [37] * 16):
        b = _batch(na, [(m, 1)])
        assert b.StreamKernelName(0) == NAME and np.isinf(b.StreamInputLimit(0))
        ys.append(_run(b, x[None, :], sizes)[0])
        b.close()
    _follows_float64(ys[0], arrays, w, x, channels)
    assert np.array_equal(ys[0], ys[1]), (channels, float(np.abs(ys[0] - ys[1]).max()))


def test_stdmath_matches_its_oracle(na, loaders):
    arrays = WC.two_array(160, 80)
    w = O.synth_wavenet_weights(arrays, seed=11)
    b = _batch(na, [(_load(loaders["exact-std"], arrays, w), 1)])
    assert b.StreamKernelName(0) == NAME
    x = O.signal_noise(3 * BLOCK + 37, seed=12)
    y = _run(b, x[None, :], [BLOCK, 37, BLOCK, BLOCK])[0]
    b.close()
    _follows_float64(y, arrays, w, x, "stdmath", O.MATH_STD)


def test_refused_weights_and_a_hot_input_follow_float64_unclamped(na, loaders):
    arrays = WC.two_array(160, 80)
    w = O.synth_wavenet_weights(arrays, seed=160)
    ws = O.scale_wavenet_tensors(arrays, w, WC.WEIGHT_SCALINGS["mix-in x 1e5"])
    b = _batch(na, [(_load(loaders["exact"], arrays, ws), 1), (_load(loaders["exact"], arrays, w), 1)])
    assert [b.StreamKernelName(s) for s in (0, 1)] == [NAME, NAME] and np.isinf(b.StreamInputLimit(1))
    x = np.stack([O.signal_noise(4 * BLOCK, 5), (1e5 * O.signal_noise(4 * BLOCK, 5)).astype(np.float32)])
    y = _run(b, x, [BLOCK] * 4)
    assert b.StreamRangeEvents(0) == 0 and b.StreamRangeEvents(1) == 0
    b.close()
    _follows_float64(y[0], arrays, ws, x[0], "mix-in x 1e5")
    _follows_float64(y[1], arrays, w, x[1], "1e5 x noise")


def test_more_streams_than_cus_and_streams_that_leave(na, loaders, num_cus):
    arrays = WC.chain([144], [([3, 2], [1, 64])])
    w = O.synth_wavenet_weights(arrays, seed=144)
    streams = num_cus + 4
    b = _batch(na, [(_load(loaders["exact"], arrays, w), streams)])
    assert b.StreamKernelName(streams - 1) == NAME
    x5 = np.stack([O.signal_noise(3 * BLOCK + 37, 30 + s) for s in range(5)])
    x = x5[np.arange(streams) % 5]
    cut = 2 * BLOCK
    y = _run(b, x[:, :cut], [BLOCK, BLOCK])
    for s in range(5, streams):
        assert np.array_equal(y[s], y[s % 5]), s
    gone = (streams // 2, streams // 2 + 2)
    for s in gone:
        b.RemoveStreams(s)
    y2 = _run(b, x[:, cut:], [BLOCK, 37])  # the live rows are no longer contiguous: the index lists
    b.close()
    for s in (0, streams // 3, streams // 2 + 1, streams - 1):
        _follows_float64(np.concatenate([y[s], y2[s]]), arrays, w, x5[s % 5], (s, "after RemoveStreams"))
    assert not np.any(y2[list(gone)])


def test_a_panel_group_shares_a_batch_with_the_other_families(na, loaders):
    wide, narrow = WC.two_array(160, 80), WC.two_array(40, 20)
    ww, wn = O.synth_wavenet_weights(wide, seed=160), O.synth_wavenet_weights(narrow, seed=40)
    std = loaders["default"].CreateFromFile(os.path.join(O.MODELS_DIR, "BossWN-standard.nam"))
    b = _batch(na, [(_load(loaders["exact"], wide, ww), 2), (_load(loaders["default"], narrow, wn), 2), (std, 2)])
    assert [b.StreamKernelName(s) for s in (0, 2, 4)] == [NAME, "WaveNetGenericKernel", "WaveNetSpecKernel"]
    x = np.stack([O.signal_noise(2 * BLOCK + 37, 70 + s) for s in range(6)])
    y = _run(b, x, [BLOCK, 37, BLOCK])
    b.close()
    _follows_float64(y[1], wide, ww, x[1], "panel group")
    for s in (2, 5):
        yo = (O.OracleWaveNet(narrow, wn) if s < 4 else O.oracle_from_file("BossWN-standard.nam")).process(x[s])
        assert O.rms(y[s] - yo) < 2e-6 * max(1.0, O.rms(yo)), s  # the suite's WaveNet parity tolerance


def test_a_live_stream_moves_to_a_fresh_batch_mid_signal(na, loaders):
    arrays = WC.two_array(160, 80)
    m = _load(loaders["exact"], arrays, O.synth_wavenet_weights(arrays, seed=7))
    x = O.signal_noise(4 * BLOCK + 100, seed=8)[None, :]
    whole, first, second = _batch(na, [(m, 1)]), _batch(na, [(m, 1)]), _batch(na, [(m, 1)])
    assert second.StreamKernelName(0) == NAME
    y = _run(whole, x, [BLOCK] * 5)
    cut = 2 * BLOCK + 37
    _run(first, x[:, :cut], [BLOCK, BLOCK, 37])
    second.LoadStreams([0], first.SaveStreams([0]))
    y2 = _run(second, x[:, cut:], [BLOCK] * 3)
    for b in (whole, first, second):
        b.close()
    assert np.array_equal(y2[0], y[0, cut:])
