"""WaveNetWideF32Kernel (csrc/wavenet_wide_f32_kernels.hip): WaveNets of 17 .. 128 channels in exact f32, for models of a loader with
SetWaveNetExactF32(True) -- against the f32 oracle at the suite's parity tolerance, and against the float64 evaluation (ref_np) where the
default kernels would refuse the weights or clamp the input.  Every batch asserts the kernel name before its output is trusted."""
import os

import numpy as np
import pytest

import na_oracle as O
import ref_np
import wide_cases as WC
from test_gpu_wide import BLOCK, _assert_parity, _blocks, _float64_bound, _run, na, num_cus  # noqa: F401 (fixtures)

FORCED = bool(os.environ.get("NA_WN_KERNEL") or os.environ.get("NA_WN_PACK") or os.environ.get("NA_WN_SPEC") or os.environ.get("NA_WN_PAD"))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(FORCED, reason="forced kernel family")]
NAME = "WaveNetWideF32Kernel"


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


def _ratio(y, yo, y64, what):
    """_float64_bound, and the ratio g / o it leaves room under (DESIGN.md 2.5 quotes the worst one)"""
    _float64_bound(y, yo, y64, what)
    print("%s: g / o = %.3f" % (what, O.rms(y - y64) / max(O.rms(yo - y64), 1e-300)))


@pytest.mark.parametrize("channels,act", WC.FIXED_CASES, ids=["-".join(map(str, c)) for c, _ in WC.FIXED_CASES])
def test_named_edge_shapes_match_the_f32_oracle_whatever_the_call_sizes(na, loaders, channels, act):
    """test_gpu_wide.py's named edges (K = 1 / 4 / 3, d = 128 / 129 / 1000, widths 17 .. 128, narrow arrays beside wide ones): whole blocks
    against the oracle, and 300 single samples followed by 37-sample calls with the same bits out."""
    arrays = WC.fixed_case(channels, act)
    w = O.synth_wavenet_weights(arrays, seed=sum(channels))
    m = _load(loaders["exact"], arrays, w)
    x = O.signal_noise(300 + 37 * 20, seed=sum(channels))
    ys = []
    for sizes in ([BLOCK] * 9, [1] * 300 + [37] * 20):
        b = _batch(na, [(m, 1)])
        assert b.StreamKernelName(0) == NAME
        ys.append(_run(b, x[None, :], sizes)[0])
        b.close()
    _assert_parity(ys[0], O.OracleWaveNet(arrays, w).process(x), channels)
    assert np.array_equal(ys[0], ys[1]), (channels, float(np.abs(ys[0] - ys[1]).max()))


@pytest.mark.parametrize("which,arrays,math", [("exact-std", WC.two_array(48, 24), O.MATH_STD),
                                               ("exact", WC.chain([40], [([3, 2, 3], [1, 9, 130])], head_kernel=7), O.MATH_FAST)], ids=["stdmath", "conv-head"])
def test_stdmath_and_a_conv_head_match_their_oracles(na, loaders, which, arrays, math):
    w = O.synth_wavenet_weights(arrays, seed=11)
    b = _batch(na, [(_load(loaders[which], arrays, w), 1)])
    assert b.StreamKernelName(0) == NAME
    x = O.signal_noise(3 * BLOCK + 37, seed=12)
    y = _run(b, x[None, :], [BLOCK, 37, BLOCK, BLOCK])[0]
    b.close()
    _assert_parity(y, O.OracleWaveNet(arrays, w, math_mode=math).process(x), which)


@pytest.mark.parametrize("scaling", list(WC.WEIGHT_SCALINGS))
@pytest.mark.parametrize("name", ["32/8 tanh", "80/72 tanh"])
def test_weights_the_default_loader_refuses_follow_the_float64_reference(na, loaders, name, scaling):
    """Every WC.WEIGHT_SCALINGS variant is refused by the default loader (test_host_cpu.py) and kept here: the f32 oracle is finite and
    not silent for all six (checked without a GPU: levels between 1.0e-9 and 2.0e-2), so none was dropped."""
    arrays, w = WC.range_model(name)
    ws = O.scale_wavenet_tensors(arrays, w, WC.WEIGHT_SCALINGS[scaling])
    with pytest.raises(na.NeuralAudioError, match="wider than 16 channels"):
        _load(loaders["default"], arrays, ws)
    b = _batch(na, [(_load(loaders["exact"], arrays, ws), 1)])
    assert b.StreamKernelName(0) == NAME
    x = O.signal_noise(BLOCK * 8, seed=8)
    y = _blocks(b, x)
    assert b.StreamRangeEvents(0) == 0
    b.close()
    yo = O.OracleWaveNet(arrays, ws).process(x)
    assert np.all(np.isfinite(yo)) and O.rms(yo) > 0
    _ratio(y, yo, ref_np.wavenet_forward(arrays, ws, x)[0], (name, scaling))


@pytest.mark.parametrize("name", ["32/8 tanh", "128/64 tanh"])
def test_an_input_beyond_every_default_limit_is_not_clamped(na, loaders, name):
    arrays, w = WC.range_model(name)
    b = _batch(na, [(_load(loaders["exact"], arrays, w), 1), (_load(loaders["default"], arrays, w), 1)])
    assert b.StreamKernelName(0) == NAME and b.StreamKernelName(1) != NAME
    assert np.isinf(b.StreamInputLimit(0)) and b.StreamInputLimit(1) <= 32752.0
    x = (1e5 * O.signal_noise(1024, 5)).astype(np.float32)
    y = _run(b, np.stack([x, x]), [BLOCK] * 8)
    assert b.StreamRangeEvents(0) == 0
    b.close()
    _ratio(y[0], O.OracleWaveNet(arrays, w).process(x), ref_np.wavenet_forward(arrays, w, x)[0], (name, "1e5 x noise"))
    assert not np.array_equal(y[0], y[1])  # the default stream was clamped


@pytest.mark.parametrize("channels", [24, 65])
def test_more_streams_than_cus_and_streams_that_leave(na, loaders, num_cus, channels):
    arrays = WC.chain([channels], [([3, 2], [1, 64])])
    w = O.synth_wavenet_weights(arrays, seed=channels)
    streams = num_cus + 4
    b = _batch(na, [(_load(loaders["exact"], arrays, w), streams)])
    assert b.StreamKernelName(streams - 1) == NAME
    x5 = np.stack([O.signal_noise(3 * BLOCK + 37, 30 + s) for s in range(5)])
    x = x5[np.arange(streams) % 5]
    yo = [O.OracleWaveNet(arrays, w).process(x5[s]) for s in range(5)]
    cut = 2 * BLOCK
    y = _run(b, x[:, :cut], [BLOCK, BLOCK])
    sampled = (0, streams // 3, (2 * streams) // 3, streams - 1)
    for s in sampled:
        _assert_parity(y[s], yo[s % 5][:cut], (channels, s))
    for s in range(5, streams):
        assert np.array_equal(y[s], y[s % 5]), (channels, s)
    gone = (streams // 2, streams // 2 + 2)
    for s in gone:
        b.RemoveStreams(s)
    y2 = _run(b, x[:, cut:], [BLOCK, 37])  # the live rows are no longer contiguous: the index lists
    b.close()
    for s in sampled + (streams // 2 + 1,):
        _assert_parity(np.concatenate([y[s], y2[s]]), yo[s % 5], (channels, s, "after RemoveStreams"))
    assert not np.any(y2[list(gone)])


def test_both_kinds_of_group_and_a_narrow_model_share_a_batch(na, loaders):
    arrays = WC.two_array(40, 20)
    w = O.synth_wavenet_weights(arrays, seed=40)
    std = loaders["default"].CreateFromFile(os.path.join(O.MODELS_DIR, "BossWN-standard.nam"))
    b = _batch(na, [(_load(loaders["exact"], arrays, w), 2), (_load(loaders["default"], arrays, w), 2), (std, 2)])
    assert [b.StreamKernelName(s) for s in (0, 2, 4)] == [NAME, "WaveNetGenericKernel", "WaveNetSpecKernel"]
    x = np.stack([O.signal_noise(2 * BLOCK + 37, 70 + s) for s in range(6)])
    y = _run(b, x, [BLOCK, 37, BLOCK])
    b.close()
    for s in range(6):
        ora = O.OracleWaveNet(arrays, w) if s < 4 else O.oracle_from_file("BossWN-standard.nam")
        _assert_parity(y[s], ora.process(x[s]), s)
