"""Gated WaveNet layer arrays (A1 key "gated") on the gated instantiations of the f32 frame kernel (wavenet_frame_kernels.hip:
LayerFrGated), against the float64 restatement of tests/gated_cases.py.  Parity is test_gpu_frame.py's rule: every 32-frame window
within 2e-6 RMS relative to max(1, level); tests/test_gated_cpu.py shows that float32 itself stays within half of that.  Every batch
asserts the kernel name before its output is trusted.  No trained gated capture was available: every gated model is synthetic."""
import os

import numpy as np
import pytest

import frame_cases as FC
import gated_cases as GC
import na_oracle as O

pytestmark = pytest.mark.gpu
KERNEL, BLOCK = "WaveNetFrameKernel", 128


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


def _load(na, case, w=None):
    ld = na.NeuralModelLoader()
    if case["std"]:
        ld.SetWaveNetMathMode(na.EMathMode.StdMath)
    return ld.CreateFromString(GC.nam_json(case["arrays"], GC.weights(case) if w is None else w), ".nam")


def _batch(na, m, streams=1):
    b = na.Batch(0)
    assert b.AddStreams(m, streams) == 0
    assert b.StreamKernelName(0) == KERNEL and b.StreamKernelName(streams - 1) == KERNEL, b.StreamKernelName(0)
    return b


def _run(batch, x, sizes, close=True):
    cuts = np.minimum(np.cumsum([0] + list(sizes)), x.shape[1])
    y = np.concatenate([batch.Process(np.ascontiguousarray(x[:, a:b])) for a, b in zip(cuts[:-1], cuts[1:]) if b > a], axis=1)
    assert y.shape == x.shape
    if close:
        batch.close()
    return y


def _assert_parity(y, case, x, what):
    ref = GC.forward(case["arrays"], GC.weights(case), x, np.float64, case["std"])
    assert y.shape == ref.shape and np.all(np.isfinite(y)) and O.rms(ref) > 1e-5, (what, O.rms(ref))  # (a silent model cannot pass)
    worst = GC.worst_window(y.astype(np.float64), ref)
    print("%s: worst window %.3g of the bound, level %.3g" % (what, worst, O.rms(ref)))
    assert worst < 1.0, (what, worst)


@pytest.mark.parametrize("case", GC.CASES, ids=[c["name"] for c in GC.CASES])
def test_gated_layers_match_the_float64_restatement_whatever_the_call_sizes(na, case):
    """128-sample calls (two waves, register prefetch) and one sample followed by 37-sample calls (one wave, no prefetch): both within
    the bound, and bit-identical."""
    m, x = _load(na, case), O.signal_noise(GC.SAMPLES, seed=case["seed"])
    assert m.IsGated()
    ys = [_run(_batch(na, m), x[None, :], sizes)[0] for sizes in ([BLOCK] * 4, [1] + [37] * 11)]
    for y in ys:
        _assert_parity(y, case, x, case["name"])
    assert np.array_equal(ys[0], ys[1]), (case["name"], float(np.abs(ys[0] - ys[1]).max()))


@pytest.mark.parametrize("std", [False, True], ids=["fastmath", "stdmath"])
@pytest.mark.parametrize("channels", [16, 6])
def test_a_zero_gate_half_equals_the_plain_kernel_with_halved_1x1_and_head_bit_for_bit(na, channels, std):
    """Gate weights, bias and mix-in zero: the sigmoid is exactly 0.5, so z is half the plain layer's z, which the plain model takes
    back with halved 1x1 and head weights (a power of two commutes with every f32 sum; nothing here is subnormal).  One array: a
    second array's head sum would add unscaled and scaled terms; K = 2: what lands a plain model on the frame kernel by default.  Pins
    the filter half's operand layout to the verified plain path."""
    gated = GC.case("zero-gate", [channels], 2, GC.LONG, 20 + channels, std=std)
    plain = GC.case("plain", [channels], 2, GC.LONG, 0, gated=[False], std=std)
    wg, wp, c = GC.weights(gated), GC.weights(plain), channels
    (rg, lg, hg, bg), (rp, lp, hp, bp) = GC.unpack(gated["arrays"], wg)[0][0], GC.unpack(plain["arrays"], wp)[0][0]
    rp[...], hp[...], bp[...], wp[-1] = rg, hg * np.float32(0.5), bg, wg[-1]
    for (wc, bc, wm, w1, b1), (pc, pb, pm, p1, pb1) in zip(lg, lp):
        wc[c:], bc[c:], wm[c:] = 0.0, 0.0, 0.0
        pc[...], pb[...], pm[...], p1[...], pb1[...] = wc[:c], bc[:c], wm[:c], w1 * np.float32(0.5), b1
    assert np.all(np.abs(wp) > 1e-30)
    x = O.signal_noise(GC.SAMPLES, seed=gated["seed"])
    yg, yp = (_run(_batch(na, _load(na, cs, w)), x[None, :], [BLOCK, 37, 64, BLOCK, BLOCK])[0] for cs, w in ((gated, wg), (plain, wp)))
    assert O.rms(yg) > 1e-3 and np.array_equal(yg, yp), float(np.abs(yg - yp).max())


def test_streams_that_share_a_workgroup_compute_what_a_stream_alone_computes(na):
    """Batches of 1, 2 and 3 streams, and of 512 and 513 -- from 512 on two streams share a workgroup and its staged weights, 513 leave the
    last workgroup half filled: every row a batch shares with another is bit-identical (rows repeat with period 3)."""
    case = GC.CASES[0]
    m, base = _load(na, case), np.stack([O.signal_noise(2 * BLOCK + 37, seed=70 + r) for r in range(3)])
    outs = {n: _run(_batch(na, m, n), base[np.arange(n) % 3], [BLOCK, 37, BLOCK]) for n in (1, 2, 3, 512, 513)}
    _assert_parity(outs[3][2], case, base[2], "stream 2 of 3")
    for n, y in outs.items():
        assert all(np.array_equal(y[s], outs[3][s % 3]) for s in range(n)), n


def test_plain_models_of_a_batch_with_a_gated_model_compute_what_they_compute_without_it(na):
    """A plain frame-kernel model shares its fused launch -- then a gated instantiation -- with the gated model; BossWN-nano runs
    packed on the f16-split kernels beside it.  Their rows are bit-identical to a batch without the gated model."""
    pc = FC.small_k2_model()
    plain = na.NeuralModelLoader().CreateFromString(O.nam_json_wavenet_generic(pc["arrays"], FC.weights(pc)), ".nam")
    nano = na.NeuralModelLoader().CreateFromFile(os.path.join(os.path.dirname(__file__), "golden", "models", "BossWN-nano.nam"))
    gated = _load(na, GC.CASES[0])
    x = np.stack([O.signal_noise(2 * BLOCK + 37, seed=80 + r) for r in range(8)])
    outs = []
    for models, rows in (([gated, plain, nano, gated], slice(0, 8)), ([plain, nano], slice(2, 6))):
        b = na.Batch(0)
        first = [b.AddStreams(m, 2) for m in models]
        names = [b.StreamKernelName(s) for s in first]
        assert [n == KERNEL for n in names] == [m is not nano for m in models], names
        outs.append(_run(b, x[rows], [BLOCK, 37, BLOCK]))
    _assert_parity(outs[0][0], GC.CASES[0], x[0], "gated row beside plain models")
    assert O.rms(outs[1]) > 1e-4 and np.array_equal(outs[0][2:6], outs[1])


def test_the_largest_gated_kernel_size_runs_short_and_long_buffers(na):
    """16 gated channels, K = 35: 162 432 bytes of LDS with 128-frame blocks, the largest that loads (K = 36 is refused at load,
    tests/test_gated_cpu.py); a 1-sample and a 128-sample buffer on two streams."""
    case = GC.case("lds-k35", [16], GC.MAX_K16, [1], 75)
    x = np.stack([O.signal_noise(1 + BLOCK, seed=75 + r) for r in range(2)])
    y = _run(_batch(na, _load(na, case), 2), x, [1, BLOCK])
    for s in range(2):
        _assert_parity(y[s], case, x[s], (case["name"], s))


def test_offline_rendering_and_snapshots_of_a_gated_model_equal_the_sequential_run(na):
    """The plan-driven paths: render_offline of 3 000 samples equals the sequential run bit for bit; a stream saved after 200 samples
    and loaded into a fresh batch continues bit-identically."""
    case = GC.CASES[0]
    m, x = _load(na, case), O.signal_noise(3000, seed=90)
    b = _batch(na, m)
    head = _run(b, x[None, :200], [BLOCK] * 2, close=False)
    blob = b.SaveStreams(0)
    y = np.concatenate([head, _run(b, x[None, 200:], [BLOCK] * 22)], axis=1)[0]
    _assert_parity(y[:GC.SAMPLES], case, x[:GC.SAMPLES], "sequential")
    assert np.array_equal(na.render_offline(m, x), y)
    b2 = _batch(na, m)
    b2.LoadStreams(0, blob)
    assert np.array_equal(_run(b2, x[None, 200:], [BLOCK] * 22)[0], y[200:])
