"""Gated layer arrays wider than 16 channels on the gated instantiations of WaveNetWideF32Kernel (csrc/wavenet_wide_f32_kernels.hip,
models of a loader with SetWaveNetWideGated(True)) against the float64 restatement of tests/gated_cases.py.  Parity is test_gpu_gated.py's
rule: every 32-frame window within 2e-6 RMS relative to max(1, level).  Every batch asserts the kernel name before its output is trusted."""
import os

import numpy as np
import pytest

import gated_cases as GC
import na_oracle as O
from test_gpu_wide import BLOCK, FORCED, _run, na, num_cus  # noqa: F401 (fixtures)
from test_wide_gated_cpu import WIDE, load, loader

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(FORCED, reason="forced kernel family")]
NAME = "WaveNetWideF32Kernel"


def _ref(case, x):
    return GC.forward(case["arrays"], GC.weights(case), x, np.float64, case["std"])


def _gated_batch(na, m, streams=1):
    b = na.Batch(0)
    b.AddStreams(m, streams)
    assert b.StreamKernelName(0) == NAME and b.StreamKernelName(streams - 1) == NAME and np.isinf(b.StreamInputLimit(0))
    return b


def _assert_parity(y, ref, what):
    assert y.shape == ref.shape and np.all(np.isfinite(y)) and O.rms(ref) > 1e-5, (what, O.rms(ref))  # (a silent model cannot pass)
    worst = GC.worst_window(y.astype(np.float64), ref)
    print("%s: worst window %.3g of the bound, level %.3g" % (what, worst, O.rms(ref)))
    assert worst < 1.0, (what, worst)


@pytest.mark.parametrize("case", WIDE, ids=[c["name"] for c in WIDE])
def test_wide_gated_layers_match_the_float64_restatement_whatever_the_call_sizes(na, case):
    m, x = load(loader(std=case["std"]), case, prewarm=True), O.signal_noise(GC.SAMPLES, seed=case["seed"])
    assert m.IsGated()
    ys, ref = [], _ref(case, x)
    for sizes in ([BLOCK] * 4, [1] + [37] * 11):
        b = _gated_batch(na, m)
        ys.append(_run(b, x[None, :], sizes)[0])
        assert b.StreamRangeEvents(0) == 0
        b.close()
        _assert_parity(ys[-1], ref, case["name"])
    assert np.array_equal(ys[0], ys[1]), (case["name"], float(np.abs(ys[0] - ys[1]).max()))


@pytest.mark.parametrize("std", [False, True], ids=["fastmath", "stdmath"])
@pytest.mark.parametrize("channels", [24, 64])
def test_a_zero_gate_half_equals_the_plain_wide_kernel_with_halved_1x1_and_head_bit_for_bit(na, channels, std):
    """test_gpu_gated.py's construction (sigmoid exactly 0.5, taken back by halved 1x1 and head weights), the plain model on the plain
    WaveNetWideF32Kernel through SetWaveNetExactF32: pins the filter half's image rows and accumulators to the plain path."""
    gated = GC.case("zero-gate", [channels], 3, GC.LONG, 20 + channels, std=std)
    plain = GC.case("plain", [channels], 3, GC.LONG, 0, gated=[False], std=std)
    wg, wp, c = GC.weights(gated), GC.weights(plain), channels
    (rg, lg, hg, bg), (rp, lp, hp, bp) = GC.unpack(gated["arrays"], wg)[0][0], GC.unpack(plain["arrays"], wp)[0][0]
    rp[...], hp[...], bp[...], wp[-1] = rg, hg * np.float32(0.5), bg, wg[-1]
    for (wc, bc, wm, w1, b1), (pc, pb, pm, p1, pb1) in zip(lg, lp):
        wc[c:], bc[c:], wm[c:] = 0.0, 0.0, 0.0
        pc[...], pb[...], pm[...], p1[...], pb1[...] = wc[:c], bc[:c], wm[:c], w1 * np.float32(0.5), b1
    assert np.all(np.abs(wp) > 1e-30)
    x, ys = O.signal_noise(GC.SAMPLES, seed=gated["seed"]), []
    for cs, w, ld in ((gated, wg, loader(std=std)), (plain, wp, loader(wide=False, exact=True, std=std))):
        m = ld.CreateFromString(GC.nam_json(cs["arrays"], w), ".nam")
        assert m.IsGated() == (cs is gated)
        b = _gated_batch(na, m)
        ys.append(_run(b, x[None, :], [BLOCK, 37, 64, BLOCK, BLOCK])[0])
        b.close()
    assert O.rms(ys[0]) > 1e-3 and np.array_equal(ys[0], ys[1]), float(np.abs(ys[0] - ys[1]).max())


def test_more_streams_than_cus_and_streams_that_leave(na, num_cus):
    """five distinct inputs repeated: sampled rows within the bound, repeated rows bit-identical; the index-list launch once two left"""
    case, streams = WIDE[1], num_cus + 4
    b = _gated_batch(na, load(loader(), case, prewarm=True), streams)
    x5 = np.stack([O.signal_noise(3 * BLOCK + 24, 30 + s) for s in range(5)])
    x, cut = x5[np.arange(streams) % 5], 2 * BLOCK
    y = _run(b, x[:, :cut], [BLOCK, BLOCK])
    gone = (streams // 2, streams // 2 + 2)
    for s in gone:
        b.RemoveStreams(s)
    y = np.concatenate([y, _run(b, x[:, cut:], [BLOCK, 24])], axis=1)
    b.close()
    for s in (0, streams // 3, streams // 2 + 1, streams - 1):
        _assert_parity(y[s], _ref(case, x5[s % 5]), (case["name"], s))
    assert all(np.array_equal(y[s], y[s % 5]) for s in range(streams) if s not in gone) and not np.any(y[list(gone), cut:])


def test_wide_gated_narrow_gated_exact_f32_and_standard_groups_share_a_batch(na):
    wide, narrow, plain = WIDE[6], GC.CASES[0], GC.case("plain-40-20", [40, 20], 3, [1, 64], 41, gated=[False, False])
    models = [load(loader(), wide, True), load(loader(), narrow, True), load(loader(wide=False, exact=True), plain, True),
              loader(wide=False).CreateFromFile(os.path.join(O.MODELS_DIR, "BossWN-standard.nam"))]
    b = na.Batch(0)
    assert [b.StreamKernelName(b.AddStreams(m, 2)) for m in models] == [NAME, "WaveNetFrameKernel", NAME, "WaveNetSpecKernel"]
    x = np.stack([O.signal_noise(2 * BLOCK + 37, 70 + s) for s in range(8)])
    y = _run(b, x, [BLOCK, 37, BLOCK])
    b.close()
    for s, case in zip(range(6), (wide, wide, narrow, narrow, plain, plain)):
        _assert_parity(y[s], _ref(case, x[s]), (case["name"], s))
    for s in (6, 7):
        yo = O.oracle_from_file("BossWN-standard.nam").process(x[s])
        assert O.rms(y[s] - yo) < 2e-6 * max(1.0, O.rms(yo)), s


def test_a_saved_stream_continues_bit_identically_in_a_second_batch(na):
    case = WIDE[0]
    m, x = load(loader(), case, prewarm=True), O.signal_noise(GC.SAMPLES, seed=90)
    b = _gated_batch(na, m)
    head = _run(b, x[None, :200], [BLOCK] * 2)
    blob = b.SaveStreams(0)
    y = np.concatenate([head, _run(b, x[None, 200:], [BLOCK] * 2)], axis=1)[0]
    b.close()
    _assert_parity(y, _ref(case, x), "uninterrupted")
    b2 = _gated_batch(na, m)
    b2.LoadStreams(0, blob)
    assert np.array_equal(_run(b2, x[None, 200:], [BLOCK] * 2)[0], y[200:])
    b2.close()
