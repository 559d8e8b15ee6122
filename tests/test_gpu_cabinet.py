"""GPU tests of the cabinet stage (NA_BatchEnableCabinetStage / LoadIR / SetStreamIR, csrc/cabinet_stage.h): the
per-stream convolution of a row with an impulse response, behind the model launches and in front of the output stage.

Part 1 drives the stage through its hook (NA_DebugRunCabinetStage) on rows that stand in for model outputs; the expected value is
np.convolve in float64.  Integer taps in [-4, 4] and integer samples in [-8, 8] keep every partial sum below 2^24 (4096 * 4 * 8 = 2^17,
8192 taps: 2^18), so any f32 summation order is exact and the comparison is np.array_equal: these cases carry the structural proof.
Random floats are held to the forward bound of any f32 order, (K + 4) * 2^-24 * sum |h_k| |y_{t-k}| + 1e-30, and to twice the RMS error
of a sequential f32 sum.  Part 2 runs the twelve-row batch of tests/handover_cases.py beside its twin without the stage."""
import ctypes as C
import os

import numpy as np
import pytest

import cabinet_cases as K
import handover_cases as H

FORCED = bool(os.environ.get("NA_WN_KERNEL") or os.environ.get("NA_WN_PACK") or os.environ.get("NA_WN_SPEC") or os.environ.get("NA_SP_T")
              or os.environ.get("NA_SP_GEN") or os.environ.get("NA_WN_PAD"))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(FORCED, reason="forced kernel family")]

ROWS = 5
EXACT_K = [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4096]


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


@pytest.fixture(scope="module")
def models(na):
    return H.load_models(na)


@pytest.fixture(scope="module")
def launches():
    from neuralaudio_amd import capi
    return capi.load_library().NA_DebugCabinetLaunches


def odd(n):
    return n + 3


def aligned(n):
    return (n + 3) // 4 * 4


# ================================================================================================ 1: through the hook

@pytest.mark.parametrize("max_taps", [4096, 8192])
def test_exact_cases(na, models, launches, max_taps):
    """Integer taps and rows: rows 0, 2 and 3 carry IRs of K taps (rows 0 and 3 share one), rows 1 and 4 keep their bits.  Every K on
    the same batch, one after the other; each starts from a dry row (T0 = the set call) and runs as three ragged calls.  Once with
    maxTaps = 4096 and once with 8192, where K = maxTaps is added: the same values whatever maxTaps is."""
    rng = np.random.default_rng(11)
    hb = K.HookBatch(na, models[H.NANO], ROWS, max_taps)
    info = hb.b.CabinetInfo()
    assert info["maxTaps"] == max_taps and info["ringSamples"] & (info["ringSamples"] - 1) == 0
    assert info["ringSamples"] >= max_taps - 1 + info["pieceSamples"] and info["deviceBytes"] >= ROWS * info["ringSamples"] * 4
    total = 700
    for taps in EXACT_K + ([max_taps] if max_taps not in EXACT_K else []):
        h1, h2 = K.integers(rng, taps, 4), K.integers(rng, taps, 4)
        h1[-1], h2[-1] = 3.0, -2.0  # (the last tap counts)
        a, b = hb.b.LoadIR(h1), hb.b.LoadIR(h2)
        x = K.integers(rng, (ROWS, total), 8)
        x[1, 5] = np.float32(-0.0)
        for s, ir in ((0, a), (2, b), (3, a)):
            hb.b.SetStreamIR(s, ir, 0)
            assert hb.b.GetStreamIR(s) == ir
        before = launches()
        y = hb.run(x, [300, 1, 399], stride=odd)
        assert launches() - before == 6, "two launches per piece"
        for s, h in ((0, h1), (2, h2), (3, h1)):
            assert np.array_equal(y[s].astype(np.float64), K.conv64(h, x[s])), (taps, s)
        assert K.same_bits(y[1], x[1]) and K.same_bits(y[4], x[4]), taps
        for s in (0, 2, 3):
            hb.b.SetStreamIR(s, -1, 0)
        hb.b.UnloadIR(a)
        hb.b.UnloadIR(b)
    assert hb.b.CabinetInfo()["numIRs"] == 0
    hb.close()


def test_delta_irs(na, models):
    """{1} is the identity and e_k a pure delay of k samples, on random floats, exactly."""
    rng = np.random.default_rng(12)
    hb = K.HookBatch(na, models[H.NANO], ROWS, 2048)
    x = rng.standard_normal((ROWS, 900)).astype(np.float32)
    delays = {0: 0, 1: 1, 2: 127, 3: 1024, 4: 2047}
    for s, d in delays.items():
        e = np.zeros(d + 1, np.float32)
        e[d] = 1.0
        hb.b.SetStreamIR(s, hb.b.LoadIR(e), 0)
    y = hb.run(x, [129, 471, 300], stride=aligned)
    for s, d in delays.items():
        expect = np.concatenate([np.zeros(d, np.float32), x[s]])[:900]
        assert np.array_equal(y[s], expect), (s, d)
    hb.close()


def test_switches_without_a_fade_are_exact(na, models):
    """N = 0 between two IRs: B from the first sample after the call, on the history A saw (integers: exact); to dry and back: a new T0."""
    rng = np.random.default_rng(13)
    hb = K.HookBatch(na, models[H.NANO], ROWS, 512)
    hA, hB = K.integers(rng, 300, 4), K.integers(rng, 77, 4)
    a, b = hb.b.LoadIR(hA), hb.b.LoadIR(hB)
    x = K.integers(rng, (ROWS, 1200), 8)
    hb.b.SetStreamIR(2, a, 0)
    y1 = hb.run(x[:, :400], [400])
    hb.b.SetStreamIR(2, b, 0)
    y2 = hb.run(x[:, 400:800], [17, 383])
    assert np.array_equal(y1[2], K.conv64(hA, x[2])[:400]) and np.array_equal(y2[2], K.conv64(hB, x[2])[400:800])
    hb.b.SetStreamIR(2, -1, 0)
    assert hb.b.GetStreamIR(2) == -1
    y3 = hb.run(x[:, 800:900], [100])
    assert K.same_bits(y3, x[:, 800:900])
    hb.b.SetStreamIR(2, a, 0)
    y4 = hb.run(x[:, 900:], [300])
    assert np.array_equal(y4[2], K.conv64(hA, x[2, 900:])), "the history starts empty at the new T0"
    hb.close()


@pytest.mark.parametrize("taps", [5, 129, 1000, 4096])
def test_random_floats_stay_within_the_forward_bound(na, models, taps):
    """|err| <= (K + 4) * 2^-24 * sum |h_k| |y_{t-k}| + 1e-30, and an RMS error of at most twice a sequential f32 sum's."""
    rng = np.random.default_rng(14 + taps)
    hb = K.HookBatch(na, models[H.NANO], ROWS, 4096)
    n = 2 * taps + 300
    h = (rng.standard_normal(taps) * np.exp(-np.arange(taps) / (0.3 * taps))).astype(np.float32)
    x = (0.25 * rng.standard_normal((ROWS, n))).astype(np.float32)
    ir = hb.b.LoadIR(h)
    for s in (0, 3):
        hb.b.SetStreamIR(s, ir, 0)
    y = hb.run(x, H.ragged(n), stride=odd)
    for s in (0, 3):
        ref = K.conv64(h, x[s])
        err = np.abs(y[s] - ref)
        limit = K.conv_bound(h, x[s])
        assert np.all(err <= limit), (s, int(np.argmax(err - limit)), float(np.max(err / limit)))
        seq = K.sequential_f32(h, x[s])
        ours, theirs = float(np.sqrt(np.mean((y[s] - ref) ** 2))), float(np.sqrt(np.mean((seq - ref) ** 2)))
        print("K=%d row %d: rms error %.3g, sequential f32 %.3g, ratio %.3f; largest error %.4f of the bound"
              % (taps, s, ours, theirs, ours / theirs, float(np.max(err / limit))))
        assert ours <= 2.0 * theirs
    assert K.same_bits(y[1], x[1])
    hb.close()


def test_the_cut_into_calls_and_the_stride_never_show(na, models):
    """1500 samples as one call, in RAGGED lengths with odd strides, and in RAGGED lengths with 16-byte aligned strides: the same
    bits.  Random floats, IRs of 1000 and 3 taps, one of them on two rows (the number of entries differs from the fourth run, where a
    single row has an IR)."""
    rng = np.random.default_rng(15)
    h1, h2 = rng.standard_normal(1000).astype(np.float32), rng.standard_normal(3).astype(np.float32)
    x = rng.standard_normal((ROWS, 1500)).astype(np.float32)
    assert H.RAGGED == [1, 15, 17, 64, 128, 129, 300]
    outs = []
    for calls, stride, rows in (([1500], aligned, (0, 1, 4)), (H.ragged(1500), odd, (0, 1, 4)), (H.ragged(1500), aligned, (0, 1, 4)), (H.ragged(1500), odd, (1,))):
        hb = K.HookBatch(na, models[H.NANO], ROWS, 1024 if len(rows) > 1 else 2048)
        a, b = hb.b.LoadIR(h1), hb.b.LoadIR(h2)
        for s in rows:
            hb.b.SetStreamIR(s, b if s == 4 else a, 0)
        outs.append(hb.run(x, calls, stride=stride))
        hb.close()
    for y in outs[1:3]:
        assert np.array_equal(y, outs[0])
    assert np.array_equal(outs[3][1], outs[0][1]), "row 1 alone, maxTaps 2048: the same values"
    assert K.same_bits(outs[0][2], x[2]) and K.same_bits(outs[3][0], x[0])
    assert np.all(np.abs(outs[0][0] - K.conv64(h1, x[0])) <= K.conv_bound(h1, x[0]))


@pytest.mark.parametrize("max_taps", [64, 8192])
def test_ring_wrap(na, models, max_taps):
    """More than four times ringSamples samples through a K = maxTaps IR, in calls longer than a piece and ragged ones: exact."""
    rng = np.random.default_rng(16)
    hb = K.HookBatch(na, models[H.NANO], ROWS, max_taps)
    ring = hb.b.CabinetInfo()["ringSamples"]
    piece = hb.b.CabinetInfo()["pieceSamples"]
    total = 4 * ring + 777
    h = K.integers(rng, max_taps, 4)
    h[-1] = 1.0
    x = K.integers(rng, (ROWS, total), 8)
    hb.b.SetStreamIR(1, hb.b.LoadIR(h), 0)
    calls, left = [], total
    for n in [piece + 1, 3 * piece + 5, 100, ring - 1, ring + 1] * 8:
        if left == 0:
            break
        calls.append(min(n, left))
        left -= calls[-1]
    assert left == 0
    y = hb.run(x, calls, stride=odd)
    assert np.array_equal(y[1].astype(np.float64), K.conv64(h, x[1]))
    assert K.same_bits(y[0], x[0])
    hb.close()


@pytest.mark.parametrize("N", [1, 64, 129, 1000])
def test_fades(na, models, N):
    """dry -> A, A -> B and A -> dry with cuts inside the fade.  During a fade the row lies within the two convolution bounds weighted
    by (1 - w) and w plus three roundings; from the sample after it on it equals, bit for bit, a row that had the target since the same
    T0 (row 3: A since T0 of the first fade, then B by a switch without a fade)."""
    rng = np.random.default_rng(17 + N)
    hA = (rng.standard_normal(700) * np.exp(-np.arange(700) / 150.0)).astype(np.float32)
    hB = (rng.standard_normal(130) * np.exp(-np.arange(130) / 40.0)).astype(np.float32)
    seg = N + 450
    x = (0.25 * rng.standard_normal((ROWS, 3 * seg))).astype(np.float32)
    x[3] = x[0]
    hb = K.HookBatch(na, models[H.NANO], ROWS, 1024)
    ids = {"A": hb.b.LoadIR(hA), "B": hb.b.LoadIR(hB)}
    cab = K.CabContract(ROWS, {"A": hA, "B": hB})
    steps = [("A", "A"), ("B", "B"), (None, None)]  # (row 0 fades to, row 3 switches to)
    worst, pos = 0.0, 0
    for fade_to, switch_to in steps:
        hb.b.SetStreamIR(0, -1 if fade_to is None else ids[fade_to], N)
        cab.set_ir(0, fade_to, N)
        hb.b.SetStreamIR(3, -1 if switch_to is None else ids[switch_to], 0)
        cab.set_ir(3, switch_to, 0)
        assert hb.b.IRFadeRemaining(0) == N and hb.b.IRFadeRemaining(3) == 0
        with pytest.raises(na.NeuralAudioError, match="an IR fade of stream 0 is running"):
            hb.b.SetStreamIR(0, ids["A"], 0)
        with pytest.raises(na.NeuralAudioError, match="in use"):
            hb.b.UnloadIR(ids["A"] if fade_to == "A" else ids["B"])  # (the target, or the IR the row fades from)
        done = 0
        for n in H.ragged(seg):
            xs = x[:, pos:pos + n]
            y = hb.run(xs, [n], stride=odd)
            e, bound, exact = cab.step(xs)
            for s in range(ROWS):
                if exact[s]:
                    assert K.same_bits(y[s], xs[s]), (fade_to, s)
                else:
                    err = np.abs(y[s] - e[s])
                    worst = max(worst, float(np.max(err / bound[s])))
                    assert np.all(err <= bound[s]), (fade_to, s, done, int(np.argmax(err - bound[s])), float(np.max(err / bound[s])))
            # behind the fade's last sample: the row that had the target all along
            after = np.arange(done, done + n) >= N - 1
            assert np.array_equal(y[0][after], y[3][after]), (fade_to, done)
            done += n
            pos += n
            assert hb.b.IRFadeRemaining(0) == max(N - done, 0)
        assert hb.b.GetStreamIR(0) == (-1 if fade_to is None else ids[fade_to])
    print("fades N=%d: largest error %.4f of the bound" % (N, worst))
    hb.b.UnloadIR(ids["A"])
    hb.b.UnloadIR(ids["B"])
    hb.close()


# ================================================================================================ 2: with models

def _irs(seed=0):
    rng = np.random.default_rng(100 + seed)
    mk = lambda taps, tau: (rng.standard_normal(taps) * np.exp(-np.arange(taps) / tau) * 0.3).astype(np.float32)
    return {"cabA": mk(200, 40.0), "cabB": mk(131, 30.0), "short": mk(3, 2.0)}


PATHS = ("process", "registered", "submit", "device", "device-odd")


def test_off_is_off(na, models, launches):
    """The stage is enabled, IRs are loaded and no stream has one: every path gives the twin's bits and launches none of the stage's
    kernels."""
    calls = [128, 17, 300, 128]
    x = H.signal(sum(calls), 21)
    before = launches()
    for path in PATHS:
        y, yt, _ = K.run_scenario(na, models, x, calls, {}, _irs(), path=path)
        assert np.array_equal(y, yt), path
        assert np.any(y[0]) and np.any(y[4]) and np.any(y[8]) and not np.any(y[2])
    assert launches() == before


def test_off_is_off_for_the_half_batch_launches(na, models, launches):
    """512 A1 Standard streams on the batch's own stream, device pointers: with the stage enabled and no IR the free-running mode
    engages as in the twin and the bits are the twin's; an IR on one stream orders the launches; cleared again, the mode comes back."""
    import torch
    dev = torch.device("cuda", 0)
    S, n = 512, 128
    x = np.stack([H.noise(4 * n, 60 + r) for r in range(5)])[np.arange(S) % 5]
    dx = torch.from_numpy(x).to(dev)
    torch.cuda.synchronize(dev)
    halves, outs = {}, {}
    h = _irs()["cabA"]
    for stage in (True, False):
        b = na.Batch(0)
        assert b.ReserveStreams(models[H.STD], S) == 0
        for s in range(S):
            b.ActivateStream(s, 1.0)
        if stage:
            b.EnableCabinetStage(256)
            ir = b.LoadIR(h)
        dy = torch.zeros(S, 4 * n, device=dev)
        before = launches()
        for k in range(4):
            if stage and k == 2:
                b.SetStreamIR(7, ir, 0)
            if stage and k == 3:
                b.SetStreamIR(7, -1, 0)
            b.ProcessDevice(dx.data_ptr() + 4 * k * n, dy.data_ptr() + 4 * k * n, n, 4 * n, 4 * n)
            b.Synchronize()
            halves[(stage, k)] = b.UsesHalfLaunches()
        assert launches() - before == (2 if stage else 0)
        outs[stage] = dy.cpu().numpy()
        b.close()
    assert halves[(True, 0)] == halves[(False, 0)] and halves[(True, 1)] == halves[(False, 1)]
    print("half-batch launches: twin %s, with the stage and an IR %s, cleared again %s" % (halves[(False, 1)], halves[(True, 2)], halves[(True, 3)]))
    assert not halves[(True, 2)] and halves[(True, 3)] == halves[(False, 3)]
    keep = np.ones(outs[True].shape, bool)
    keep[7, 2 * n:3 * n] = False
    assert np.array_equal(outs[True][keep], outs[False][keep])
    seg = slice(2 * n, 3 * n)
    ref = K.conv64(h, outs[False][7, seg])
    assert np.all(np.abs(outs[True][7, seg] - ref) <= K.conv_bound(h, outs[False][7, seg]))


@pytest.mark.parametrize("path", PATHS)
def test_irs_on_one_stream_of_each_family(na, models, path):
    """IRs on rows 0 (packed nano), 4 (Standard) and 9 (LSTM), one shared, set in front of call 1; a fade to another IR on row 4 and to
    dry on row 9 later.  Every other row -- the packed neighbours of row 0 among them -- keeps the twin's bits in every call."""
    calls = [128, 100, 128, 17, 300, 128, 128]
    x = H.signal(sum(calls), 22)
    ops = {1: [("ir", 0, "cabA", 0), ("ir", 4, "cabA", 64), ("ir", 9, "short", 0)],
           3: [("ir", 4, "cabB", 129), ("ir", 9, None, 200)]}
    seen = {}

    def hook(b, cab, outc, i):
        seen[i] = (b.GetStreamIR(9), b.IRFadeRemaining(4), b.IRFadeRemaining(9))

    y, yt, worst = K.run_scenario(na, models, x, calls, ops, _irs(), path=path, hook=hook)
    print("IRs on (%s): largest error %.4f of the limit" % (path, worst))
    assert worst > 0.0
    assert seen[1][1] == 0 and seen[3] == (-1, 129 - 17, 200 - 17) and seen[4] == (-1, 0, 0)
    tail = sum(calls[:5])
    assert np.array_equal(y[9, tail:], yt[9, tail:]), "faded to dry: the twin's bits again"
    for s in (1, 5, 8):
        assert np.array_equal(y[s], yt[s])


def test_with_the_output_stage(na, models):
    """A gain ramp on a row with an IR, and a hand-over between two rows that both have IRs (the host sets `to`'s right behind the
    hand-over): every row is convolved with its own IR first, then scaled and cross-faded."""
    calls = H.ragged(1300)
    f, t = 4, 2  # Standard -> packed nano
    x = H.signal(sum(calls), 23, same=[(f, t)])
    ops = {1: [("ir", f, "cabA", 0), ("ir", 8, "cabB", 0), ("gain", 8, 0.3, 300)],
           4: [("handover", f, t, 257), ("ir", t, "cabB", 0), ("gain", t, 1.5, 0)],
           9: [("gain", 8, 1.0, 64)]}
    state = {}

    def hook(b, cab, outc, i):
        if b.IsParked(f) and "parked" not in state:
            state["parked"] = i
            assert b.GetStreamIR(f) == -1, "the park that ends a hand-over makes the stream dry"

    y, yt, worst = K.run_scenario(na, models, x, calls, ops, _irs(), out_stage=True, hook=hook)
    print("with the output stage: largest error %.4f of the limit" % worst)
    assert worst > 0.0 and "parked" in state and np.any(y[t, -100:])


def test_resampling_batch(na, models):
    """A 44.1 kHz resampling batch: the stage runs behind the down kernel, on the samples the caller sees."""
    calls = [128, 441, 100, 300]
    x = H.signal(sum(calls), 24)
    ops = {1: [("ir", 0, "cabA", 0), ("ir", 5, "cabB", 100), ("ir", 8, "short", 0)], 3: [("ir", 5, None, 0)]}
    y, yt, worst = K.run_scenario(na, models, x, calls, ops, _irs(), resample=44100)
    print("resampling: largest error %.4f of the limit" % worst)
    assert worst > 0.0 and np.array_equal(y[5, -300:], yt[5, -300:])


def test_both_stages_on_a_resampling_batch(na, models):
    """A 44.1 kHz resampling batch with both stages at work: an IR and a gain ramp on row 8, a hand-over from row 4 to row 2 whose fade
    ends on a call boundary of both cuts (the call behind it parks row 4 in both).  Once as calls of 128, 441, 100 and 300, once with
    each of those cut into RAGGED lengths: both within the helpers' bounds, and the same bits in every row."""
    segments = [128, 441, 100, 300]
    f, t = 4, 2  # Standard -> packed nano
    x = H.signal(sum(segments), 28, same=[(f, t)])
    at = {1: [("ir", 8, "cabB", 0), ("gain", 8, 0.3, 300), ("handover", f, t, segments[1])], 3: [("gain", 8, 1.0, 64), ("ir", 8, "cabA", 100)]}
    outs = []
    for cut in (lambda n: [n], H.ragged):
        calls, ops = [], {}
        for i, n in enumerate(segments):
            if i in at:
                ops[len(calls)] = at[i]
            calls += cut(n)
        state = {}

        def hook(b, cab, outc, i):
            if b.IsParked(f):
                state.setdefault("parked by the call at", sum(calls[:i]))

        y, yt, worst = K.run_scenario(na, models, x, calls, ops, _irs(), resample=44100, out_stage=True, hook=hook)
        print("both stages, resampling, %d calls: largest error %.4f of the limit" % (len(calls), worst))
        assert worst > 0.0 and np.any(y[t, -100:])
        assert state["parked by the call at"] == sum(segments[:2])
        outs.append(y)
    assert len(outs) == 2 and np.array_equal(outs[0], outs[1]), np.flatnonzero(np.any(outs[0] != outs[1], axis=1))


def test_ring_growth_keeps_the_histories(na, models):
    """Four Standard streams, an IR on row 1, two calls of 128; sixteen more streams take the rows past the rings' first capacity of 16,
    so the rings move to a larger block; two more calls.  Row 1 is, bit for bit, the row of a batch that had twenty streams all along,
    and (row 0 runs the same input dry) the convolution of its whole history, the samples from before the move included."""
    n, taps = 128, _irs()["cabA"]
    x = np.stack([H.noise(4 * n, 2900 + r) for r in range(20)])
    x[1] = x[0]
    rows = {}
    for grown in (True, False):
        b = na.Batch(0)
        assert b.AddStreams(models[H.STD], 4) == 0
        if not grown:
            assert b.AddStreams(models[H.STD], 16) == 4
        b.EnableCabinetStage(256)
        b.SetStreamIR(1, b.LoadIR(taps), 0)
        before = b.CabinetInfo()["deviceBytes"]
        out = []
        for k in range(4):
            if grown and k == 2:
                assert b.AddStreams(models[H.STD], 16) == 4
                info = b.CabinetInfo()
                assert info["deviceBytes"] > before and info["deviceBytes"] >= 20 * info["ringSamples"] * 4
            out.append(b.Process(x[:b.NumStreams(), k * n:(k + 1) * n])[:4])
        rows[grown] = np.concatenate(out, axis=1)
        b.close()
    assert np.array_equal(rows[True][0], rows[False][0]), "a dry row does not depend on the number of rows"
    assert np.array_equal(rows[True][1], rows[False][1])
    assert np.all(np.abs(rows[True][1] - K.conv64(taps, rows[True][0])) <= K.conv_bound(taps, rows[True][0]))


def test_park_and_reactivate(na, models):
    """A parked stream comes back dry; an IR set again starts from an empty history (the contract's T0 is the new set call)."""
    calls = [128, 128, 64, 128, 200, 128]
    x = H.signal(sum(calls), 25)
    ops = {1: [("ir", 4, "cabA", 0), ("ir", 0, "cabB", 300)], 2: [("park", 4), ("park", 0)], 3: [("activate", 4), ("activate", 0)],
           4: [("ir", 4, "cabA", 0)]}
    seen = {}

    def hook(b, cab, outc, i):
        seen[i] = (b.GetStreamIR(4) if not b.IsParked(4) else "parked", b.IRFadeRemaining(0) if not b.IsParked(0) else "parked")

    y, yt, worst = K.run_scenario(na, models, x, calls, ops, _irs(), hook=hook)
    assert seen[2] == ("parked", "parked") and seen[3] == (-1, 0) and seen[4][0] >= 0
    a = sum(calls[:3])
    assert np.array_equal(y[4, a:a + calls[3]], yt[4, a:a + calls[3]]) and np.array_equal(y[0, a:], yt[0, a:])


def test_rules(na, models):
    """Every rule fails with a message that names it."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    b = H.make_batch(na, models, stage=False)
    for call in (lambda: b.SetStreamIR(0, -1, 0), lambda: b.GetStreamIR(0), lambda: b.IRFadeRemaining(0), lambda: b.LoadIR(np.ones(4, np.float32)),
                 lambda: b.UnloadIR(0), lambda: b.CabinetInfo()):
        with pytest.raises(na.NeuralAudioError, match="cabinet stage not enabled"):
            call()
    assert lib.NA_BatchGetStreamIR(b._h, 0) <= -2 and lib.NA_BatchStreamIRFadeRemaining(b._h, 0) < 0
    for bad in (0, 8193, -5):
        with pytest.raises(na.NeuralAudioError, match=r"maxTaps must lie in \[1, 8192\]"):
            b.EnableCabinetStage(bad)
    b.EnableCabinetStage(256)
    b.EnableCabinetStage(256)
    b.EnableCabinetStage(100)  # idempotent for an equal or smaller maxTaps
    assert b.CabinetInfo()["maxTaps"] == 256
    with pytest.raises(na.NeuralAudioError, match=r"numTaps must lie in \[1, maxTaps\]"):
        b.LoadIR(np.ones(257, np.float32))
    with pytest.raises(na.NeuralAudioError, match=r"numTaps must lie in \[1, maxTaps\]"):
        b.LoadIR(np.ones(0, np.float32))
    with pytest.raises(na.NeuralAudioError, match="taps must be finite"):
        b.LoadIR(np.array([1.0, np.inf], np.float32))
    with pytest.raises(na.NeuralAudioError, match="taps must be finite"):
        b.LoadIR(np.array([np.nan], np.float32))
    a, c = b.LoadIR(np.ones(256, np.float32)), b.LoadIR(np.ones(2, np.float32))
    assert (a, c) == (0, 1) and b.CabinetInfo()["numIRs"] == 2
    b.UnloadIR(a)
    assert b.LoadIR(np.ones(7, np.float32)) == a, "ids of unloaded IRs are recycled"
    with pytest.raises(na.NeuralAudioError, match="IR 5 is not loaded"):
        b.SetStreamIR(0, 5, 0)
    with pytest.raises(na.NeuralAudioError, match="IR 5 is not loaded"):
        b.UnloadIR(5)
    with pytest.raises(na.NeuralAudioError, match="stream 2 is parked"):
        b.SetStreamIR(2, a, 0)
    with pytest.raises(na.NeuralAudioError, match="stream 12 is not a live stream"):
        b.SetStreamIR(12, a, 0)
    for fade in (-1, (1 << 20) + 1):
        with pytest.raises(na.NeuralAudioError, match=r"fadeSamples must lie in \[0, 1 << 20\]"):
            b.SetStreamIR(0, a, fade)
    b.SetStreamIR(0, a, 1 << 20)
    with pytest.raises(na.NeuralAudioError, match="an IR fade of stream 0 is running"):
        b.SetStreamIR(0, c, 0)
    with pytest.raises(na.NeuralAudioError, match="in use"):
        b.UnloadIR(a)
    with pytest.raises(na.NeuralAudioError, match="a larger maxTaps is refused while a stream has an IR"):
        b.EnableCabinetStage(512)
    assert b.GetStreamIR(0) == a and b.IRFadeRemaining(0) == 1 << 20 and b.GetStreamIR(1) == -1
    b.ParkStream(0)  # dry at once: the IR is free, the stage may grow
    b.UnloadIR(a)
    b.EnableCabinetStage(512)
    assert b.CabinetInfo()["maxTaps"] == 512
    # the stage grows with the batch, and a snapshot leaves the assignment alone
    b.SetStreamIR(4, c, 0)
    first = b.ReserveStreams(models[H.LSTM], 30)
    b.ActivateStream(first + 29, 1.0)
    b.SetStreamIR(first + 29, c, 0)
    blob = b.SaveStreams([5])
    b.LoadStreams([4], blob)
    assert b.GetStreamIR(4) == c and b.GetStreamIR(first + 29) == c
    y = b.Process(H.signal(64, 26)[np.arange(b.NumStreams()) % H.ROWS])
    assert np.any(y[first + 29]) and np.all(np.isfinite(y))
    # a broken batch refuses everything
    b.SetWaitLimitMs(20.0)
    b.DebugStallDevice(80.0)
    with pytest.raises(na.NeuralAudioError, match="did not answer within"):
        b.Synchronize()
    assert b.IsBroken()
    for call in (lambda: b.SetStreamIR(4, -1, 0), lambda: b.LoadIR(np.ones(4, np.float32)), lambda: b.UnloadIR(c), lambda: b.EnableCabinetStage(512)):
        with pytest.raises(na.NeuralAudioError, match="broken"):
            call()
    b.close()


def test_set_calls_and_processing_with_fades_are_real_time_safe(na, models):
    """NA_DebugDeviceResourceCalls stays where it is across set calls and 20 processing calls with fades running, over the blocking
    and the pipelined host path and device pointers (after three warm calls of each, which size the staging block and the three
    pipeline slots)."""
    import torch
    from neuralaudio_amd import capi
    lib = capi.load_library()
    dev = torch.device("cuda", 0)
    b, ids = K.make_batch(na, models, _irs(), 256)
    n = 128
    x = H.signal(n, 27)
    dx, dy = torch.from_numpy(x).to(dev), torch.zeros(H.ROWS, n, device=dev)
    torch.cuda.synchronize(dev)

    def three():
        b.Process(x)
        b.Collect(b.Submit(x))
        b.ProcessDevice(dx.data_ptr(), dy.data_ptr(), n, n, n)
        b.Synchronize()

    b.SetStreamIR(0, ids["short"], 0)
    for _ in range(3):  # (warm: the staging block and every pipeline slot's blocks of this buffer size)
        three()
    before = lib.NA_DebugDeviceResourceCalls()
    b.SetStreamIR(0, ids["cabA"], 5000)
    b.SetStreamIR(4, ids["cabB"], 4000)
    b.SetStreamIR(8, ids["cabA"], 100)
    for i in range(7):
        three()
        if i == 3:
            b.SetStreamIR(8, -1, 2000)
            b.SetStreamIR(9, ids["short"], 0)
    assert b.IRFadeRemaining(0) == 5000 - 21 * n and b.IRFadeRemaining(8) == 2000 - 9 * n
    assert lib.NA_DebugDeviceResourceCalls() == before
    b.close()
