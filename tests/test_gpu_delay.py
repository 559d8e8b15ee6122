"""GPU tests of the delay stage (NA_BatchEnableDelayStage / SetStreamDelay, csrc/delay_stage.h): a per-stream feedback
delay line behind the cabinet stage and in front of the reverb stage.

The contract states every f32 operation and its order, so the expected value is the numpy float32 restatement of tests/delay_cases.py
and every comparison is on the bits.  Part 1 drives the stage through its hook (NA_DebugRunDelayStage) on rows that stand in for model
outputs; part 2 runs the twelve-row batch of tests/handover_cases.py beside its twin without the stage."""
import os

import numpy as np
import pytest

import cabinet_cases as K
import delay_cases as D
import handover_cases as H
import reverb_cases as R

FORCED = bool(os.environ.get("NA_WN_KERNEL") or os.environ.get("NA_WN_PACK") or os.environ.get("NA_WN_SPEC") or os.environ.get("NA_SP_T")
              or os.environ.get("NA_SP_GEN") or os.environ.get("NA_WN_PAD"))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(FORCED, reason="forced kernel family")]

F = np.float32
CAB = np.array([0.0, 0.0, 0.5], F)  # the cabinet IR of the order tests


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
    return capi.load_library().NA_DebugDelayLaunches


def odd(n):
    return n + 3


def pieces(calls):
    """launches of calls with an entry: one per piece of 2048 samples"""
    return sum((n + 2047) // 2048 for n in calls)


def expect_rows(refs, x, calls):
    """the restatements of `refs` {row: DelayRef} over x cut into `calls`; the other rows keep their bits"""
    e, pos = x.copy(), 0
    for n in calls:
        for row, ref in refs.items():
            e[row, pos:pos + n] = ref.process(x[row, pos:pos + n])
        pos += n
    return e


def assert_same(y, e, what=()):
    for row in range(y.shape[0]):
        assert D.same_bits(y[row], e[row]), what + ("row", row, D.first_difference(y[row], e[row]))


# ================================================================================================ 1: through the hook

def test_known_answer_and_subnormals(na, models, launches):
    """aL = 1, aH = 0, fb = 0.5, wet = dry = 1.  D = 3 on a unit impulse: the impulse, then echoes of exactly 1, 0.5, 0.25, ... at 3, 6,
    9, ...  D = 4 on an impulse of 2^-120 over 256 samples: the echoes walk through the subnormals to zero, exactly -- a build that
    flushes to zero ends at 2^-126.  wet = 0, dry = 1: the row is x' bit for bit."""
    n = 256
    hb = D.HookBatch(na, models[H.NANO], 4, 300)
    x = np.zeros((4, n), F)
    x[0, 0], x[1, 0] = 1.0, F(2.0 ** -120)
    x[2] = D.noise(n, 1)
    x[2, 3], x[2, 4], x[2, 5], x[2, 6] = F("nan"), F("inf"), F(-1e30), F(-0.0)
    x[3] = D.noise(n, 2)
    hb.b.SetStreamDelay(0, D.params(3, 0.5))
    hb.b.SetStreamDelay(1, D.params(4, 0.5))
    hb.b.SetStreamDelay(2, D.params(5, 0.9, 0.5, 0.1, 0.0, 1.0))
    before = launches()
    y = hb.run(x, [100, 156], stride=odd)
    assert launches() - before == 2
    e0 = np.zeros(n, F)
    e0[0] = 1.0
    e0[3::3] = [F(2.0 ** -m) for m in range(len(e0[3::3]))]
    e1 = np.zeros(n, F)
    e1[0] = F(2.0 ** -120)
    e1[4::4] = [F(2.0 ** -(120 + m)) for m in range(len(e1[4::4]))]
    assert 0 < e1[4 * 8] < np.finfo(F).tiny and e1[4 * 30] == F(2.0 ** -149) and not np.any(e1[4 * 31:])
    assert_same(y, np.stack([e0, e1, D.sanitise(x[2]), x[3]]))
    hb.close()


def test_delays_around_every_boundary(na, models, launches):
    """maxDelaySamples = 300: a ring of 4096.  D = 1, 2, 3, 63, 64, 65, 127, 128, 129, 299, 300 on eleven rows of one launch, both
    filters in the loop, 10000 samples in calls of 1, 7, 64, 128, 129, 2048, 2049 and 3000 with an odd stride: D below, at and above the
    tile and the piece, the ring wraps more than twice, and the twelfth row keeps its bits."""
    rows, total = 12, 10000
    hb = D.HookBatch(na, models[H.NANO], rows, 300)
    info = hb.b.GetDelayInfo()
    assert (info["maxDelaySamples"], info["ringSamples"], info["pieceSamples"], info["numDelays"]) == (300, 4096, 2048, 0)
    assert info["deviceBytes"] >= 16 * (4096 * 4 + 8)
    x = np.stack([D.noise(total, 10 + r) for r in range(rows)])
    refs = {}
    for r, d in enumerate(D.BOUNDARY_DELAYS):
        p = D.filtered(d, feedback=(-0.85 if r % 2 else 0.85))
        hb.b.SetStreamDelay(r, p)
        assert hb.b.GetStreamDelay(r) == p
        refs[r] = D.DelayRef()
        refs[r].set(p)
    assert hb.b.GetDelayInfo()["numDelays"] == 11 and hb.b.GetStreamDelay(11) is None
    calls = D.cuts(total, D.BOUNDARY_CALLS)
    assert set(D.BOUNDARY_CALLS) <= set(calls)
    before = launches()
    y = hb.run(x, calls, stride=odd)
    assert launches() - before == pieces(calls), "one launch per piece"
    assert_same(y, expect_rows(refs, x, calls))
    hb.close()


def test_long_delays(na, models):
    """maxDelaySamples = 1 << 18: a ring of 1 << 19.  First D = 2047, 2048, 2049 -- around the piece -- with both filters in the loop,
    7000 samples.  Then the longest line there is, D = 262144, with D = 2048 beside it (no filters: the restatement runs as arrays),
    over 2 * 262144 + 5000 samples in calls of 4096 and one of 2049: the longest line repeats once and the ring wraps."""
    hb = D.HookBatch(na, models[H.NANO], 4, 1 << 18)
    info = hb.b.GetDelayInfo()
    assert info["ringSamples"] == 1 << 19 and info["deviceBytes"] >= 16 * (1 << 19) * 4
    total = 7000
    x = np.stack([D.noise(total, 30 + r) for r in range(4)])
    refs = {}
    for r, d in enumerate(D.LONG_DELAYS[:3]):
        refs[r] = D.DelayRef()
        refs[r].set(D.filtered(d))
        hb.b.SetStreamDelay(r, D.filtered(d))
    calls = D.cuts(total, [2048, 1, 2049, 500])
    assert_same(hb.run(x, calls), expect_rows(refs, x, calls), ("filters",))
    for r in range(3):
        hb.b.SetStreamDelay(r, None)
    assert hb.b.GetDelayInfo()["numDelays"] == 0
    total = 2 * D.LONG_DELAYS[3] + 5000
    x = np.stack([D.noise(total, 40 + r) for r in range(4)])
    refs = {}
    for r, d in ((0, 2048), (3, D.LONG_DELAYS[3])):
        refs[r] = D.DelayRef()
        refs[r].set(D.params(d, -0.9, wet=0.5))
        hb.b.SetStreamDelay(r, D.params(d, -0.9, wet=0.5))
    calls = [2049] + D.cuts(total - 2049, [4096])
    y = hb.run(x, calls)
    assert_same(y, expect_rows(refs, x, calls), ("long",))
    assert np.any(y[3, 2 * D.LONG_DELAYS[3]:] != x[3, 2 * D.LONG_DELAYS[3]:]) and np.any(y[0] != x[0])
    hb.close()


def test_the_cut_into_calls_never_shows(na, models):
    """One signal, three different cuts, the same bits -- and the restatement's."""
    total = 5000
    x = np.stack([D.noise(total, 50 + r) for r in range(4)])
    delays = (1, 64, 100, 300)
    outs = []
    for calls, stride in (([total], odd), (D.cuts(total, H.RAGGED), lambda n: n), (D.cuts(total, [63, 2049, 65, 1]), lambda n: (n + 3) // 4 * 4)):
        hb = D.HookBatch(na, models[H.NANO], 4, 300 if len(calls) > 1 else 4000)
        for r, d in enumerate(delays):
            hb.b.SetStreamDelay(r, D.filtered(d))
        outs.append(hb.run(x, calls, stride=stride))
        hb.close()
    refs = {r: D.DelayRef() for r in range(4)}
    for r, d in enumerate(delays):
        refs[r].set(D.filtered(d))
    e = expect_rows(refs, x, [total])
    for y in outs:
        assert_same(y, e)


def test_more_entries_than_one_wave(na, models, launches):
    """130 streams, delays on 67 of them with distinct D: two workgroups, the second with three entries.  The 63 rows without an entry
    are untouched bit for bit."""
    rows, total = 130, 700
    hb = D.HookBatch(na, models[H.NANO], rows, 300)
    x = np.stack([D.noise(total, 100 + r) for r in range(rows)])
    refs = {}
    for i, r in enumerate([r for r in range(rows) if r % 2 == 0] + [1, 129]):
        p = D.filtered(1 + 4 * i, feedback=0.5 + 0.005 * i)
        hb.b.SetStreamDelay(r, p)
        refs[r] = D.DelayRef()
        refs[r].set(p)
    assert len(refs) == 67 and hb.b.GetDelayInfo()["numDelays"] == 67
    calls = [129, 1, 570]
    before = launches()
    y = hb.run(x, calls, stride=odd)
    assert launches() - before == 3
    assert_same(y, expect_rows(refs, x, calls))
    hb.close()


def test_fades(na, models, launches):
    """none -> A (the echo fades in on an empty line), A -> B with another D (the read head cross-fades), B -> C on the same D (the
    gains ramp), C -> none (the echo fades out), each with cuts inside the fade: FadeRemaining counts down, a set call during a fade is
    refused, the entry retires with the sample at which the fade ends -- the rest of that call keeps the input's bits, a NaN included
    -- and the launch counter stops."""
    hb = D.HookBatch(na, models[H.NANO], 4, 300)
    total = 4000
    x = np.stack([D.noise(total, 60 + r) for r in range(4)])
    x[1, 3150] = F("nan")
    a, b, c = D.filtered(300), D.params(77, -0.6, 0.5, 0.0, 0.8, 1.0), D.params(77, 0.9, 0.25, 0.1, 0.3, 0.6)
    ref = D.DelayRef()
    script = [(a, 500, [100, 399, 1, 200]), (b, 700, [64, 65, 570, 1, 300]), (c, 129, [128, 1, 171]), (None, 150, [100, 49, 151, 1700])]
    out, e, pos = [], x.copy(), 0
    for p, N, calls in script:
        hb.b.SetStreamDelay(1, p, N)
        ref.set(p, N)
        assert hb.b.GetStreamDelay(1) == p
        left = N
        for i, n in enumerate(calls):
            before = launches()
            out.append(hb.run(x[:, pos:pos + n], [n], stride=odd))
            e[1, pos:pos + n] = ref.process(x[1, pos:pos + n])
            pos += n
            left = max(left - n, 0)
            assert hb.b.StreamDelayFadeRemaining(1) == left == ref.remaining()
            if left > 0:
                with pytest.raises(na.NeuralAudioError, match="SetStreamDelay: a delay fade of stream 1 is running"):
                    hb.b.SetStreamDelay(1, a, 0)
            retired = p is None and left == 0
            assert hb.b.GetDelayInfo()["numDelays"] == (0 if retired else 1)
            assert launches() - before == (0 if p is None and i == 3 else 1)
    assert pos == total
    y = np.concatenate(out, axis=1)
    assert_same(y, e)
    assert np.isnan(y[1, 3150]) and not ref.on, "behind the retirement the row is not touched"
    hb.close()


def test_a_stale_ring_does_not_leak(na, models):
    """A delay, a loud signal, a fade to none -- and a delay again: the ring still holds the loud line, the output equals a fresh
    restatement that starts from an empty line.  The same behind a retirement at once (N = 0) and behind a larger maxDelaySamples."""
    hb = D.HookBatch(na, models[H.NANO], 4, 300)
    loud = np.stack([D.noise(3000, 70 + r, gain=1000.0) for r in range(4)])
    quiet = np.stack([D.noise(900, 80 + r, gain=0.01) for r in range(4)])
    p = D.filtered(250, 0.95)
    for s in (0, 2):
        hb.b.SetStreamDelay(s, p)
    hb.run(loud, [3000])
    hb.b.SetStreamDelay(0, None, 64)
    hb.b.SetStreamDelay(2, None, 0)
    hb.run(loud[:, :64], [64])
    assert hb.b.GetDelayInfo()["numDelays"] == 0
    refs = {}
    for s in (0, 2):
        hb.b.SetStreamDelay(s, p)
        refs[s] = D.DelayRef()
        refs[s].set(p)
    calls = [100, 149, 2, 649]
    assert_same(hb.run(quiet, calls), expect_rows(refs, quiet, calls))
    hb.close()


def test_nan_inf_and_huge_inputs(na, models):
    """NaN, +-inf and +-1e30 all over the rows, feedback at its limit: every output is finite and equals the restatement."""
    hb = D.HookBatch(na, models[H.NANO], 4, 300)
    total = 3000
    rng = np.random.default_rng(90)
    x = np.stack([D.noise(total, 91 + r) for r in range(4)])
    bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3e38, -0.0, 1e-45], F)
    where = rng.random(x.shape) < 0.2
    x[where] = rng.choice(bad, int(where.sum()))
    refs = {}
    for r, p in enumerate((D.params(1, 0.99, wet=1e6, dry=1e6), D.params(2, -0.99, 1.0, 0.0, -1e6, 1.0), D.filtered(64, 0.99), D.params(300, 0.99, 0.999, 0.999, 1.0, 0.0))):
        hb.b.SetStreamDelay(r, p)
        refs[r] = D.DelayRef()
        refs[r].set(p)
    calls = [1000, 1, 1999]
    y = hb.run(x, calls)
    assert np.all(np.isfinite(y)) and np.max(np.abs(y)) > 1e20
    assert_same(y, expect_rows(refs, x, calls))
    hb.close()


# ================================================================================================ 2: the twelve-row batch

def run_batch(na, models, x, calls, ops, path="process", resample=None, prepare=None):
    """The batch under test through `path`, call by call; ops: {call index: [(stream, params or None, N)]}.  Returns its rows."""
    b = H.make_batch(na, models, stage=True, resample=resample)
    b.EnableDelayStage(4800)
    if prepare:
        prepare(b)
    runner, out, pos = H.Runner(na, b, path), [], 0
    try:
        for i, n in enumerate(calls):
            for s, p, N in ops.get(i, ()):
                b.SetStreamDelay(s, p, N)
            out.append(runner.call(x[:, pos:pos + n]))
            pos += n
    finally:
        runner.close()
        b.close()
    return np.concatenate(out, axis=1)


def twin_rows(na, models, x, calls, resample=None):
    return np.concatenate(H.run_twin(na, models, x, calls, {}, resample), axis=1)


def test_off_is_off(na, models, launches):
    """The stage is enabled and no stream has a delay: every path gives the twin's bits and launches none of the stage's kernels."""
    calls = [128, 17, 300, 128]
    x = H.signal(sum(calls), 21)
    yt = twin_rows(na, models, x, calls)
    before = launches()
    for path in ("process", "registered", "submit", "device", "device-odd"):
        y = run_batch(na, models, x, calls, {}, path)
        assert np.array_equal(y, yt), path
    assert launches() == before and np.any(yt[0]) and np.any(yt[4]) and np.any(yt[8]) and not np.any(yt[2])


def test_off_is_off_for_the_half_batch_launches(na, models, launches):
    """512 A1 Standard streams on the batch's own stream, device pointers: with the stage enabled and no delay the free-running mode
    engages as in the twin and the bits are the twin's; a delay on one stream orders the launches; taken away (N = 0: it retires at
    the set call), the mode comes back."""
    import torch
    dev = torch.device("cuda", 0)
    S, n, calls = 512, 128, 5
    x = np.stack([D.noise(calls * n, 200 + r) for r in range(5)])[np.arange(S) % 5]
    dx = torch.from_numpy(x).to(dev)
    torch.cuda.synchronize(dev)
    halves, outs = {}, {}
    p = D.filtered(100)
    for stage in (True, False):
        b = na.Batch(0)
        assert b.ReserveStreams(models[H.STD], S) == 0
        for s in range(S):
            b.ActivateStream(s, 1.0)
        if stage:
            b.EnableDelayStage(300)
        dy = torch.zeros(S, calls * n, device=dev)
        before = launches()
        for k in range(calls):
            if stage and k == 2:
                b.SetStreamDelay(7, p)
            if stage and k == 3:
                b.SetStreamDelay(7, None)
            b.ProcessDevice(dx.data_ptr() + 4 * k * n, dy.data_ptr() + 4 * k * n, n, calls * n, calls * n)
            b.Synchronize()
            halves[(stage, k)] = b.UsesHalfLaunches()
        assert launches() - before == (1 if stage else 0), "one launch per piece of a call with an entry"
        outs[stage] = dy.cpu().numpy()
        b.close()
    for k in (0, 1, 3, 4):
        assert halves[(True, k)] == halves[(False, k)], k
    print("half-batch launches: twin %s, with a delay %s, behind it %s" % (halves[(False, 1)], halves[(True, 2)], halves[(True, 3)]))
    assert not halves[(True, 2)]
    ref = D.DelayRef()
    ref.set(p)
    expect = outs[False].copy()
    expect[7, 2 * n:3 * n] = ref.process(outs[False][7, 2 * n:3 * n])
    assert np.array_equal(outs[True], expect)


DELAYED = {0: D.filtered(63), 4: D.filtered(1000, -0.7), 8: D.params(1, 0.9, 0.5, 0.0, 0.5, 1.0), 9: D.params(129, 0.5)}


@pytest.mark.parametrize("path", ["process", "device", "device-odd"])
def test_delays_on_one_stream_of_each_family(na, models, launches, path):
    """Delays on rows 0 (packed nano), 4 (Standard), 8 and 9 (LSTM) from the second call on, through the blocking host path and device
    pointers with aligned and odd row strides; calls around the tile and one longer than a piece.  Every row of every call: the
    restatement on the twin's row, or the twin's bits."""
    calls = list(H.RAGGED) + [127, 128, 129, 2049, 700]
    total = sum(calls)
    x = H.signal(total, 22)
    yt = twin_rows(na, models, x, calls)
    before = launches()
    y = run_batch(na, models, x, calls, {1: [(s, p, 0) for s, p in DELAYED.items()]}, path)
    assert launches() - before == pieces(calls[1:])
    refs = {s: D.DelayRef() for s in DELAYED}
    for s, p in DELAYED.items():
        refs[s].set(p)
    e = yt.copy()
    e[:, calls[0]:] = expect_rows(refs, yt[:, calls[0]:], calls[1:])
    assert_same(y, e, (path,))
    assert any(not np.array_equal(y[s], yt[s]) for s in DELAYED)


def test_the_order_is_cabinet_delay_reverb_gain(na, models):
    """Row 4 gets a cabinet IR in front of call 1, a delay in front of call 2, a reverb in front of call 3 and an output gain of 0.5 in
    front of call 4.  The IR is 0.5 e_2, exact in any order of summation, so the delay's input is known bit for bit, samples from
    before its T0 included; the row equals the composition of the four restatements, and differs from the one with delay and reverb
    swapped."""
    calls = [128, 100, 300, 128, 17, 300]
    x = H.signal(sum(calls), 23)
    yts = H.run_twin(na, models, x, calls, {})
    tw = R.library_twiddles()
    room = (np.random.default_rng(7).standard_normal(700) * np.exp(-np.arange(700) / 150.0) * 0.1).astype(F)
    p = D.filtered(90, 0.7)
    b = H.make_batch(na, models, stage=True)
    b.EnableCabinetStage(256)
    b.EnableDelayStage(300)
    b.EnableReverbStage(2048)
    cab, rev = b.LoadIR(CAB), b.LoadReverbIR(room)
    ref, cab_in, rev_in, swapped_in, pos = D.DelayRef(), [], [], [], 0
    for i, n in enumerate(calls):
        if i == 1:
            b.SetStreamIR(4, cab, 0)
        if i == 2:
            b.SetStreamDelay(4, p, 0)
            ref.set(p)
        if i == 3:
            b.SetStreamReverb(4, rev, 0.6, 1.0, 0)
        if i == 4:
            b.SetStreamGain(4, 0.5, 0)
        y = b.Process(np.ascontiguousarray(x[:, pos:pos + n]))
        z = yts[i][4]
        if i >= 1:
            cab_in.append(yts[i][4])
            hist = np.concatenate(cab_in)
            z = K.conv64(CAB, hist).astype(F)[len(hist) - n:]  # (0.5 e_2: exact in any order of summation)
        if i >= 2:
            z = ref.process(z)
        if i >= 3:
            rev_in.append(z)
            z = R.reverb_f32(room, np.concatenate(rev_in), tw, 0.6, 1.0, start=sum(len(r) for r in rev_in) - n)
        if i >= 4:
            z = (z * F(0.5)).astype(F)
        assert D.same_bits(y[4], z), (i, D.first_difference(y[4], z))
        for s in (0, 1, 5, 8, 9):
            assert np.array_equal(y[s], yts[i][s]), (i, s)
        pos += n
    b.close()
    # the other order on the last calls' input: reverb first, then the delay -- not what the batch gave
    other = D.DelayRef()
    other.set(p)
    hist = np.concatenate(cab_in)
    c = K.conv64(CAB, hist).astype(F)
    t_delay, t_rev = calls[1], calls[1] + calls[2]
    wrong = c.copy()
    wrong[t_rev:] = R.reverb_f32(room, c[t_rev:], tw, 0.6, 1.0)
    wrong[t_delay:] = other.process(wrong[t_delay:])
    assert not D.same_bits((wrong[-calls[5]:] * F(0.5)).astype(F), z), "the test can tell the two orders apart"


def test_the_same_composition_on_a_resampling_batch(na, models):
    """A 44.1 kHz resampling batch: the stage acts on the external-rate rows behind the down kernel.  Cabinet (0.5 e_2), delay and
    reverb on row 8, a delay alone on row 0: the composition of the restatements on the twin's rows, in two different cuts."""
    segments = [128, 441, 100, 300, 500]
    total = sum(segments)
    x = H.signal(total, 24)
    tw = R.library_twiddles()
    room = (np.random.default_rng(8).standard_normal(300) * np.exp(-np.arange(300) / 60.0) * 0.1).astype(F)
    p = D.filtered(441, 0.6)
    outs = []
    for cut in (lambda n: [n], H.ragged):
        calls = [n for seg in segments for n in cut(seg)]
        b = H.make_batch(na, models, stage=True, resample=44100)
        b.EnableCabinetStage(64)
        b.EnableDelayStage(4410)
        b.EnableReverbStage(1024)
        ir, rev = b.LoadIR(CAB), b.LoadReverbIR(room)
        y, pos = [], 0
        for n in calls:
            if pos == segments[0]:
                b.SetStreamIR(8, ir, 0)
                b.SetStreamDelay(8, p, 0)
                b.SetStreamDelay(0, p, 200)
                b.SetStreamReverb(8, rev, 0.5, 1.0, 0)
            y.append(b.Process(np.ascontiguousarray(x[:, pos:pos + n])))
            pos += n
        outs.append(np.concatenate(y, axis=1))
        b.close()
    assert np.array_equal(outs[0], outs[1]), np.flatnonzero(np.any(outs[0] != outs[1], axis=1))
    yt = twin_rows(na, models, x, segments, resample=44100)
    t0 = segments[0]
    r0, r8 = D.DelayRef(), D.DelayRef()
    r0.set(p, 200)
    r8.set(p)
    e0 = yt[0].copy()
    e0[t0:] = r0.process(yt[0, t0:])
    c = K.conv64(CAB, yt[8, t0:]).astype(F)
    e8 = yt[8].copy()
    e8[t0:] = R.reverb_f32(room, r8.process(c), tw, 0.5, 1.0)
    assert D.same_bits(outs[0][0], e0), D.first_difference(outs[0][0], e0)
    assert D.same_bits(outs[0][8], e8), D.first_difference(outs[0][8], e8)
    assert np.array_equal(outs[0][4], yt[4])


def test_in_place(na, models):
    """NA_BatchProcessDevice with dIn == dOut on streams with a delay: the bits are those of separate buffers."""
    import torch
    dev = torch.device("cuda", 0)
    calls = [128, 300, 129, 700]
    x = H.signal(sum(calls), 25)
    outs = {}
    for in_place in (False, True):
        b = H.make_batch(na, models, stage=False)
        b.EnableDelayStage(4800)
        for s, p in DELAYED.items():
            b.SetStreamDelay(s, p, 100)
        y, pos = [], 0
        for n in calls:
            xs = np.ascontiguousarray(x[:, pos:pos + n])
            buf = torch.from_numpy(xs).to(dev)
            out = buf if in_place else torch.zeros(H.ROWS, n, device=dev)
            torch.cuda.synchronize(dev)
            b.ProcessDevice(buf.data_ptr(), out.data_ptr(), n, n, n)
            b.Synchronize()
            rows = out.cpu().numpy()
            if in_place:
                rows[list(set(range(H.ROWS)) - set(H.LIVE))] = 0.0  # (device rows of parked streams are left alone: here, the input)
            y.append(rows)
            pos += n
        outs[in_place] = np.concatenate(y, axis=1)
        b.close()
    assert np.array_equal(outs[True], outs[False]) and np.any(outs[True][4])


def test_rules(na, models):
    """Each refusal carries its text; park, remove and the park that ends a hand-over drop the delay; an activated stream has none; a
    larger maximum is refused while a stream has a delay; a broken batch refuses everything."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    b = H.make_batch(na, models, stage=True)  # (with the output stage, for the hand-over)
    p = D.filtered(100)
    for call in (lambda: b.SetStreamDelay(0, p), lambda: b.SetStreamDelay(0, None), lambda: b.GetStreamDelay(0), lambda: b.StreamDelayFadeRemaining(0),
                 lambda: b.GetDelayInfo(), lambda: b.DebugRunDelayStage(np.zeros((H.ROWS, 8), F))):
        with pytest.raises(na.NeuralAudioError, match=D.NOT_ENABLED):
            call()
    assert lib.NA_BatchGetStreamDelay(b._h, 0, None) < 0 and lib.NA_BatchStreamDelayFadeRemaining(b._h, 0) < 0
    for bad in (0, (1 << 18) + 1, -5):
        with pytest.raises(na.NeuralAudioError, match=r"EnableDelayStage: maxDelaySamples must lie in \[1, 1 << 18\]"):
            b.EnableDelayStage(bad)
    b.EnableDelayStage(1000)
    b.EnableDelayStage(1000)
    b.EnableDelayStage(10)  # idempotent for an equal or smaller maximum
    info = b.GetDelayInfo()
    assert (info["maxDelaySamples"], info["ringSamples"], info["pieceSamples"], info["numDelays"]) == (1000, 4096, 2048, 0)
    with pytest.raises(na.NeuralAudioError, match="SetStreamDelay: stream 2 is parked"):
        b.SetStreamDelay(2, p)
    with pytest.raises(na.NeuralAudioError, match="SetStreamDelay: stream 12 is not a live stream of the batch"):
        b.SetStreamDelay(12, p)
    with pytest.raises(na.NeuralAudioError, match="GetStreamDelay: stream 12 is not a stream of the batch"):
        b.GetStreamDelay(12)
    with pytest.raises(na.NeuralAudioError, match="StreamDelayFadeRemaining: stream -1 is not a stream of the batch"):
        b.StreamDelayFadeRemaining(-1)
    nan, inf = float("nan"), float("inf")
    for change, text in ((dict(delaySamples=0), r"delaySamples must lie in \[1, maxDelaySamples\] \(maxDelaySamples = 1000\)"),
                         (dict(delaySamples=1001), r"delaySamples must lie in \[1, maxDelaySamples\] \(maxDelaySamples = 1000\)"),
                         (dict(feedback=0.995), r"feedback must lie in \[-0.99, 0.99\]"), (dict(feedback=-1.0), r"feedback must lie in \[-0.99, 0.99\]"),
                         (dict(feedback=nan), r"feedback must lie in \[-0.99, 0.99\]"), (dict(lowpassCoeff=0.0), r"lowpassCoeff must lie in \(0, 1\]"),
                         (dict(lowpassCoeff=1.5), r"lowpassCoeff must lie in \(0, 1\]"), (dict(lowpassCoeff=nan), r"lowpassCoeff must lie in \(0, 1\]"),
                         (dict(highpassCoeff=1.0), r"highpassCoeff must lie in \[0, 1\)"), (dict(highpassCoeff=-0.1), r"highpassCoeff must lie in \[0, 1\)"),
                         (dict(highpassCoeff=nan), r"highpassCoeff must lie in \[0, 1\)"), (dict(wet=inf), "wet must be finite and at most 1e6 in magnitude"),
                         (dict(wet=-2e6), "wet must be finite and at most 1e6 in magnitude"), (dict(dry=nan), "dry must be finite and at most 1e6 in magnitude"),
                         (dict(dry=1.5e6), "dry must be finite and at most 1e6 in magnitude")):
        with pytest.raises(na.NeuralAudioError, match="SetStreamDelay: " + text):
            b.SetStreamDelay(0, dict(p, **change))
    for fade in (-1, (1 << 20) + 1):
        with pytest.raises(na.NeuralAudioError, match=r"SetStreamDelay: fadeSamples must lie in \[0, 1 << 20\]"):
            b.SetStreamDelay(0, p, fade)
    assert b.GetDelayInfo()["numDelays"] == 0 and b.GetStreamDelay(0) is None
    b.SetStreamDelay(1, None)  # (no delay: nothing to take away)
    b.SetStreamDelay(0, D.params(1000, -0.99, 1.0, 0.0, -1e6, 1e6), 1 << 20)
    with pytest.raises(na.NeuralAudioError, match="a delay fade of stream 0 is running"):
        b.SetStreamDelay(0, None, 0)
    with pytest.raises(na.NeuralAudioError, match="a larger maxDelaySamples is refused while a stream has a delay"):
        b.EnableDelayStage(2000)
    assert b.StreamDelayFadeRemaining(0) == 1 << 20 and b.GetStreamDelay(0)["delaySamples"] == 1000 and b.StreamDelayFadeRemaining(1) == 0
    # park, remove and the end of a hand-over drop the delay at once; an activated stream has none
    for s in (1, 4, 5, 8):
        b.SetStreamDelay(s, p, 0 if s != 5 else 300)
    assert b.GetDelayInfo()["numDelays"] == 5
    b.ParkStream(0)
    assert b.GetDelayInfo()["numDelays"] == 4 and b.GetStreamDelay(0) is None and b.StreamDelayFadeRemaining(0) == 0
    b.ActivateStream(0, 1.0)
    assert b.GetStreamDelay(0) is None
    blob = b.SaveStreams([5])
    b.LoadStreams([4], blob)
    assert b.GetStreamDelay(4) == p and b.StreamDelayFadeRemaining(4) == 0 and b.GetDelayInfo()["numDelays"] == 4, "delays are not part of a snapshot"
    b.Handover(4, 6, 1.0, 64)
    x = H.signal(64, 26)
    b.Process(x)
    assert b.GetStreamDelay(4) is not None and b.GetStreamDelay(6) is None
    b.Process(x)  # (parks row 4 in front of its launches)
    assert b.IsParked(4) and b.GetStreamDelay(4) is None and b.GetDelayInfo()["numDelays"] == 3
    # the stage grows with the batch, and with a larger maximum once no stream has a delay
    first = b.ReserveStreams(models[H.LSTM], 30)
    b.ActivateStream(first + 29, 1.0)
    b.SetStreamDelay(first + 29, D.params(3, 0.5))
    y = b.Process(H.signal(64, 27)[np.arange(b.NumStreams()) % H.ROWS])
    assert np.any(y[first + 29]) and np.all(np.isfinite(y)) and b.GetStreamDelay(1) is not None
    assert b.GetDelayInfo()["deviceBytes"] >= b.NumStreams() * 4096 * 4
    for s in (1, 5, 8, first + 29):
        b.ParkStream(s)
    b.EnableDelayStage(5000)
    assert b.GetDelayInfo()["ringSamples"] == 8192
    # a broken batch refuses everything
    b.SetWaitLimitMs(20.0)
    b.DebugStallDevice(80.0)
    with pytest.raises(na.NeuralAudioError, match="did not answer within"):
        b.Synchronize()
    assert b.IsBroken()
    for call in (lambda: b.SetStreamDelay(9, p), lambda: b.SetStreamDelay(9, None), lambda: b.EnableDelayStage(100)):
        with pytest.raises(na.NeuralAudioError, match="broken"):
            call()
    b.close()


def test_remove_streams_drops_the_delay(na, models):
    b = na.Batch(0)
    assert b.AddStreams(models[H.LSTM], 4) == 0
    b.EnableDelayStage(300)
    b.SetStreamDelay(1, D.filtered(10))
    b.SetStreamDelay(2, D.filtered(20), 500)
    b.RemoveStreams(1, 1)
    assert b.GetDelayInfo()["numDelays"] == 1
    assert b.AddStreams(models[H.LSTM], 1) == 1 and b.GetStreamDelay(1) is None and b.GetStreamDelay(2) is not None
    b.close()


def test_growth_keeps_the_lines(na, models):
    """Four Standard streams, a delay on row 1, two calls; sixteen more streams take the rows past the stage's first capacity of 16, so
    its rings move; two more calls.  Row 1 is the restatement on the whole history (row 0 runs the same input without a delay)."""
    n = 128
    x = np.stack([H.noise(4 * n, 3200 + r) for r in range(20)])
    x[1] = x[0]
    b = na.Batch(0)
    assert b.AddStreams(models[H.STD], 4) == 0
    b.EnableDelayStage(300)
    p = D.filtered(200, 0.8)
    b.SetStreamDelay(1, p)
    before = b.GetDelayInfo()["deviceBytes"]
    out = []
    for k in range(4):
        if k == 2:
            assert b.AddStreams(models[H.STD], 16) == 4
            assert b.GetDelayInfo()["deviceBytes"] > before
        out.append(b.Process(x[:b.NumStreams(), k * n:(k + 1) * n])[:4])
    y = np.concatenate(out, axis=1)
    ref = D.DelayRef()
    ref.set(p)
    e = ref.process(y[0])
    assert D.same_bits(y[1], e), D.first_difference(y[1], e)
    b.close()


def test_set_calls_and_processing_with_delays_are_real_time_safe(na, models):
    """NA_DebugDeviceResourceCalls stays where it is across set calls and 21 processing calls with entries and fades, over the blocking
    and the pipelined host path and device pointers (after three warm calls of each, which size the staging block and the pipeline
    slots)."""
    import torch
    from neuralaudio_amd import capi
    lib = capi.load_library()
    dev = torch.device("cuda", 0)
    b = H.make_batch(na, models, stage=False)
    b.EnableDelayStage(4800)
    n = 128
    x = H.signal(n, 28)
    dx, dy = torch.from_numpy(x).to(dev), torch.zeros(H.ROWS, n, device=dev)
    torch.cuda.synchronize(dev)

    def three():
        b.Process(x)
        b.Collect(b.Submit(x))
        b.ProcessDevice(dx.data_ptr(), dy.data_ptr(), n, n, n)
        b.Synchronize()

    b.SetStreamDelay(0, D.filtered(100))
    for _ in range(3):
        three()
    before = lib.NA_DebugDeviceResourceCalls()
    b.SetStreamDelay(0, D.filtered(4800), 5000)
    b.SetStreamDelay(4, D.filtered(333), 4000)
    b.SetStreamDelay(8, D.params(7, 0.5), 100)
    for i in range(7):
        three()
        if i == 3:
            b.SetStreamDelay(8, None, 2000)
            b.SetStreamDelay(9, D.params(64, 0.5), 0)
    assert b.StreamDelayFadeRemaining(0) == 5000 - 21 * n and b.StreamDelayFadeRemaining(8) == 2000 - 9 * n
    assert b.GetStreamDelay(8) is None and b.GetStreamDelay(9) is not None and b.GetDelayInfo()["numDelays"] == 4
    assert lib.NA_DebugDeviceResourceCalls() == before
    assert np.all(np.isfinite(dy.cpu().numpy()))
    b.close()
