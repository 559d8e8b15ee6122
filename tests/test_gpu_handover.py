"""GPU tests of the output stage (NA_BatchEnableOutputStage / SetStreamGain / Handover, csrc/output_stage.h): ramped
stream gains and the cross-fade that hands a session from a live stream to a parked, armed stream of another model.

Every case runs the batch of tests/handover_cases.py -- BossWN-nano (packed four to a virtual stream), BossWN-standard, BossLSTM-2x8 --
beside its TWIN: the same reserve / activate / park history, no output stage, both streams of a hand-over kept running.  The expected
row is the header's formula in float64 on the twin's rows, elementwise to |y - e| <= 1e-6 * (|g_from * y_from| + |g_to * y_to|) + 1e-9;
where the stage must do nothing the check is np.array_equal.  Every scenario checks EVERY row of the batch in every call, so "the
neighbours never notice" -- the three streams that share `to`'s packed virtual stream, the streams of `from`'s group -- is part of each."""
import os

import numpy as np
import pytest

import handover_cases as H

FORCED = bool(os.environ.get("NA_WN_KERNEL") or os.environ.get("NA_WN_PACK") or os.environ.get("NA_WN_SPEC") or os.environ.get("NA_SP_T")
              or os.environ.get("NA_SP_GEN") or os.environ.get("NA_WN_PAD"))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(FORCED, reason="forced kernel family")]

# (from, to): live row of one model, parked row of the other
PAIRS = {"nano-standard": (0, 6), "standard-lstm": (4, 10), "lstm-nano": (8, 2), "standard-standard": (4, 6)}


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


@pytest.fixture(scope="module")
def models(na):
    return H.load_models(na)


def _level_gain(na, models, f, t):
    """what a host applies to `to` so that the session keeps its level: the two captures' recommended output adjustments, as a gain"""
    db = models[H.model_of(t)].GetRecommendedOutputDBAdjustment() - models[H.model_of(f)].GetRecommendedOutputDBAdjustment()
    return na.db_to_gain(db)


# ---------------------------------------------------------------------------------------------------------------- 1

def test_off_is_off(na, models):
    """The stage is enabled and nothing is set: NA_BatchProcess, a registered block, Submit / Collect and NA_BatchProcessDevice on torch
    tensors (both strides) give the twin's bits, row for row."""
    calls = [128, 17, 300, 128]
    x = H.signal(sum(calls), 1)
    for path in ("process", "registered", "submit", "device", "device-odd"):
        y, yt, _ = H.run_scenario(na, models, x, calls, {}, path=path)
        assert np.array_equal(y, yt), path
        assert np.any(y[0]) and np.any(y[4]) and np.any(y[8]) and not np.any(y[2])


def test_off_is_off_for_the_half_batch_launches(na, models):
    """... and the free-running modes engage as in the twin: 512 A1 Standard streams on the batch's own stream, device pointers."""
    import torch
    dev = torch.device("cuda", 0)
    S, n = 512, 128
    x = np.stack([H.noise(2 * n, 40 + r) for r in range(5)])[np.arange(S) % 5]
    dx = torch.from_numpy(x).to(dev)
    torch.cuda.synchronize(dev)
    answers, outs = [], []
    for stage in (True, False):
        b = na.Batch(0)
        assert b.ReserveStreams(models[H.STD], S) == 0
        for s in range(S):
            b.ActivateStream(s, 1.0)
        if stage:
            b.EnableOutputStage()
        dy = torch.zeros(S, 2 * n, device=dev)
        for k in range(2):
            b.ProcessDevice(dx.data_ptr() + 4 * k * n, dy.data_ptr() + 4 * k * n, n, 2 * n, 2 * n)
        b.Synchronize()
        answers.append(b.UsesHalfLaunches())
        outs.append(dy.cpu().numpy())
        b.close()
    assert answers[0] == answers[1]
    assert np.array_equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------------------- 2

def test_gain(na, models):
    """A constant gain matches the formula, gain 0 gives exact zeros, and after a ramp back to 1 the rows are the twin's bits again (the
    entries have retired).  One stream of each family; the packed neighbour (row 1) and the others are checked by the scenario."""
    calls = [128, 100, 128, 17, 128, 300, 128, 128]
    x = H.signal(sum(calls), 2)
    ops = {1: [("gain", 0, 0.5, 0), ("gain", 4, 1.7, 0), ("gain", 8, 0.0, 0)],
           3: [("gain", 9, 0.25, 0)],
           4: [("gain", 0, 1.0, 64), ("gain", 4, 1.0, 200), ("gain", 8, 1.0, 1), ("gain", 9, 1.0, 0)]}
    seen = {}

    def hook(b, contract, i):
        seen[i] = [b.GetStreamGain(s) for s in (0, 4, 8, 9, 1)]

    y, yt, worst = H.run_scenario(na, models, x, calls, ops, hook=hook)
    print("gain: largest error %.3f of the limit" % worst)
    assert seen[0] == [1.0, 1.0, 1.0, 1.0, 1.0] and seen[1] == [0.5, np.float32(1.7), 0.0, 1.0, 1.0] and seen[3][3] == 0.25 and seen[4] == [1.0] * 5
    a, c = calls[0], sum(calls[:4])
    assert not np.any(y[8, a:c]) and np.any(yt[8, a:c]), "gain 0 is exact silence"
    tail = sum(calls[:6])  # every ramp is over by then
    assert np.array_equal(y[:, tail:], yt[:, tail:])


def test_set_gain_before_enable_fails(na, models):
    b = H.make_batch(na, models, stage=False)
    for call in (lambda: b.SetStreamGain(0, 0.5, 0), lambda: b.GetStreamGain(0), lambda: b.Handover(0, 6, 1.0, 64), lambda: b.HandoverRemaining(0)):
        with pytest.raises(na.NeuralAudioError, match="output stage not enabled"):
            call()
    from neuralaudio_amd import capi
    assert capi.load_library().NA_BatchHandoverRemaining(b._h, 0) < 0 and "output stage not enabled" in capi.last_error()
    b.EnableOutputStage()
    b.EnableOutputStage()  # idempotent
    b.SetStreamGain(0, 0.5, 0)
    assert b.GetStreamGain(0) == 0.5
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 3

@pytest.mark.parametrize("R", [1, 7, 128, 300])
def test_ramps(na, models, R):
    """A ramp of R samples down and one up again, across ragged calls, on one stream of each family."""
    calls = H.ragged(1400)
    x = H.signal(sum(calls), 3)
    ops = {1: [("gain", 0, 0.2, R), ("gain", 5, 2.0, R), ("gain", 8, 0.0, R)],
           7: [("gain", 0, 1.0, R), ("gain", 5, 0.5, R), ("gain", 8, 1.0, R)]}
    y, yt, worst = H.run_scenario(na, models, x, calls, ops)
    print("ramp R=%d: largest error %.3f of the limit" % (R, worst))
    assert worst > 0.0


def test_a_retarget_in_mid_ramp_continues_from_the_reached_value(na, models):
    """300-sample ramp 1 -> 0.2, re-targeted to 0.9 over 128 samples after 96 of them, then to 0.1 over 7 in mid-ramp again.  The row
    matches the contract, and the per-sample gain step implied by the output (a constant input through gain alone: row / twin row)
    never exceeds |g_b - g_a| / R of the ramp that is active."""
    calls = [128, 64, 32, 50, 17, 128, 128]
    x = H.signal(sum(calls), 4)
    ops = {1: [("gain", 4, 0.2, 300)], 3: [("gain", 4, 0.9, 128)], 4: [("gain", 4, 0.1, 7)]}
    y, yt, worst = H.run_scenario(na, models, x, calls, ops)
    print("re-target: largest error %.3f of the limit" % worst)
    # the gain the stage applied, where the twin's sample is large enough to divide by
    big = np.abs(yt[4]) > 1e-3
    g = np.where(big, y[4].astype(np.float64) / np.where(big, yt[4], 1.0), np.nan)
    # per sample: the largest step of the ramp that is active there, |g_b - g_a| / R with g_a the value reached at the set call
    c, allowed = H.Contract(), []
    for i, n in enumerate(calls):
        step = allowed[-1] if allowed else 0.0
        for op in ops.get(i, ()):
            g_a = c.reached(4)
            c.apply(op)
            step = abs(c.ramp[4]["b"] - g_a) / c.ramp[4]["R"]
        allowed += [step] * n
        c.step(np.zeros((H.ROWS, n), np.float32))
    d = np.abs(np.diff(g))  # d[j]: the step into sample j + 1 (nan where a neighbour was too small to divide by)
    ok = ~np.isnan(d)
    assert np.count_nonzero(ok) > 200
    # (g comes from a quotient of f32 samples >= 1e-3 that are each good to 1e-6 relative: a few 1e-6 absolute at gains <= 1)
    assert np.all(d[ok] <= np.asarray(allowed[1:])[ok] + 4e-6), (int(np.argmax(np.where(ok, d - np.asarray(allowed[1:]), -1))), float(np.nanmax(d)))
    assert np.nanmax(d) > 1e-3, "the ramps moved the gain at all"


# ---------------------------------------------------------------------------------------------------------------- 4

@pytest.mark.parametrize("with_gain", [False, True], ids=["plain", "levelled"])
@pytest.mark.parametrize("N", [0, 1, 64, 128, 129, 1000])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_handover(na, models, pair, N, with_gain):
    """One hand-over in front of call 1.  During the fade row `to` matches the formula; NA_BatchHandoverRemaining counts down; `from`
    reports parked after the call behind the one that held the fade's last sample, and NA_BatchFindParked finds it; after the fade, at
    gain 1, row `to` is the twin's bits.  `levelled`: `to` takes the gain that keeps the session's level (the two captures'
    GetRecommendedOutputDBAdjustment), and goes back to 1 at the end.  Activated again, `from` equals a freshly added stream."""
    f, t = PAIRS[pair]
    calls = H.ragged(N + 600)
    x = H.signal(sum(calls), 5, same=[(f, t)])
    g = _level_gain(na, models, f, t) if with_gain else 1.0
    ops = {1: [("handover", f, t, N)] + ([("gain", t, g, 0)] if with_gain else [])}
    last = len(calls) - 2
    if with_gain:
        ops[last] = [("gain", t, 1.0, 0)]
    starts = np.cumsum([0] + calls)
    state = {}

    def hook(b, contract, i):
        done = starts[i + 1] - starts[1]
        if i >= 1:
            assert b.HandoverRemaining(f) == b.HandoverRemaining(t) == max(N - done, 0), i
        ended = N == 0 or (i >= 2 and starts[i] - starts[1] >= N)  # the call in front of this one held the fade's last sample
        assert b.IsParked(f) == (i >= 1 and ended), (i, done)
        if b.IsParked(f) and "parked_at" not in state:
            state["parked_at"] = i
            assert b.FindParked(models[H.model_of(f)]) == f
        assert b.IsLive(t) == (i >= 1)

    y, yt, worst = H.run_scenario(na, models, x, calls, ops, hook=hook)
    print("%s N=%d gain %.4f: largest error %.3f of the limit; from parked after call %s" % (pair, N, g, worst, state.get("parked_at")))
    assert "parked_at" in state
    after = starts[state["parked_at"]] if not with_gain else starts[last]
    assert np.array_equal(y[t, after:], yt[t, after:]) and np.any(y[t, after:]), "after the fade, at gain 1, row `to` is the twin's"
    assert not np.any(y[f, starts[state["parked_at"]]:])


@pytest.mark.parametrize("pair", list(PAIRS))
def test_the_stream_that_was_handed_over_comes_back_as_a_fresh_one(na, models, pair):
    """... test_gpu_pool.py's rule: after the automatic park `from` is armed; activated again it computes what a stream freshly added
    with NA_BatchAddStreams computes, bit for bit."""
    f, t = PAIRS[pair]
    calls = [128, 128, 128, 128, 17, 300]
    x = H.signal(sum(calls), 6, same=[(f, t)])
    b = H.make_batch(na, models, stage=True)
    b.SetStreamGain(f, 0.5, 0)
    pos, out = 0, []
    for i, n in enumerate(calls):
        if i == 1:
            b.Handover(f, t, 1.0, 100)
        if i == 3:
            assert b.IsParked(f) and b.GetStreamGain(f) == 1.0
            b.ActivateStream(f, 1.0)
        out.append(b.Process(np.ascontiguousarray(x[:, pos:pos + n])))
        pos += n
    b.close()
    y = np.concatenate(out, axis=1)
    fresh = na.Batch(0)
    fresh.AddStreams(models[H.model_of(f)], 4 if H.model_of(f) == H.NANO else 1)
    start = sum(calls[:3])
    xf = np.zeros((fresh.NumStreams(), sum(calls) - start), np.float32)
    xf[0] = x[f, start:]
    want = fresh.Process(xf)[0]
    fresh.close()
    assert np.array_equal(y[f, start:], want), int(np.count_nonzero(y[f, start:] != want))


# ---------------------------------------------------------------------------------------------------------------- 5

@pytest.mark.parametrize("pair", ["lstm-nano", "standard-standard"])
def test_call_size_independence(na, models, pair):
    """The same hand-over (N = 300, ramping gains on both sides) through calls of 128 and through the ragged list: identical samples
    on rows `from` and `to`."""
    f, t = PAIRS[pair]
    lead, body = 128, 128 * 9
    x = H.signal(lead + body, 7, same=[(f, t)])
    ops = {0: [("gain", f, 0.8, 500)], 1: [("handover", f, t, 300), ("gain", t, 0.6, 200)]}
    ya, _, _ = H.run_scenario(na, models, x, [lead] + [128] * 9, ops)
    yb, _, _ = H.run_scenario(na, models, x, [lead] + H.ragged(body), ops)
    n = lead + 300  # (`from` is parked by the first call behind the fade's last sample: which one depends on the cut)
    assert np.array_equal(ya[f, :n], yb[f, :n])
    assert np.array_equal(ya[t], yb[t])
    assert np.any(ya[t, lead:])


# ---------------------------------------------------------------------------------------------------------------- 6

@pytest.mark.parametrize("path", ["process", "registered", "device", "device-odd"])
def test_every_path(na, models, path):
    """Two hand-overs and a ramp through host buffers, a registered block, and device pointers with an aligned stride (the vector path)
    and with outStride = n + 3 (the scalar path)."""
    calls = [128, 129, 17, 128, 300, 64, 128]
    x = H.signal(sum(calls), 8, same=[(4, 10), (8, 2)])
    ops = {1: [("handover", 4, 10, 200), ("gain", 10, 0.7, 0), ("gain", 0, 0.3, 150)], 2: [("handover", 8, 2, 129)], 5: [("gain", 0, 1.0, 64)]}
    _, _, worst = H.run_scenario(na, models, x, calls, ops, path=path)
    print("%s: largest error %.3f of the limit" % (path, worst))
    assert worst > 0.0


def test_a_fade_that_spans_three_submit_tickets(na, models):
    """Three tickets in flight, the hand-over in front of the first: positions advance at Submit, in submission order."""
    n, f, t, N = 128, 4, 10, 300
    calls = [n] * 6
    x = H.signal(sum(calls), 9, same=[(f, t)])
    ops = {1: [("handover", f, t, N), ("gain", f, 0.5, 100)]}
    yts = H.run_twin(na, models, x, calls, ops)
    b = H.make_batch(na, models, stage=True)
    blk = lambda k: np.ascontiguousarray(x[:, k * n:(k + 1) * n])
    ys = [b.Collect(b.Submit(blk(0)))]
    for op in ops[1]:
        H.drive(b, op, True)
    tickets = [b.Submit(blk(k)) for k in (1, 2, 3)]
    assert b.HandoverRemaining(t) == 0 and not b.IsParked(f), "the fade's last sample is in the third ticket"
    ys += [b.Collect(tk) for tk in tickets]
    tickets = [b.Submit(blk(k)) for k in (4, 5)]
    assert b.IsParked(f)
    ys += [b.Collect(tk) for tk in tickets]
    b.close()
    contract = H.Contract()
    worst = 0.0
    for k in range(6):
        for op in ops.get(k, ()):
            contract.apply(op)
        worst = max(worst, H.check_call(ys[k], yts[k], contract, ("ticket", k)))
    print("three tickets: largest error %.3f of the limit" % worst)


def test_entries_come_and_go_with_submit_tickets_in_flight(na, models):
    """A one-model batch without a pool (AddStreams), two or three tickets in flight throughout.  An entry that appears through
    SetStreamGain alone, and one that retires inside a Submit (a ramp back to 1), move the buffers between the batch stream and the
    slots' own streams while the buffer before is still running: consecutive buffers stay ordered -- every other row is the twin's
    bits throughout, row 1 follows the contract and is the twin's bits again once its entry has retired -- and from EnableOutputStage
    on no Submit creates a stream or an event (the slots' buffers exist after one round of the three slots)."""
    from collections import deque
    from neuralaudio_amd import capi
    lib = capi.load_library()
    S, n, K = 8, 128, 18
    x = np.stack([H.noise(n * K, 300 + r) for r in range(S)])
    blk = lambda k: np.ascontiguousarray(x[:, k * n:(k + 1) * n])
    ops = {3: [("gain", 1, 0.5, 0)], 5: [("gain", 1, 1.0, 100)],     # appears with 1, 2 in flight; retires inside Submit 5
           8: [("gain", 1, 0.3, 200)], 9: [("gain", 1, 1.0, 0)],      # one buffer on a slot's stream between two on the batch stream
           11: [("gain", 1, 0.0, 1)], 12: [("gain", 1, 1.0, 129)]}   # retires inside Submit 13
    twin = na.Batch(0)
    assert twin.AddStreams(models[H.STD], S) == 0
    yts = [twin.Process(blk(k)) for k in range(K)]
    twin.close()
    b = na.Batch(0)
    assert b.AddStreams(models[H.STD], S) == 0
    b.EnableOutputStage()
    flight, ys, calls = deque(), [], None
    for k in range(K):
        if len(flight) == 3:
            ys.append(b.Collect(flight.popleft()))
        if k == 3:
            calls = lib.NA_DebugDeviceResourceCalls()
        for op in ops.get(k, ()):
            H.drive(b, op, True)
        flight.append(b.Submit(blk(k)))
        assert len(flight) >= min(k + 1, 3)
    moved = lib.NA_DebugDeviceResourceCalls() - calls
    while flight:
        ys.append(b.Collect(flight.popleft()))
    b.close()
    print("resource calls across the switches: %d" % moved)
    assert moved == 0
    contract, worst = H.Contract(rows=S, live=range(S)), 0.0
    for k in range(K):
        for op in ops.get(k, ()):
            contract.apply(op)
        worst = max(worst, H.check_call(ys[k], yts[k], contract, ("ticket", k)))
    print("switches with tickets in flight: largest error %.3f of the limit" % worst)
    y, yt = np.concatenate(ys, axis=1), np.concatenate(yts, axis=1)
    assert worst > 0.0 and np.any(y[1] != yt[1])
    for a, e in ((0, 3), (6, 8), (9, 11), (14, K)):  # no entry in these buffers: the twin's bits, row 1 included
        assert np.array_equal(y[:, a * n:e * n], yt[:, a * n:e * n]), (a, e)


def test_a_stream_awaiting_its_park_hands_nothing_over(na, models):
    """Between the call that holds a fade's last sample and the next one, `from` is still live but on its way to the pool: a
    hand-over from it is refused (the park would end the new fade at once); the stream that took the session over can hand it on."""
    b = H.make_batch(na, models, stage=True)
    x = H.signal(256, 14, same=[(4, 10), (4, 6)])
    b.Handover(4, 10, 1.0, 64)
    b.Process(np.ascontiguousarray(x[:, :128]))
    assert b.HandoverRemaining(4) == 0 and b.IsLive(4)
    with pytest.raises(na.NeuralAudioError, match="from .*parked by the next buffer"):
        b.Handover(4, 6, 1.0, 64)
    assert b.IsParked(6)
    b.Handover(10, 6, 1.0, 64)
    b.Process(np.ascontiguousarray(x[:, 128:]))
    assert b.IsParked(4) and b.IsLive(10) and b.HandoverRemaining(6) == 0
    b.close()


def test_a_resampling_batch_counts_external_samples(na, models):
    """44.1 kHz clients: the stage runs behind the down kernel, N and R count external samples, the twin resamples too."""
    calls = [441, 100, 441, 37, 300, 441]
    x = H.signal(sum(calls), 10, same=[(4, 10)])
    ops = {1: [("handover", 4, 10, 500), ("gain", 10, 0.8, 0), ("gain", 8, 0.4, 441)], 4: [("gain", 8, 1.0, 100)]}
    y, yt, worst = H.run_scenario(na, models, x, calls, ops, resample=44100)
    print("44.1 kHz: largest error %.3f of the limit" % worst)
    assert worst > 0.0 and np.any(y[10])


# ---------------------------------------------------------------------------------------------------------------- 8

def test_many_at_once(na, models):
    """Sixteen pairs in one batch (36 rows: sixteen pairs do not fit into fewer): 16 live A1 Standard streams, each handed to a parked
    Standard or LSTM 2x8 stream, with different N and start buffers, plus single-stream ramps beside them.  Every row is held against
    its own formula."""
    n, buffers = 128, 10
    std, lstm = models[H.STD], models[H.LSTM]
    rows = 16 + 8 + 8 + 4
    x = np.stack([H.noise(n * buffers, 500 + r) for r in range(rows)])
    pairs = [(s, 16 + s) for s in range(16)]  # to: rows 16-23 Standard, 24-31 LSTM
    for f, t in pairs:
        x[t] = x[f]
    ops = {}
    for i, (f, t) in enumerate(pairs):
        ops.setdefault(1 + i % 4, []).append(("handover", f, t, [1, 50, 128, 129, 300, 511, 640, 77][i % 8] + i))
        if i % 3 == 0:
            ops[1 + i % 4].append(("gain", t, 0.5 + 0.05 * i, 40 * (i % 2)))
    ops.setdefault(2, []).extend([("gain", 32, 0.3, 200), ("gain", 33, 0.0, 0)])
    ops.setdefault(6, []).extend([("gain", 32, 1.0, 100), ("gain", 34, 1.5, 129)])

    def build(stage):
        b = na.Batch(0)
        assert b.ReserveStreams(std, 24) == 0 and b.ReserveStreams(lstm, 8) == 24 and b.ReserveStreams(std, 4) == 32
        for s in list(range(16)) + [32, 33, 34, 35]:
            b.ActivateStream(s, 1.0)
        if stage:
            b.EnableOutputStage()
        return b

    b, twin = build(True), build(False)
    contract = H.Contract(rows, live=list(range(16)) + [32, 33, 34, 35])
    worst = 0.0
    for k in range(buffers):
        for op in ops.get(k, ()):
            H.drive(b, op, True)
            H.drive(twin, op, False)
            contract.apply(op)
        blk = np.ascontiguousarray(x[:, k * n:(k + 1) * n])
        worst = max(worst, H.check_call(b.Process(blk), twin.Process(blk), contract, ("buffer", k)))
    print("sixteen pairs: largest error %.3f of the limit" % worst)
    assert all(b.IsParked(f) for f, _ in pairs) and b.NumParked() == 16
    b.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------- 9

def test_gain_handover_and_the_automatic_park_neither_allocate_nor_create(na, models):
    """A batch on a caller's stream, after one warm-up hand-over: NA_DebugDeviceResourceCalls does not move across SetStreamGain,
    Handover, the buffers of the fade, the automatic park and the buffers after it."""
    import torch
    from neuralaudio_amd import capi
    lib = capi.load_library()
    dev = torch.device("cuda", 0)
    n = 128
    stream = torch.cuda.Stream(dev)
    b = H.make_batch(na, models, stage=True, hip_stream=stream.cuda_stream)
    x = H.signal(n * 16, 11)
    dx = torch.from_numpy(x).to(dev)
    dy = torch.zeros(H.ROWS, n * 16, device=dev)
    torch.cuda.synchronize(dev)

    def step(k):
        b.ProcessDevice(dx.data_ptr() + 4 * k * n, dy.data_ptr() + 4 * k * n, n, 16 * n, 16 * n)

    step(0)
    # warm-up: a gain, a hand-over Standard -> LSTM and its park, the streams back where they were
    b.SetStreamGain(0, 0.5, 64)
    b.Handover(4, 10, 1.0, 200)
    for k in (1, 2, 3):
        step(k)
    assert b.IsParked(4)
    b.ParkStream(10)
    b.ActivateStream(4, 1.0)
    b.SetStreamGain(0, 1.0, 0)
    step(4)
    b.Synchronize()
    calls = lib.NA_DebugDeviceResourceCalls()
    b.SetStreamGain(8, 0.7, 100)
    b.Handover(4, 10, 1.0, 300)
    b.SetStreamGain(10, 0.9, 0)
    for k in range(5, 8):
        step(k)  # the fade: 384 samples hold its 300
    assert b.HandoverRemaining(10) == 0 and not b.IsParked(4)
    step(8)  # the automatic park
    assert b.IsParked(4)
    b.SetStreamGain(10, 1.0, 0)
    b.SetStreamGain(8, 1.0, 0)
    for k in range(9, 12):
        step(k)
    moved = lib.NA_DebugDeviceResourceCalls() - calls
    b.Synchronize()
    print("resource calls across gain + hand-over + fade + park + 4 buffers: %d" % moved)
    assert moved == 0
    assert not b.IsBroken() and torch.any(dy[10, 5 * n:12 * n] != 0)
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 10

def test_free_running_modes_come_back_when_the_last_entry_retires(na, models):
    """516 reserved / 512 active A1 Standard streams on the batch's own stream (the size at which test_gpu_pool.py sees the half-batch
    chains engage).  While a ramp or a fade is active the batch may run ordered; once the fade is over and the gains are 1 the
    half-batch launches are back.  Streams that took no part are the twin's bits throughout."""
    import torch
    dev = torch.device("cuda", 0)
    m = models[H.STD]
    S, act, n, buffers = 516, 512, 128, 9
    knobs = any(os.environ.get(k) for k in ("NA_WN_KERNEL", "NA_WN_SPEC", "NA_HOST_HALVES", "NA_SP_T", "NA_SP_GEN", "NA_RESIDENT"))
    base = np.stack([H.noise(n * buffers, 10 + r) for r in range(7)])
    x = base[np.arange(S) % 7].copy()
    x[514] = x[7]

    def build(stage):
        b = na.Batch(0)
        assert b.ReserveStreams(m, S) == 0
        for s in range(act):
            b.ActivateStream(s, 1.0)
        if stage:
            b.EnableOutputStage()
        return b

    b, twin = build(True), build(False)
    dx = torch.from_numpy(x).to(dev)
    dy = torch.zeros(S, n * buffers, device=dev)
    torch.cuda.synchronize(dev)

    def step(k):
        b.ProcessDevice(dx.data_ptr() + 4 * k * n, dy.data_ptr() + 4 * k * n, n, buffers * n, buffers * n)

    step(0)
    step(1)
    b.WaitOutputs()
    assert knobs or b.UsesHalfLaunches()
    b.SetStreamGain(3, 0.5, 64)
    b.Handover(7, 514, 1.0, 200)
    step(2)
    step(3)
    ordered = not b.UsesHalfLaunches()
    b.SetStreamGain(3, 1.0, 64)
    step(4)  # the automatic park of 7; the ramp back ends in this buffer
    assert b.IsParked(7) and b.HandoverRemaining(514) == 0
    step(5)
    step(6)
    b.WaitOutputs()
    print("ordered while entries existed: %s; half-batch launches afterwards: %s" % (ordered, b.UsesHalfLaunches()))
    assert knobs or b.UsesHalfLaunches()
    step(7)
    step(8)
    b.Synchronize()
    got = dy.cpu().numpy()
    want = []
    for k in range(buffers):
        if k == 2:
            twin.ActivateStream(514, 1.0)
        want.append(twin.Process(np.ascontiguousarray(x[:, k * n:(k + 1) * n])))
    want = np.concatenate(want, axis=1)
    for r in (0, 6, 8, 255, 256, 511):
        assert np.array_equal(got[r], want[r]), r
    assert np.array_equal(got[514, 4 * n:], want[514, 4 * n:]) and np.array_equal(got[3, 5 * n:], want[3, 5 * n:])
    w = (np.minimum(np.arange(2 * n), 199) + 1) / 200.0
    e = (1 - w) * want[7, 2 * n:4 * n].astype(np.float64) + w * want[514, 2 * n:4 * n]
    lim = H.REL * (np.abs(want[7, 2 * n:4 * n]) + np.abs(want[514, 2 * n:4 * n])) + H.ABS
    assert np.all(np.abs(got[514, 2 * n:4 * n] - e) <= lim)
    b.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------- 11

def test_the_rules(na, models):
    std = models[H.STD]
    b = na.Batch(0)
    assert b.AddStreams(std, 2) == 0  # not from the pool
    assert b.ReserveStreams(std, 6) == 2
    b.EnableOutputStage()
    for s in (2, 3):
        b.ActivateStream(s, 1.0)
    with pytest.raises(na.NeuralAudioError, match="did not come from ReserveStreams"):
        b.Handover(0, 4, 1.0, 64)
    with pytest.raises(na.NeuralAudioError, match="from .*is not a live stream"):
        b.Handover(5, 4, 1.0, 64)
    with pytest.raises(na.NeuralAudioError, match="from .*is not a live stream"):
        b.Handover(99, 4, 1.0, 64)
    with pytest.raises(na.NeuralAudioError, match="to .*is not a parked stream"):
        b.Handover(2, 3, 1.0, 64)
    with pytest.raises(na.NeuralAudioError, match="to .*is not a parked stream"):
        b.Handover(2, -1, 1.0, 64)
    with pytest.raises(na.NeuralAudioError, match="the same stream"):
        b.Handover(2, 2, 1.0, 64)
    for bad in (-1, (1 << 20) + 1):
        with pytest.raises(na.NeuralAudioError, match="fadeSamples must lie in"):
            b.Handover(2, 4, 1.0, bad)
        with pytest.raises(na.NeuralAudioError, match="rampSamples must lie in"):
            b.SetStreamGain(2, 0.5, bad)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(na.NeuralAudioError, match="gain must be finite and >= 0"):
            b.SetStreamGain(2, bad, 0)
    for bad in (4, 99, -1):  # parked, out of range
        with pytest.raises(na.NeuralAudioError, match="not a live stream"):
            b.SetStreamGain(bad, 0.5, 0)
    with pytest.raises(na.NeuralAudioError, match="not a stream of the batch"):
        b.GetStreamGain(99)
    assert b.GetStreamGain(4) == 1.0 and b.GetStreamGain(0) == 1.0 and b.HandoverRemaining(2) == 0
    assert b.IsParked(4) and b.NumParked() == 4, "a refused hand-over activates nothing"
    b.Handover(2, 4, 1.0, 1 << 20)
    assert b.HandoverRemaining(2) == b.HandoverRemaining(4) == 1 << 20 and b.IsLive(4)
    for call in (lambda: b.Handover(2, 5, 1.0, 64), lambda: b.Handover(4, 5, 1.0, 64)):
        with pytest.raises(na.NeuralAudioError, match="from .*is part of a running fade"):
            call()
    b.ParkStream(4)  # cancels it
    assert b.HandoverRemaining(2) == 0 and b.IsLive(2)
    b.SetStreamGain(0, 0.5, 0)  # (streams that did not come from the pool have gains too)
    # gains are not part of a snapshot; LoadStreams leaves the destination's gain alone
    b.SetStreamGain(3, 0.25, 0)
    blob = b.SaveStreams([2])
    b.LoadStreams([3], blob)
    assert b.GetStreamGain(3) == 0.25 and b.GetStreamGain(2) == 1.0
    # park resets the gain
    b.ParkStream(3)
    assert b.GetStreamGain(3) == 1.0
    b.RemoveStreams(0)
    assert b.AddStreams(std, 1) == 0 and b.GetStreamGain(0) == 1.0
    b.close()


@pytest.mark.parametrize("who", ["to", "from"])
def test_a_park_in_mid_fade(na, models, who):
    """Parking `to` cancels the fade, parking `from` completes it at once; the other stream carries on alone at its own gain from the
    next buffer on."""
    f, t = 4, 10
    calls = [128, 128, 64, 128, 128]
    x = H.signal(sum(calls), 12, same=[(f, t)])
    ops = {1: [("handover", f, t, 1000), ("gain", f, 0.5, 0), ("gain", t, 0.8, 0)], 3: [("park", t if who == "to" else f)]}

    def hook(b, contract, i):
        if i == 3:
            assert b.HandoverRemaining(f) == b.HandoverRemaining(t) == 0
            assert b.IsParked(t if who == "to" else f) and b.IsLive(f if who == "to" else t)
            assert b.GetStreamGain(t if who == "to" else f) == 1.0

    y, yt, worst = H.run_scenario(na, models, x, calls, ops, hook=hook)
    print("park of `%s` in mid-fade: largest error %.3f of the limit" % (who, worst))
    tail = sum(calls[:3])
    alone, gain = (f, 0.5) if who == "to" else (t, 0.8)
    assert np.allclose(y[alone, tail:], np.float32(gain) * yt[alone, tail:], rtol=1e-6, atol=1e-9) and np.any(y[alone, tail:])


def test_a_removal_in_mid_fade(na, models):
    """NA_BatchRemoveStreams on `from` does what the park does: the fade is complete at once."""
    b = H.make_batch(na, models, stage=True)
    x = H.signal(256, 13, same=[(4, 10)])
    b.Handover(4, 10, 1.0, 1000)
    y0 = b.Process(np.ascontiguousarray(x[:, :128]))
    b.RemoveStreams(4)
    assert b.HandoverRemaining(10) == 0 and b.IsLive(10)
    y1 = b.Process(np.ascontiguousarray(x[:, 128:]))
    twin = H.make_batch(na, models, stage=False)
    twin.ActivateStream(10, 1.0)
    t0, t1 = twin.Process(np.ascontiguousarray(x[:, :128])), twin.Process(np.ascontiguousarray(x[:, 128:]))
    assert np.array_equal(y1[10], t1[10]) and not np.any(y1[4]) and not np.array_equal(y0[10], t0[10])
    b.close()
    twin.close()


def test_a_snapshot_taken_during_a_fade_continues_in_an_ordinary_stream(na, models):
    """test_gpu_snapshot.py's comparison: the blob of `to`, saved in mid-fade, loads into a stream added with NA_BatchAddStreams in
    another batch, which continues with the model's own output (the twin's row) bit for bit."""
    f, t, n = 4, 10, 128
    x = H.signal(4 * n, 14, same=[(f, t)])
    b = H.make_batch(na, models, stage=True)
    twin = H.make_batch(na, models, stage=False)
    blk = lambda k: np.ascontiguousarray(x[:, k * n:(k + 1) * n])
    b.Process(blk(0))
    twin.Process(blk(0))
    b.Handover(f, t, 1.0, 3 * n)
    b.SetStreamGain(t, 0.5, 0)
    twin.ActivateStream(t, 1.0)
    b.Process(blk(1))
    twin.Process(blk(1))
    blob = b.SaveStreams([t])
    assert b.HandoverRemaining(t) == 2 * n, "saving changes nothing"
    c = na.Batch(0)
    c.AddStreams(models[H.LSTM], 1, doPrewarm=False)
    c.LoadStreams([0], blob)
    for k in (2, 3):
        want = twin.Process(blk(k))[t]
        assert np.array_equal(c.Process(blk(k)[t:t + 1])[0], want), k
    for bt in (b, twin, c):
        bt.close()


def test_a_broken_batch_refuses_the_calls(na, models):
    import torch
    b = H.make_batch(na, models, stage=True)
    b.Process(H.signal(128, 15))
    b.SetWaitLimitMs(20.0)
    b.DebugStallDevice(80.0)
    with pytest.raises(na.NeuralAudioError, match="did not answer within"):
        b.Synchronize()
    assert b.IsBroken()
    for call in (lambda: b.EnableOutputStage(), lambda: b.SetStreamGain(0, 0.5, 0), lambda: b.Handover(4, 10, 1.0, 64)):
        with pytest.raises(na.NeuralAudioError, match="broken"):
            call()
    torch.cuda.synchronize()
    b.close()
