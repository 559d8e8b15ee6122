"""GPU tests of the meter stage (NA_BatchEnableMeterStage / NA_BatchSetStreamMeter / NA_BatchReadStreamMeter, csrc/meter_stage.h,
DESIGN.md 2.14): per-stream level meters on the input row (in front of the model launches) and on the row the caller receives (behind
the output stage), a gain-reduction meter on the gate's gains, and the result path that brings the readings to the host without a wait.

Everything goes through the C ABI, beside a twin batch without the stage (tests/meter_cases.py).  The stage never writes an audio row, so
every row is the twin's, bit for bit; every quantity of a reading is a max, a min or an integer sum, so every reading equals the numpy
restatement's, field for field."""
import os

import numpy as np
import pytest

import gate_cases as G
import handover_cases as H
import meter_cases as M

FORCED = bool(os.environ.get("NA_WN_KERNEL") or os.environ.get("NA_WN_PACK") or os.environ.get("NA_WN_SPEC") or os.environ.get("NA_SP_T")
              or os.environ.get("NA_SP_GEN") or os.environ.get("NA_WN_PAD"))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(FORCED, reason="forced kernel family")]

PATHS = ("process", "registered", "submit", "device", "device-odd")
CALLS = [128, 17, 300, 128]
CLIP_IN, CLIP_OUT = 0.5, 0.05
METERED = {0: 48, 4: 32, 8: 100, 9: 48}  # packed nano, Standard, and both live LSTM rows: row -> windowSamples


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
    return capi.load_library().NA_DebugMeterLaunches


def signal(total, seed):
    """[ROWS, total] noise at 0.4 (it runs over CLIP_IN); row 4 -- A1 Standard, whose kernel clamps its input and reads NaN as silence --
    also carries the special inputs of the CPU list"""
    x = np.stack([H.noise(total, 9000 + 100 * seed + r, gain=0.4) for r in range(H.ROWS)])
    sp = M.special_inputs(CLIP_IN)
    at = 3 + 5 * np.arange(len(sp))
    at = at[at < total]
    x[4, at] = sp[:len(at)]
    return x


def meter_ops(at=0, rows=METERED):
    return {at: [("meter", s, M.params(W, CLIP_IN, CLIP_OUT)) for s, W in rows.items()]}


# ================================================================================================ 1: off is off

def test_off_is_off(na, models, launches):
    """The stage is enabled and no stream has a meter: every path gives the twin's bits and launches none of the stage's kernels."""
    x = signal(sum(CALLS), 1)
    before = launches()
    for path in PATHS:
        y, yt, _, _ = M.run_scenario(na, models, x, CALLS, {}, path=path)
        assert np.array_equal(y, yt), path
        assert np.any(y[0]) and np.any(y[4]) and np.any(y[8]) and not np.any(y[2])
    assert launches() == before


def test_off_is_off_for_the_half_batch_launches(na, models, launches):
    """512 A1 Standard streams on the batch's own stream, device pointers: with the stage enabled and no meter the free-running mode
    engages as in the twin; one meter orders the launches; taken away, the mode is back with the next call.  The bits are the twin's
    throughout, and the one call with an entry made two launches."""
    import torch
    dev = torch.device("cuda", 0)
    S, n, K = 512, 128, 5
    x = np.stack([H.noise(K * n, 60 + r) for r in range(5)])[np.arange(S) % 5]
    dx = torch.from_numpy(x).to(dev)
    torch.cuda.synchronize(dev)
    halves, outs = {}, {}
    for stage in (True, False):
        b = na.Batch(0)
        assert b.ReserveStreams(models[H.STD], S) == 0
        for s in range(S):
            b.ActivateStream(s, 1.0)
        if stage:
            b.EnableMeterStage()
        dy = torch.zeros(S, K * n, device=dev)
        before = launches()
        for k in range(K):
            if stage and k == 2:
                b.SetStreamMeter(7, M.params(64, CLIP_IN, CLIP_OUT))
            if stage and k == 3:
                b.SetStreamMeter(7, None)
            b.ProcessDevice(dx.data_ptr() + 4 * k * n, dy.data_ptr() + 4 * k * n, n, K * n, K * n)
            b.Synchronize()
            halves[(stage, k)] = b.UsesHalfLaunches()
            if stage and k == 2:
                ref = M.MeterRef(M.params(64, CLIP_IN, CLIP_OUT))
                ref.feed(x[7, 2 * n:3 * n], dy[7, 2 * n:3 * n].cpu().numpy())
                assert M.norm(b.ReadStreamMeter(7)) == ref.latest() and ref.windows == 2
        assert launches() - before == (2 if stage else 0), "two launches per call with an entry"
        outs[stage] = dy.cpu().numpy()
        b.close()
    for k in (0, 1, 3, 4):
        assert halves[(True, k)] == halves[(False, k)], k
    print("half-batch launches: twin %s, with a meter %s, behind it %s" % (halves[(False, 1)], halves[(True, 2)], halves[(True, 3)]))
    assert not halves[(True, 2)]
    assert np.array_equal(outs[True], outs[False])


# ================================================================================================ 2, 3: never the audio, always the restatement

_by_window = {}


@pytest.mark.parametrize("path", PATHS)
def test_meters_on_one_stream_of_each_family(na, models, launches, path):
    """Meters on rows 0 (packed nano), 4 (Standard, with the special inputs), 8 and 9 (LSTM), W = 48, 32, 100, 48, in calls of
    [128, 17, 300, 128]: every row of every call is the twin's (run_scenario), and behind a synchronise every field of every reading --
    `windows` too -- is the restatement's: the IN tap on the input rows, the OUT tap on the twin's output rows.  Two launches per call.
    The readings of a window are the same on every path."""
    x = signal(sum(CALLS), 2)
    seen = {}

    def hook(b, contract, i):
        for s in METERED:
            r = M.norm(b.ReadStreamMeter(s))
            if r is not None:
                seen[(s, r["windows"])] = r

    before = launches()
    _, _, contract, last = M.run_scenario(na, models, x, CALLS, meter_ops(), path=path, hook=hook)
    assert launches() - before == 2 * len(CALLS)
    for s, W in METERED.items():
        assert last[s]["windows"] == sum(CALLS) // W and last[s]["windowSamples"] == W
        assert last[s]["in"]["oversTotal"] > 0 and last[s]["out"]["oversTotal"] > 0, "the condition on the inputs: both taps count overs"
        assert last[s]["gateGainMin"] == M.bits(1.0) and last[s]["gateGainLast"] == M.bits(1.0), "no gate stage: 1"
    assert last[4]["in"]["peakHold"] == M.bits(1e18), "the special inputs went through the IN tap"
    for key, r in seen.items():
        assert _by_window.setdefault(key, r) == r, (path, key)


@pytest.mark.parametrize("calls", [[1, 63, 64, 65], [145, 300]], ids=["1-63-64-65", "145-300"])
def test_the_cut_into_calls_never_shows(na, models, calls):
    """The same signal in calls of [1, 63, 64, 65] and in a call of 300 behind one of 145 (six windows of 48 complete inside it; the
    reading is the last one's): each reading is the restatement's, and at the positions the cuts share with [128, 17, 300, 128] -- 128,
    145 and 445 -- the readings equal those that cut gave."""
    x = signal(sum(CALLS), 2)[:, :sum(calls)]
    seen = {}

    def hook(b, contract, i):
        for s in METERED:
            r = M.norm(b.ReadStreamMeter(s))
            if r is not None:
                seen[(s, r["windows"])] = r

    _, _, _, last = M.run_scenario(na, models, x, calls, meter_ops(), hook=hook)
    assert last[0]["windows"] == sum(calls) // 48
    shared = [key for key in seen if key in _by_window]
    assert shared or not _by_window
    for key in shared:
        assert seen[key] == _by_window[key], key


@pytest.mark.parametrize("window", [32, 100, 32768])
def test_a_window_at_the_energy_limit(na, models, window):
    """Row 4 takes |x| >= 8 throughout (8, 1e30, inf, 9.5 in turn), W = 32, 100 and 32768: energy == W * 2^48 -- 2^63 exactly for the
    longest window -- while the peak reads 1e18; the window completes in the second of two calls."""
    total = window
    x = signal(total, 3)
    x[4] = np.tile(np.array([8.0, -1e30, np.inf, 9.5], np.float32), total // 4 + 1)[:total]
    calls = [total - 12, 12]
    _, _, _, last = M.run_scenario(na, models, x, calls, {0: [("meter", 4, M.params(window, 8.0, CLIP_OUT))]})
    assert last[4]["windows"] == 1 and last[4]["in"]["energy"] == window << 48 and last[4]["in"]["overs"] == window
    assert last[4]["in"]["peak"] == M.bits(1e18)
    if window == 32768:
        assert last[4]["in"]["energy"] == 1 << 63


def test_on_a_resampling_batch_positions_count_external_samples(na, models):
    """A 44.1 kHz batch: the IN tap reads the external-rate rows the caller passed, the OUT tap the rows it receives, and windows
    count the caller's samples."""
    x = signal(sum(CALLS), 4)
    _, _, _, last = M.run_scenario(na, models, x, CALLS, meter_ops(), resample=44100)
    for s, W in METERED.items():
        assert last[s]["windows"] == sum(CALLS) // W


def test_in_place(na, models):
    """NA_BatchProcessDevice with dIn == dOut on metered streams: the IN tap has read the input before any model writes -- the readings
    are those of separate buffers (the restatement's), and so are the rows."""
    import torch
    dev = torch.device("cuda", 0)
    x = signal(sum(CALLS), 5)
    yt = np.concatenate(H.run_twin(na, models, x, CALLS, {}), axis=1)
    b = M.make_batch(na, models, meter=True)
    refs = {}
    for s, W in METERED.items():
        b.SetStreamMeter(s, M.params(W, CLIP_IN, CLIP_OUT))
        refs[s] = M.MeterRef(M.params(W, CLIP_IN, CLIP_OUT))
    pos = 0
    for n in CALLS:
        buf = torch.from_numpy(np.ascontiguousarray(x[:, pos:pos + n])).to(dev)
        torch.cuda.synchronize(dev)
        b.ProcessDevice(buf.data_ptr(), buf.data_ptr(), n, n, n)
        b.Synchronize()
        rows = buf.cpu().numpy()
        for s in H.LIVE:
            assert np.array_equal(rows[s], yt[s, pos:pos + n]), s
        for s, ref in refs.items():
            ref.feed(x[s, pos:pos + n], yt[s, pos:pos + n])
            assert M.norm(b.ReadStreamMeter(s)) == ref.latest(), (s, pos)
        pos += n
    b.close()


# ================================================================================================ 4: the GATE tap

def test_the_gate_tap(na, models):
    """Row 4 is gated (floor 0) and metered, row 5 metered alone, W = 48, over a signal that closes the gate and reopens it:
    gateGainMin / gateGainLast are the min / last of the gate reference's gains over each window (run_scenario) -- an exact 0.0 while
    shut, an exact 1.0 while open, ramps between --, row 5 reads 1.0 throughout, and once the gate has been taken away and its tail has
    ended row 4 reads 1.0 again."""
    calls = [300, 190, 67, 17, 300, 500, 96, 96]
    x = np.stack([G.gate_signal(300 + r, sum(calls)) for r in range(H.ROWS)])
    p = G.params(floorGain=0.0)
    ops = {0: [("gate", 4, p, True), ("meter", 4, M.params(48, 0.1, 0.01)), ("meter", 5, M.params(48, 0.1, 0.01))], 6: [("ungate", 4)]}
    seen = {4: [], 5: []}

    def hook(b, contract, i):
        for s in seen:
            seen[s].append(M.norm(b.ReadStreamMeter(s)))

    _, _, contract, last = M.run_scenario(na, models, x, calls, ops, gate=True, hook=hook)
    mins = [r["gateGainMin"] for r in seen[4][:6]]
    lasts = [r["gateGainLast"] for r in seen[4][:6]]
    assert M.bits(0.0) in mins and M.bits(0.0) in lasts, "a window with the gate shut"
    assert M.bits(1.0) in mins, "a window with the gate open throughout"
    assert any(0 < v < M.bits(1.0) for v in lasts), "a window that ends on a ramp"
    assert all(r["gateGainMin"] == M.bits(1.0) and r["gateGainLast"] == M.bits(1.0) for r in seen[5])
    assert contract.gates.gate[4] is None, "the removal's tail (attackSamples 32) ended inside call 6"
    assert last[4]["gateGainMin"] == M.bits(1.0) and last[4]["windows"] == sum(calls) // 48


# ================================================================================================ 5: the result path

def test_a_read_never_waits_and_says_which_window_it_is(na, models):
    """ReadStreamMeter straight after ProcessDevice, no synchronise: whatever it returns is the restatement's reading for the window
    index it reports, never one ahead of the samples handed in; after a synchronise it is the newest."""
    import torch
    dev = torch.device("cuda", 0)
    calls = [64] * 12
    x = signal(sum(calls), 6)
    yt = np.concatenate(H.run_twin(na, models, x, calls, {}), axis=1)
    b = M.make_batch(na, models, meter=True)
    p = M.params(48, CLIP_IN, CLIP_OUT)
    b.SetStreamMeter(4, p)
    ref = M.MeterRef(p)
    dx, dy = torch.from_numpy(x).to(dev), torch.zeros(H.ROWS, sum(calls), device=dev)
    torch.cuda.synchronize(dev)
    pos, arrived = 0, []
    for n in calls:
        b.ProcessDevice(dx.data_ptr() + 4 * pos, dy.data_ptr() + 4 * pos, n, sum(calls), sum(calls))
        ref.feed(x[4, pos:pos + n], yt[4, pos:pos + n])
        r = M.norm(b.ReadStreamMeter(4))
        if r is not None:
            assert 1 <= r["windows"] <= ref.windows and r == ref.reading(r["windows"] - 1), (pos, r)
            arrived.append(r["windows"])
        pos += n
    b.Synchronize()
    assert M.norm(b.ReadStreamMeter(4)) == ref.latest() and ref.windows == 16
    assert arrived == sorted(arrived), "readings never go back"
    print("windows read without a wait, call by call:", arrived)
    b.close()


def test_nothing_from_before_a_restart_or_a_removal_is_read_again(na, models):
    """A restart mid-window: no reading until the new meter's first window completes, then that window's -- also when the records of
    the earlier meter are still on their way at the restart (no synchronise in front of it).  A removal makes Read return 0; a meter
    set again on the row starts from nothing."""
    x = signal(400, 7)
    yt = np.concatenate(H.run_twin(na, models, x, [100, 30, 30, 100, 10, 60, 70], {}), axis=1)
    b = M.make_batch(na, models, meter=True)
    p = M.params(48, CLIP_IN, CLIP_OUT)

    def call(lo, hi, sync=True):
        y = b.Process(np.ascontiguousarray(x[:, lo:hi]))
        assert np.array_equal(y, yt[:, lo:hi])
        if sync:
            b.Synchronize()

    def fresh(lo, hi):
        ref = M.MeterRef(p)
        ref.feed(x[4, lo:hi], yt[4, lo:hi])
        return ref.latest()

    b.SetStreamMeter(4, p)
    call(0, 100)
    assert M.norm(b.ReadStreamMeter(4)) == fresh(0, 100) and fresh(0, 100)["windows"] == 2
    b.SetStreamMeter(4, p)  # position 100: 4 samples into the third window
    assert b.ReadStreamMeter(4) is None and b.GetStreamMeter(4) == p
    call(100, 130)
    assert b.ReadStreamMeter(4) is None, "30 samples of the new meter: no window yet, and not the old meter's"
    call(130, 160)
    assert M.norm(b.ReadStreamMeter(4)) == fresh(100, 160) and fresh(100, 160)["windows"] == 1
    # the device path leaves the records in flight: restart right behind the call
    import torch
    dev = torch.device("cuda", 0)
    dx = torch.from_numpy(np.ascontiguousarray(x[:, 160:260])).to(dev)
    dy = torch.zeros(H.ROWS, 100, device=dev)
    torch.cuda.synchronize(dev)
    b.ProcessDevice(dx.data_ptr(), dy.data_ptr(), 100, 100, 100)
    b.SetStreamMeter(4, p)
    assert b.ReadStreamMeter(4) is None
    call(260, 270)
    assert b.ReadStreamMeter(4) is None, "the earlier meter's records have arrived by now and were dropped"
    call(270, 330)
    assert M.norm(b.ReadStreamMeter(4)) == fresh(260, 330)
    b.SetStreamMeter(4, None)
    assert b.ReadStreamMeter(4) is None and b.GetStreamMeter(4) is None and b.GetMeterInfo()["numMeters"] == 0
    b.SetStreamMeter(4, p)
    assert b.ReadStreamMeter(4) is None
    call(330, 400)
    assert M.norm(b.ReadStreamMeter(4)) == fresh(330, 400)
    b.close()


def test_rules(na, models):
    """Each refusal carries its text; park, remove and the park that ends a hand-over drop the meter; GetMeterInfo counts entries and
    bytes; save and load leave meters alone; a broken batch refuses everything."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    b = H.make_batch(na, models, stage=True)  # (with the output stage, for the hand-over)
    p = M.params(64, 1.0, 1.0)
    for call in (lambda: b.SetStreamMeter(0, p), lambda: b.SetStreamMeter(0, None), lambda: b.GetStreamMeter(0), lambda: b.ReadStreamMeter(0), lambda: b.GetMeterInfo()):
        with pytest.raises(na.NeuralAudioError, match=r"meter stage not enabled \(NA_BatchEnableMeterStage\)"):
            call()
    assert lib.NA_BatchGetStreamMeter(b._h, 0, None) < 0 and lib.NA_BatchReadStreamMeter(b._h, 0, None) < 0
    b.EnableMeterStage()
    b.EnableMeterStage()
    info = b.GetMeterInfo()
    assert info["numMeters"] == 0 and info["deviceBytes"] >= 16 * 176 + 4 * 16 * (32 + 96)
    with pytest.raises(na.NeuralAudioError, match="SetStreamMeter: stream 2 is parked"):
        b.SetStreamMeter(2, p)
    with pytest.raises(na.NeuralAudioError, match="SetStreamMeter: stream 12 is not a live stream of the batch"):
        b.SetStreamMeter(12, p)
    with pytest.raises(na.NeuralAudioError, match="GetStreamMeter: stream 12 is not a stream of the batch"):
        b.GetStreamMeter(12)
    with pytest.raises(na.NeuralAudioError, match="ReadStreamMeter: stream -1 is not a stream of the batch"):
        b.ReadStreamMeter(-1)
    for change, text in ((dict(window=31), r"windowSamples must lie in \[32, 32768\]"), (dict(window=32769), r"windowSamples must lie in \[32, 32768\]"),
                         (dict(clip_in=0.0), "clipLevelIn must be finite and > 0"), (dict(clip_in=float("inf")), "clipLevelIn must be finite and > 0"),
                         (dict(clip_out=float("nan")), "clipLevelOut must be finite and > 0"), (dict(clip_out=-0.5), "clipLevelOut must be finite and > 0")):
        with pytest.raises(na.NeuralAudioError, match="SetStreamMeter: " + text):
            b.SetStreamMeter(0, M.params(**change))
    assert b.GetMeterInfo()["numMeters"] == 0 and b.GetStreamMeter(0) is None and b.ReadStreamMeter(0) is None
    b.SetStreamMeter(1, None)  # (no meter: nothing to take away)
    for s in (0, 1, 4, 5, 8):
        b.SetStreamMeter(s, p)
    assert b.GetMeterInfo()["numMeters"] == 5 and b.GetStreamMeter(4) == p and b.GetMeterInfo()["deviceBytes"] == info["deviceBytes"]
    x = signal(64, 8)
    b.Process(x)
    b.Synchronize()
    assert b.ReadStreamMeter(0)["windows"] == 1
    b.ParkStream(0)
    assert b.GetMeterInfo()["numMeters"] == 4 and b.GetStreamMeter(0) is None and b.ReadStreamMeter(0) is None
    b.ActivateStream(0, 1.0)
    assert b.GetStreamMeter(0) is None and b.ReadStreamMeter(0) is None
    blob = b.SaveStreams([5])
    b.LoadStreams([4], blob)
    assert b.GetStreamMeter(4) == p and b.GetMeterInfo()["numMeters"] == 4
    b.Handover(4, 6, 1.0, 64)
    b.Process(x)
    assert b.GetStreamMeter(4) is not None and b.GetStreamMeter(6) is None
    b.Process(x)  # (parks row 4 in front of its launches)
    assert b.IsParked(4) and b.GetStreamMeter(4) is None and b.GetMeterInfo()["numMeters"] == 3
    # the stage grows with the batch
    first = b.ReserveStreams(models[H.LSTM], 30)
    b.ActivateStream(first + 29, 1.0)
    b.SetStreamMeter(first + 29, p)
    assert b.GetMeterInfo()["deviceBytes"] > info["deviceBytes"]
    b.Process(signal(64, 9)[np.arange(b.NumStreams()) % H.ROWS])
    b.Synchronize()
    assert b.ReadStreamMeter(first + 29)["windows"] == 1 and b.GetStreamMeter(1) is not None
    # a broken batch refuses everything
    b.SetWaitLimitMs(20.0)
    b.DebugStallDevice(80.0)
    with pytest.raises(na.NeuralAudioError, match="did not answer within"):
        b.Synchronize()
    assert b.IsBroken()
    for call in (lambda: b.SetStreamMeter(1, p), lambda: b.SetStreamMeter(1, None), lambda: b.ReadStreamMeter(1), lambda: b.EnableMeterStage()):
        with pytest.raises(na.NeuralAudioError, match="broken"):
            call()
    assert lib.NA_BatchReadStreamMeter(b._h, 1, None) < 0
    b.close()


def test_remove_streams_drops_the_meter(na, models):
    b = na.Batch(0)
    assert b.AddStreams(models[H.LSTM], 4) == 0
    b.EnableMeterStage()
    b.SetStreamMeter(1, M.params())
    b.SetStreamMeter(2, M.params())
    b.RemoveStreams(1, 1)
    assert b.GetMeterInfo()["numMeters"] == 1
    assert b.AddStreams(models[H.LSTM], 1) == 1 and b.GetStreamMeter(1) is None and b.GetStreamMeter(2) is not None
    b.close()


def test_set_read_and_processing_calls_are_real_time_safe(na, models, launches):
    """NA_DebugDeviceResourceCalls stays where it is across set, restart, remove and read calls and 21 processing calls with entries,
    over the blocking and the pipelined host path and device pointers (after three warm calls of each, which size the staging block
    and the pipeline slots); NA_DebugMeterLaunches moves by exactly two per call with an entry."""
    import torch
    from neuralaudio_amd import capi
    lib = capi.load_library()
    dev = torch.device("cuda", 0)
    b = M.make_batch(na, models, meter=True)
    n = 128
    x = signal(n, 10)
    dx, dy = torch.from_numpy(x).to(dev), torch.zeros(H.ROWS, n, device=dev)
    torch.cuda.synchronize(dev)

    def three():
        b.Process(x)
        b.ReadStreamMeter(0)
        b.Collect(b.Submit(x))
        b.ReadStreamMeter(0)
        b.ProcessDevice(dx.data_ptr(), dy.data_ptr(), n, n, n)
        b.ReadStreamMeter(0)
        b.Synchronize()

    b.SetStreamMeter(0, M.params(48))
    for _ in range(3):
        three()
    before, count = lib.NA_DebugDeviceResourceCalls(), launches()
    b.SetStreamMeter(4, M.params(32))
    b.SetStreamMeter(8, M.params(100))
    for i in range(7):
        three()
        if i == 2:
            b.SetStreamMeter(0, M.params(64))
            b.SetStreamMeter(8, None)
        if i == 4:
            b.SetStreamMeter(9, M.params(1024))
            b.SetStreamMeter(4, None)
    assert b.GetStreamMeter(8) is None and b.GetMeterInfo()["numMeters"] == 2 and b.ReadStreamMeter(0)["windowSamples"] == 64
    assert lib.NA_DebugDeviceResourceCalls() == before
    assert launches() - count == 2 * 21
    b.SetStreamMeter(0, None)
    b.SetStreamMeter(9, None)
    three()
    assert launches() - count == 2 * 21, "no entry: no launch"
    b.close()


@pytest.mark.parametrize("streams,path", [(65, "process"), (257, "device-odd")])
def test_every_entry_gets_its_own_reading(na, models, streams, path):
    """65 and 257 BossLSTM-2x8 streams, every one metered with its own window and its own input: a table of more entries than a wave
    has lanes and than one byte counts; every entry's reading is its own restatement's.  device-odd: an odd row stride and rows that
    are not 16-byte aligned."""
    S = streams
    calls = [130, 129]
    x = np.stack([H.noise(sum(calls), 4000 + r, gain=0.1 + 0.01 * (r % 50)) for r in range(S)])
    batches = {}
    for stage in (False, True):
        b = na.Batch(0)
        assert b.AddStreams(models[H.LSTM], S) == 0
        if stage:
            b.EnableMeterStage()
        batches[stage] = b
    runner, twin = H.Runner(na, batches[True], path), batches[False]
    refs = {}
    try:
        for r in range(S):
            p = M.params(32 + r % 90, 0.2, 0.01 * (1 + r % 5))
            batches[True].SetStreamMeter(r, p)
            refs[r] = M.MeterRef(p)
        assert batches[True].GetMeterInfo()["numMeters"] == S
        pos = 0
        for n in calls:
            xs = np.ascontiguousarray(x[:, pos:pos + n])
            yt, y = twin.Process(xs), runner.call(xs)
            assert np.array_equal(y, yt)
            batches[True].Synchronize()
            for r in range(S):
                refs[r].feed(xs[r], yt[r])
                assert M.norm(batches[True].ReadStreamMeter(r)) == refs[r].latest(), (path, pos, r)
            pos += n
        assert len({M.norm(batches[True].ReadStreamMeter(r))["in"]["energy"] for r in range(S)}) > S // 2
    finally:
        runner.close()
        for b in batches.values():
            b.close()
