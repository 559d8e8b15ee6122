"""GPU tests of the gate stage (NA_BatchEnableGateStage / NA_BatchSetStreamGate, csrc/gate_stage.h): a per-stream noise
gate whose detector reads the input rows in front of the model launches and whose gain scales the rows behind them, in front of the
cabinet and output stages.

Everything goes through the C ABI, beside a twin batch without the stage (tests/gate_cases.py, as tests/test_gpu_handover.py does).  The
contract is bit-exact: the expected row of a gated stream is fl(twin_row * g_ref) with g_ref from the numpy float32 restatement, of any
other stream the twin's row, and every comparison is np.array_equal."""
import os

import numpy as np
import pytest

import gate_cases as G
import handover_cases as H

FORCED = bool(os.environ.get("NA_WN_KERNEL") or os.environ.get("NA_WN_PACK") or os.environ.get("NA_WN_SPEC") or os.environ.get("NA_SP_T")
              or os.environ.get("NA_SP_GEN") or os.environ.get("NA_WN_PAD"))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(FORCED, reason="forced kernel family")]

PATHS = ("process", "registered", "submit", "device", "device-odd")
GATED = {0: "floor0", 4: "floor0.1", 8: "attack1", 9: "hold0"}  # packed nano, Standard, and both live LSTM rows


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
    return capi.load_library().NA_DebugGateLaunches


def signal(total=G.TOTAL, seed=0, lead=0):
    """[ROWS, total]: every row alternates bursts and quiet stretches, each from its own noise"""
    return np.stack([G.gate_signal(100 * seed + r, total, lead) for r in range(H.ROWS)])


# ================================================================================================ 1: off is off

def test_off_is_off(na, models, launches):
    """The stage is enabled and no stream has a gate: every path gives the twin's bits and launches none of the stage's kernels."""
    calls = [128, 17, 300, 128]
    x = signal(sum(calls), 1)
    before = launches()
    for path in PATHS:
        y, yt, _ = G.run_scenario(na, models, x, calls, {}, path=path)
        assert np.array_equal(y, yt), path
        assert np.any(y[0]) and np.any(y[4]) and np.any(y[8]) and not np.any(y[2])
    assert launches() == before


def test_off_is_off_for_the_half_batch_launches(na, models, launches):
    """512 A1 Standard streams on the batch's own stream, device pointers: with the stage enabled and no gate the free-running mode
    engages as in the twin and the bits are the twin's; a gate on one stream orders the launches; taken away again (attackSamples 32:
    the tail ends inside the next call), the mode comes back with the call after."""
    import torch
    dev = torch.device("cuda", 0)
    S, n, K = 512, 128, 5
    x = np.stack([G.gate_signal(60 + r, K * n) for r in range(5)])[np.arange(S) % 5]
    dx = torch.from_numpy(x).to(dev)
    torch.cuda.synchronize(dev)
    halves, outs = {}, {}
    p = G.params()
    for stage in (True, False):
        b = na.Batch(0)
        assert b.ReserveStreams(models[H.STD], S) == 0
        for s in range(S):
            b.ActivateStream(s, 1.0)
        if stage:
            b.EnableGateStage()
        dy = torch.zeros(S, K * n, device=dev)
        before = launches()
        for k in range(K):
            if stage and k == 2:
                b.SetStreamGate(7, p, True)
            if stage and k == 3:
                b.SetStreamGate(7, None)
            b.ProcessDevice(dx.data_ptr() + 4 * k * n, dy.data_ptr() + 4 * k * n, n, K * n, K * n)
            b.Synchronize()
            halves[(stage, k)] = b.UsesHalfLaunches()
        assert launches() - before == (4 if stage else 0), "two launches per call with an entry"
        outs[stage] = dy.cpu().numpy()
        b.close()
    for k in (0, 1, 4):
        assert halves[(True, k)] == halves[(False, k)], k
    print("half-batch launches: twin %s, with a gate %s, in the removal's tail %s, behind it %s" % (halves[(False, 1)], halves[(True, 2)], halves[(True, 3)], halves[(True, 4)]))
    assert not halves[(True, 2)] and not halves[(True, 3)]
    ref = G.GateRef(p, True)
    g = ref.run(x[7, 2 * n:3 * n])
    ref.remove()
    g = np.concatenate([g, ref.run(x[7, 3 * n:4 * n])])
    expect = outs[False].copy()
    expect[7, 2 * n:4 * n] = outs[False][7, 2 * n:4 * n] * g
    assert ref.retired and np.array_equal(outs[True], expect)


# ================================================================================================ 2, 3: the gate itself

def _gate_ops(at=0):
    return {at: [("gate", s, G.variation(name), True) for s, name in GATED.items()]}


def _assert_inputs_cover_every_case(x):
    """the condition on the inputs: the reference's own gain sequence on every gated row shows every case"""
    for s, name in GATED.items():
        ref = G.GateRef(G.variation(name), True)
        G.assert_covered(ref, ref.run(x[s]), ("row", s, name))


@pytest.mark.parametrize("path", PATHS)
def test_gates_on_one_stream_of_each_family(na, models, launches, path):
    """Gates on rows 0 (packed nano), 4 (Standard), 8 and 9 (LSTM), one variation each, over the whole test signal.  Call lengths: the
    RAGGED list, 127, 128, 129, and one call of 2049 -- longer than a tile and than the first gainSamples, so it grows the gain block.
    Every row of every call is checked (run_scenario), the packed neighbours of row 0 among them.  With floorGain = 0 the closed
    stretches are exact zeros where the twin's are not."""
    x = signal(seed=2)
    _assert_inputs_cover_every_case(x)
    calls = list(H.RAGGED) + [127, 128, 129, 2049]
    calls.append(G.TOTAL - sum(calls))
    assert calls[-1] > 0
    seen = {}

    def hook(b, contract, i):
        seen[i] = b.GetGateInfo()

    before = launches()
    y, yt, contract = G.run_scenario(na, models, x, calls, _gate_ops(), path=path, hook=hook)
    assert launches() - before == 2 * len(calls), "two launches per call, whatever n"
    grow = calls.index(2049)
    assert seen[grow - 1]["gainSamples"] == 2048 and seen[grow]["gainSamples"] == 4096 and seen[0]["numGates"] == 4
    assert seen[grow]["deviceBytes"] > seen[grow - 1]["deviceBytes"] >= 16 * (2048 * 4 + 16)
    g0 = np.concatenate(contract.gains[0])
    closed = g0 == 0.0
    assert np.count_nonzero(closed) > 200 and not np.any(y[0][closed]) and np.count_nonzero(yt[0][closed]) > 200
    for s in (1, 5):
        assert np.array_equal(y[s], yt[s])


def test_the_cut_into_calls_never_shows(na, models):
    """The same 1500 samples in one call, in calls of one sample and in RAGGED lengths: the same bits (and each the reference's)."""
    total = 1500
    x = signal(total, 3)
    outs = []
    for calls in ([total], [1] * total, H.ragged(total)):
        y, _, contract = G.run_scenario(na, models, x, calls, _gate_ops())
        outs.append(y)
    g = np.concatenate(contract.gains[4])
    assert np.any(g == 1.0) and np.any(g == np.float32(0.1)) and np.any((g > np.float32(0.1)) & (g < 1.0))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


# ================================================================================================ 4: more entries than one wave

def _distinct(r):
    return G.params(detectorCoeff=0.03 + 0.001 * r, attackSamples=8 + r, holdSamples=(5 * r) % 70, releaseSamples=30 + 3 * r, floorGain=[0.0, 0.1, 0.25][r % 3],
                    openPower=1e-3 * (1.0 + 0.01 * r))


@pytest.mark.parametrize("path", ["process", "device-odd"])
def test_more_entries_than_one_wave(na, models, launches, path):
    """70 BossLSTM-2x8 streams, independent inputs, distinct constants: 1 entry, 2 entries, then 65 -- one more than a workgroup of the
    detector holds -- and 64 once one gate has been taken away.  device-odd: an odd row stride and rows that are not 16-byte aligned."""
    S = 70
    gated = [r for r in range(S) if r not in (0, 13, 31, 64, 69)]
    assert len(gated) == 65 and gated[-1] == 68
    calls = [130, 129, 300, 200, 100]
    x = np.stack([G.gate_signal(500 + r, sum(calls), lead=(7 * r) % 90) for r in range(S)])
    ops = {0: [3], 1: [40], 2: [r for r in gated if r not in (3, 40)]}
    batches = {}
    for stage in (False, True):
        b = na.Batch(0)
        assert b.AddStreams(models[H.LSTM], S) == 0
        if stage:
            b.EnableGateStage()
        batches[stage] = b
    runner, twin = H.Runner(na, batches[True], path), batches[False]
    refs, pos, counts = {}, 0, []
    before = launches()
    try:
        for i, n in enumerate(calls):
            for r in ops.get(i, ()):
                batches[True].SetStreamGate(r, _distinct(r), r % 2 == 0)
                refs[r] = G.GateRef(_distinct(r), r % 2 == 0)
            if i == 3:
                batches[True].SetStreamGate(3, None)  # attackSamples 11: gone behind this call
                refs[3].remove()
            counts.append(batches[True].GetGateInfo()["numGates"])
            xs = np.ascontiguousarray(x[:, pos:pos + n])
            yt, y = twin.Process(xs), runner.call(xs)
            for r in range(S):
                e = yt[r]
                if r in refs and not refs[r].retired:
                    e = (yt[r] * refs[r].run(xs[r])).astype(np.float32)
                assert np.array_equal(y[r], e), (path, "call", i, "row", r)
            pos += n
        assert counts == [1, 2, 65, 65, 64] and launches() - before == 2 * len(calls)
        assert batches[True].GetStreamGate(3) is None and refs[3].retired
        for r in (3, 40, 68):
            want = 1.0 if r == 3 else float(refs[r].last_g)
            assert batches[True].StreamGateGain(r) == want, r
    finally:
        runner.close()
        for b in batches.values():
            b.close()


# ================================================================================================ 5: set, change and remove

def test_set_change_and_remove(na, models, launches):
    """Row 4 gets a gate that starts closed: the first samples are floor * y and the gate opens on the first burst.  New constants
    mid-run keep the state (the reference does the same).  Taken away while closed, the row ramps up over exactly attackSamples samples;
    behind the ramp it carries the twin's bits, NA_BatchGetStreamGate answers 0 and the launch counter stands still.  On row 9 a set
    call during the tail re-arms the gate.  NA_BatchStreamGateGain equals the reference's last g after every call."""
    lead = 150
    calls = [100, 128, 300, 64, 500, 20, 20, 128, 128]
    x = signal(sum(calls), 5, lead=lead)
    p = G.params(floorGain=0.1)
    changed = G.params(floorGain=0.1, holdSamples=10, releaseSamples=20, attackSamples=40, closePower=5e-4)
    # the signal's first burst is 300 samples from `lead`, then 700 quiet: calls 4 .. 6 lie in the quiet stretch, the gates are shut
    ops = {0: [("gate", 4, p, False), ("gate", 9, p, False)], 3: [("gate", 4, changed, True), ("gate", 9, changed, True)],
           5: [("ungate", 4), ("ungate", 9)], 6: [("gate", 9, changed, True)]}
    seen, count = {}, {}

    def hook(b, contract, i):
        count[i] = launches()
        seen[i] = (b.GetStreamGate(4), b.GetStreamGate(9))
        for s in (4, 9):
            ref = contract.gate[s]
            assert b.StreamGateGain(s) == (1.0 if ref is None else float(ref.last_g)), (i, s)

    y, yt, contract = G.run_scenario(na, models, x, calls, ops, hook=hook)
    g4, g9 = np.concatenate(contract.gains[4]), np.concatenate(contract.gains[9])
    assert np.all(g4[:lead] == np.float32(0.1)), "started closed: floor * y until the first burst"
    assert np.array_equal(y[4, :lead], (yt[4, :lead] * np.float32(0.1)).astype(np.float32))
    assert np.any(g4[lead:lead + 100] == 1.0), "opened on the first burst"
    at = sum(calls[:5])
    A = changed["attackSamples"]
    ramp = g4[at:at + A]
    assert g4[at - 1] == np.float32(0.1) and np.all(np.diff(ramp) > 0) and ramp[-1] == 1.0 and ramp[-2] < 1.0, "a ramp of exactly attackSamples samples"
    assert len(g4) == at + 40, "the entry retired with the call that held the ramp's last sample"
    assert np.array_equal(y[4, at + A:], yt[4, at + A:])
    assert seen[3][0]["holdSamples"] == 10 and abs(seen[3][0]["closePower"] - 5e-4) < 1e-9 and seen[4][0] is not None
    assert seen[5][0] is None and seen[6][0] is None and seen[5][1] is None
    assert seen[6][1] is not None and contract.gate[9] is not None, "re-armed during the tail"
    assert g9[at + 20] < g9[at + 19], "row 9 was still shut: re-armed, its gain turns round"
    assert count[8] - count[7] == 2 and count[6] - count[5] == 2, "row 9 keeps the stage running; two launches per call"


def test_the_launch_counter_stops_with_the_last_entry(na, models, launches):
    b = G.make_batch(na, models, stage=True)
    x = signal(128, 6)
    b.SetStreamGate(5, G.params(attackSamples=64), True)
    b.Process(x)
    b.SetStreamGate(5, None)
    before = launches()
    b.Process(x)
    assert launches() - before == 2 and b.GetGateInfo()["numGates"] == 0
    b.Process(x)
    b.Process(x)
    assert launches() - before == 2
    b.close()


# ================================================================================================ 6: rules

def test_rules(na, models):
    """Each refusal carries its text; park, remove and the park that ends a hand-over drop the gate; an activated stream has none; save
    and load leave gates alone; a broken batch refuses everything."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    b = H.make_batch(na, models, stage=True)  # (with the output stage, for the hand-over)
    p = G.params()
    for call in (lambda: b.SetStreamGate(0, p), lambda: b.SetStreamGate(0, None), lambda: b.GetStreamGate(0), lambda: b.StreamGateGain(0), lambda: b.GetGateInfo()):
        with pytest.raises(na.NeuralAudioError, match=r"gate stage not enabled \(NA_BatchEnableGateStage\)"):
            call()
    assert lib.NA_BatchGetStreamGate(b._h, 0, None) < 0 and lib.NA_BatchStreamGateGain(b._h, 0) < 0
    b.EnableGateStage()
    b.EnableGateStage()
    info = b.GetGateInfo()
    assert info["gainSamples"] == 2048 and info["numGates"] == 0
    with pytest.raises(na.NeuralAudioError, match="SetStreamGate: stream 2 is parked"):
        b.SetStreamGate(2, p)
    with pytest.raises(na.NeuralAudioError, match="SetStreamGate: stream 12 is not a live stream of the batch"):
        b.SetStreamGate(12, p)
    with pytest.raises(na.NeuralAudioError, match="GetStreamGate: stream 12 is not a stream of the batch"):
        b.GetStreamGate(12)
    with pytest.raises(na.NeuralAudioError, match="StreamGateGain: stream -1 is not a stream of the batch"):
        b.StreamGateGain(-1)
    for change, text in ((dict(openPower=float("nan")), "openPower must be finite"), (dict(closePower=float("inf")), "closePower must be finite"),
                         (dict(floorGain=float("nan")), "floorGain must be finite"), (dict(detectorCoeff=float("inf")), "detectorCoeff must be finite"),
                         (dict(closePower=-1e-9), "closePower must be >= 0"), (dict(openPower=1e-4), "openPower must be >= closePower"),
                         (dict(floorGain=1.5), r"floorGain must lie in \[0, 1\]"), (dict(floorGain=-0.5), r"floorGain must lie in \[0, 1\]"),
                         (dict(detectorCoeff=0.0), r"detectorCoeff must lie in \(0, 1\]"), (dict(detectorCoeff=1.5), r"detectorCoeff must lie in \(0, 1\]"),
                         (dict(attackSamples=0), r"attackSamples must lie in \[1, 1 << 20\]"), (dict(attackSamples=(1 << 20) + 1), r"attackSamples must lie in \[1, 1 << 20\]"),
                         (dict(releaseSamples=0), r"releaseSamples must lie in \[1, 1 << 20\]"), (dict(holdSamples=-1), r"holdSamples must lie in \[0, 1 << 24\]"),
                         (dict(holdSamples=(1 << 24) + 1), r"holdSamples must lie in \[0, 1 << 24\]")):
        with pytest.raises(na.NeuralAudioError, match="SetStreamGate: " + text):
            b.SetStreamGate(0, G.params(**change))
    assert b.GetGateInfo()["numGates"] == 0 and b.GetStreamGate(0) is None and b.StreamGateGain(0) == 1.0
    b.SetStreamGate(0, G.params(attackSamples=1 << 20, releaseSamples=1 << 20, holdSamples=1 << 24, detectorCoeff=1.0, floorGain=1.0, closePower=0.0), False)
    assert b.StreamGateGain(0) == 1.0, "started closed at a floor of 1"
    b.SetStreamGate(0, None)
    b.SetStreamGate(1, None)  # (no gate: nothing to take away)
    # park, remove and the end of a hand-over drop the gate at once; an activated stream has none
    for s in (0, 1, 4, 5, 8):
        b.SetStreamGate(s, p, s != 5)
    assert b.GetGateInfo()["numGates"] == 5 and b.GetStreamGate(4) == b.GetStreamGate(8)
    assert b.StreamGateGain(5) == 0.0 and b.StreamGateGain(4) == 1.0, "nothing produced yet: the start"
    b.ParkStream(0)
    assert b.GetGateInfo()["numGates"] == 4 and b.GetStreamGate(0) is None
    b.ActivateStream(0, 1.0)
    assert b.GetStreamGate(0) is None and b.StreamGateGain(0) == 1.0
    blob = b.SaveStreams([5])
    b.LoadStreams([4], blob)
    assert b.GetStreamGate(4)["holdSamples"] == 50 and b.GetGateInfo()["numGates"] == 4
    b.Handover(4, 6, 1.0, 64)
    x = signal(64, 7)
    b.Process(x)
    assert b.GetStreamGate(4) is not None and b.GetStreamGate(6) is None
    b.Process(x)  # (parks row 4 in front of its launches)
    assert b.IsParked(4) and b.GetStreamGate(4) is None and b.GetGateInfo()["numGates"] == 3
    # the stage grows with the batch
    first = b.ReserveStreams(models[H.LSTM], 30)
    b.ActivateStream(first + 29, 1.0)
    b.SetStreamGate(first + 29, p, True)
    y = b.Process(signal(64, 8)[np.arange(b.NumStreams()) % H.ROWS])
    assert np.any(y[first + 29]) and np.all(np.isfinite(y)) and b.GetStreamGate(1) is not None
    # a broken batch refuses everything
    b.SetWaitLimitMs(20.0)
    b.DebugStallDevice(80.0)
    with pytest.raises(na.NeuralAudioError, match="did not answer within"):
        b.Synchronize()
    assert b.IsBroken()
    for call in (lambda: b.SetStreamGate(1, p), lambda: b.SetStreamGate(1, None), lambda: b.StreamGateGain(1), lambda: b.EnableGateStage()):
        with pytest.raises(na.NeuralAudioError, match="broken"):
            call()
    b.close()


def test_remove_streams_drops_the_gate(na, models):
    b = na.Batch(0)
    assert b.AddStreams(models[H.LSTM], 4) == 0
    b.EnableGateStage()
    b.SetStreamGate(1, G.params(), True)
    b.SetStreamGate(2, G.params(), True)
    b.RemoveStreams(1, 1)
    assert b.GetGateInfo()["numGates"] == 1
    assert b.AddStreams(models[H.LSTM], 1) == 1 and b.GetStreamGate(1) is None and b.GetStreamGate(2) is not None
    b.close()


def test_set_calls_and_processing_with_gates_are_real_time_safe(na, models):
    """NA_DebugDeviceResourceCalls stays where it is across set, change and remove calls and 21 processing calls with entries, over the
    blocking and the pipelined host path and device pointers (after three warm calls of each, which size the staging block and the
    pipeline slots)."""
    import torch
    from neuralaudio_amd import capi
    lib = capi.load_library()
    dev = torch.device("cuda", 0)
    b = G.make_batch(na, models, stage=True)
    n = 128
    x = signal(n, 9)
    dx, dy = torch.from_numpy(x).to(dev), torch.zeros(H.ROWS, n, device=dev)
    torch.cuda.synchronize(dev)

    def three():
        b.Process(x)
        b.Collect(b.Submit(x))
        b.ProcessDevice(dx.data_ptr(), dy.data_ptr(), n, n, n)
        b.Synchronize()

    b.SetStreamGate(0, G.params(), True)
    for _ in range(3):
        three()
    before = lib.NA_DebugDeviceResourceCalls()
    b.SetStreamGate(4, G.params(floorGain=0.1), False)
    b.SetStreamGate(8, G.params(), True)
    for i in range(7):
        three()
        if i == 2:
            b.SetStreamGate(0, G.params(holdSamples=3), True)
            b.SetStreamGate(8, None)
        if i == 4:
            b.SetStreamGate(9, G.params(), False)
            b.SetStreamGate(4, None)
    assert b.GetStreamGate(8) is None and b.GetStreamGate(4) is None and b.GetGateInfo()["numGates"] == 2
    assert lib.NA_DebugDeviceResourceCalls() == before
    b.close()


# ================================================================================================ 7: order with the other stages

def _twin_rows(na, models, x, calls, resample=None):
    return np.concatenate(H.run_twin(na, models, x, calls, {}, resample), axis=1)


def test_the_gate_sits_in_front_of_the_cabinet_and_the_output_gain(na, models):
    """Row 4 has a gate and the two-tap IR {0, 1} -- an exact one-sample delay by the cabinet's own rule -- so row[t] must be
    fl(y[t-1] * g[t-1]) bit for bit; a gate behind the cabinet would give y[t-1] * g[t].  Row 9 has an output gain of 0.5 on top: that
    value times 0.5 exactly."""
    calls = [128, 129, 300, 443]
    total = sum(calls)
    x = signal(total, 10)
    yt = _twin_rows(na, models, x, calls)
    b = H.make_batch(na, models, stage=True)
    b.EnableCabinetStage(64)
    b.EnableGateStage()
    delay = b.LoadIR(np.array([0.0, 1.0], np.float32))
    p = G.params(floorGain=0.1)
    refs = {}
    for s in (4, 9):
        b.SetStreamGate(s, p, True)
        b.SetStreamIR(s, delay, 0)
        refs[s] = G.GateRef(p, True)
    b.SetStreamGain(9, 0.5, 0)
    y, pos = [], 0
    for n in calls:
        y.append(b.Process(np.ascontiguousarray(x[:, pos:pos + n])))
        pos += n
    y = np.concatenate(y, axis=1)
    b.close()
    for s in (4, 9):
        g = refs[s].run(x[s])
        assert np.any(g[1:] != g[:-1])
        gated = (yt[s] * g).astype(np.float32)
        expect = np.concatenate([np.zeros(1, np.float32), gated[:-1]])
        if s == 9:
            expect = (expect * np.float32(0.5)).astype(np.float32)
        assert np.array_equal(y[s], expect), s
        wrong = np.concatenate([np.zeros(1, np.float32), yt[s][:-1]]) * g
        assert not np.array_equal(y[s], (wrong * np.float32(0.5 if s == 9 else 1.0)).astype(np.float32)), "the test can tell the two orders apart"
    for s in (0, 1, 5, 8):
        assert np.array_equal(y[s], yt[s])


def test_all_three_stages_on_a_resampling_batch(na, models):
    """A 44.1 kHz resampling batch with a gate, an IR and a gain ramp on row 8 and a gate alone on row 0, in two different cuts: the
    same bits in every row; and row 0 is fl(twin_row * g_ref), g computed from the external-rate input rows the caller passed."""
    segments = [128, 441, 100, 300, 500]
    total = sum(segments)
    x = signal(total, 11)
    rng = np.random.default_rng(5)
    taps = (rng.standard_normal(40) * np.exp(-np.arange(40) / 8.0) * 0.3).astype(np.float32)
    p = G.params(floorGain=0.1)
    outs = []
    for cut in (lambda n: [n], H.ragged):
        calls = [n for seg in segments for n in cut(seg)]
        b = H.make_batch(na, models, stage=True, resample=44100)
        b.EnableCabinetStage(64)
        b.EnableGateStage()
        ir = b.LoadIR(taps)
        y, pos = [], 0
        for n in calls:
            if pos == segments[0]:
                b.SetStreamGate(8, p, True)
                b.SetStreamGate(0, p, True)
                b.SetStreamIR(8, ir, 0)
                b.SetStreamGain(8, 0.3, 300)
            y.append(b.Process(np.ascontiguousarray(x[:, pos:pos + n])))
            pos += n
        outs.append(np.concatenate(y, axis=1))
        b.close()
    assert np.array_equal(outs[0], outs[1]), np.flatnonzero(np.any(outs[0] != outs[1], axis=1))
    yt = _twin_rows(na, models, x, segments, resample=44100)
    g = G.GateRef(p, True).run(x[0, segments[0]:])
    assert np.any(g < 1.0)
    expect = yt[0].copy()
    expect[segments[0]:] = yt[0, segments[0]:] * g
    assert np.array_equal(outs[0][0], expect)
    assert np.array_equal(outs[0][4], yt[4]) and not np.array_equal(outs[0][8], yt[8])


# ================================================================================================ 8: in place

def test_in_place(na, models):
    """NA_BatchProcessDevice with dIn == dOut on gated streams: the detector has read the input before any model writes, so the bits
    are those of separate buffers."""
    import torch
    dev = torch.device("cuda", 0)
    calls = [128, 300, 129, 700]
    x = signal(sum(calls), 12)
    outs = {}
    for in_place in (False, True):
        b = G.make_batch(na, models, stage=True)
        for s, name in GATED.items():
            b.SetStreamGate(s, G.variation(name), True)
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
    assert np.array_equal(outs[True], outs[False])
    g = G.GateRef(G.variation("floor0"), True).run(x[0])
    assert np.any(g == 0.0) and not np.any(outs[True][0][g == 0.0]) and np.any(outs[True][0][g == 1.0])
