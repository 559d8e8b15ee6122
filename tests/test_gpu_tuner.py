"""GPU tests of the tuner stage (NA_BatchEnableTunerStage / NA_BatchSetStreamTuner / NA_BatchReadStreamTuner, csrc/tuner_stage.h,
DESIGN.md 2.15): a per-stream pitch reading of the input row -- the append launch that quantises, decimates and fills the rows' rings,
the evaluate launch that sums r[t] over the lags and selects one -- and the result path that brings the readings to the host without
a wait.

Everything goes through the C ABI.  The stage never writes an audio row, so every row is that of a twin batch without the stage, bit
for bit; everything behind the one float product per sample is an integer, so every reading equals the numpy restatement's
(tests/tuner_cases.py), field for field, after NA_BatchSynchronize."""
import os
import re

import numpy as np
import pytest

import handover_cases as H
import tuner_cases as T

FORCED = bool(os.environ.get("NA_WN_KERNEL") or os.environ.get("NA_WN_PACK") or os.environ.get("NA_WN_SPEC") or os.environ.get("NA_SP_T")
              or os.environ.get("NA_SP_GEN") or os.environ.get("NA_WN_PAD"))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(FORCED, reason="forced kernel family")]

PATHS = ("process", "registered", "submit", "device", "device-odd")
CALLS = [128, 17, 300, 128]
# packed nano, Standard, and both live LSTM rows: around one and two waves of lags, a hop below and above the call lengths
TUNED = {0: T.params(1, 100, 2, 63, 37, 0), 4: T.params(2, 32, 2, 4, 16, 15), 8: T.params(3, 100, 2, 64, 100, 7), 9: T.params(1, 257, 2, 130, 257, 256)}


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
    return capi.load_library().NA_DebugTunerLaunches


def signal(total, seed):
    """[ROWS, total]: every row a tone of its own period with a weak fundamental, and a little noise"""
    return np.stack([T.pitched(total, 23.7 + 3.4 * r, 300 + 20 * seed + r) for r in range(H.ROWS)])


def tuner_ops(at=0, rows=TUNED):
    return {at: [("tuner", s, p) for s, p in rows.items()]}


def expected_launches(refs, calls):
    """an append launch per call, an evaluate launch per call that holds an evaluation end of some tuner (calls of one piece)"""
    count = 0
    for i in range(len(calls)):
        ends = [(ref.ends[i - 1] if i else 0, ref.ends[i]) for ref in refs.values()]
        count += 1 + any(after > before for before, after in ends)
    return count


# ================================================================================================ 1: off is off

def test_off_is_off(na, models, launches):
    """The stage is enabled and no stream has a tuner: every path gives the twin's bits and launches none of the stage's kernels."""
    x = signal(sum(CALLS), 1)
    yt = np.concatenate(H.run_twin(na, models, x, CALLS, {}), axis=1)
    before = launches()
    for path in PATHS:
        b = T.make_batch(na, models)
        runner = H.Runner(na, b, path)
        try:
            y, _, _ = T.run_tuners(b, runner, x, CALLS, {})
        finally:
            runner.close()
            b.close()
        assert np.array_equal(y, yt), path
        assert np.any(y[0]) and np.any(y[4]) and np.any(y[8]) and not np.any(y[2])
    assert launches() == before


def test_off_is_off_for_the_half_batch_launches(na, models, launches):
    """512 A1 Standard streams on the batch's own stream, device pointers: with the stage enabled and no tuner the free-running mode
    engages as in the twin; one tuner orders the launches; taken away, the mode is back with the next call.  The bits are the twin's
    throughout, and the one call with an entry made two launches: it holds an evaluation end."""
    import torch
    dev = torch.device("cuda", 0)
    S, n, K = 512, 128, 5
    x = np.stack([T.pitched(K * n, 20.0 + r, 60 + r) for r in range(5)])[np.arange(S) % 5]
    dx = torch.from_numpy(x).to(dev)
    torch.cuda.synchronize(dev)
    halves, outs = {}, {}
    p = T.params(1, 64, 2, 40, 128, 0)
    for stage in (True, False):
        b = na.Batch(0)
        assert b.ReserveStreams(models[H.STD], S) == 0
        for s in range(S):
            b.ActivateStream(s, 1.0)
        if stage:
            b.EnableTunerStage()
        dy = torch.zeros(S, K * n, device=dev)
        before = launches()
        for k in range(K):
            if stage and k == 2:
                b.SetStreamTuner(7, p)
            if stage and k == 3:
                b.SetStreamTuner(7, None)
            b.ProcessDevice(dx.data_ptr() + 4 * k * n, dy.data_ptr() + 4 * k * n, n, K * n, K * n)
            b.Synchronize()
            halves[(stage, k)] = b.UsesHalfLaunches()
            if stage and k == 2:
                ref = T.TunerRef(p)
                ref.feed(x[7, 2 * n:3 * n])
                assert b.ReadStreamTuner(7) == ref.latest() and ref.evaluations == 1 and ref.latest()["lag"] > 0
        assert launches() - before == (2 if stage else 0), "an append and an evaluate launch in the call with an entry"
        outs[stage] = dy.cpu().numpy()
        b.close()
    for k in (0, 1, 3, 4):
        assert halves[(True, k)] == halves[(False, k)], k
    print("half-batch launches: twin %s, with a tuner %s, behind it %s" % (halves[(False, 1)], halves[(True, 2)], halves[(True, 3)]))
    assert not halves[(True, 2)]
    assert np.array_equal(outs[True], outs[False])


# ================================================================================================ 2: never the audio, always the restatement

@pytest.mark.parametrize("path", PATHS)
def test_a_tuner_on_one_stream_of_each_family(na, models, launches, path):
    """Tuners on rows 0 (packed nano), 4 (Standard), 8 and 9 (LSTM) in calls of [128, 17, 300, 128]: every row of every call is the
    twin's, and behind a synchronise every field of every reading is the restatement's.  One append launch per call and one evaluate
    launch per call that holds an evaluation end."""
    x = signal(sum(CALLS), 2)
    yt = np.concatenate(H.run_twin(na, models, x, CALLS, {}), axis=1)
    b = T.make_batch(na, models)
    runner = H.Runner(na, b, path)
    before = launches()
    try:
        y, refs, last = T.run_tuners(b, runner, x, CALLS, tuner_ops())
    finally:
        runner.close()
        b.close()
    assert np.array_equal(y, yt), "the stage writes no audio row"
    assert launches() - before == expected_launches(refs, CALLS)
    for s, p in TUNED.items():
        assert last[s]["evaluations"] == refs[s].evaluations > 0 and last[s]["decimation"] == p["decimation"]
    assert last[0]["lag"] > 0 and last[9]["lag"] > 0, "the condition on the inputs: a pitch is found"


_by_evaluation = {}


@pytest.mark.parametrize("cut", list(T.CUTS))
def test_the_cut_into_calls_never_shows(na, models, cut):
    """The 24 tuners of tuner_cases.cut_cases -- D 1, 2, 3, 8; (W, maxLag) (32, 4), (100, 63), (100, 64), (257, 65), (257, 130); H 16, 37,
    W; phase 0, H - 1 -- six at a time on the live rows, over one 1200-sample signal (rows 4 and 8 carry NaN, +-inf and samples at and
    past +-1) in calls of 1, 7, 63, 64, 65, 100, 128 and 333 samples and a ragged mix: after every call every reading is the
    restatement's, and evaluation k of a tuner has the same bits under every cut that computes it.  Calls of 1 and 7 are shorter than
    D = 8; with H = 16 a call of 333 holds several evaluation ends: `evaluations` counts them all, the reading is the last."""
    x = T.cut_signal()
    calls, cases = T.CUTS[cut], T.cut_cases()
    b = T.make_batch(na, models)
    runner = H.Runner(na, b, "process")
    try:
        for first in range(0, len(cases), len(H.LIVE)):
            group = dict(zip(H.LIVE, cases[first:first + len(H.LIVE)]))
            seen = {}
            pos = 0
            refs = {}
            for i, n in enumerate(calls):
                ops = tuner_ops(0, group) if i == 0 else {}
                _, refs, last = T.run_tuners(b, runner, x[:, pos:pos + n], [n], ops, refs=refs)
                for s, r in last.items():
                    if r is not None:
                        seen[(first, s, r["evaluations"])] = r
                pos += n
            for s, ref in refs.items():
                assert ref.position == T.TOTAL
                if cut == "333" and ref.p["hopSamples"] == 16:
                    assert last[s]["evaluations"] == ref.evaluations > len(ref.computed()) == 4
            for key, r in seen.items():
                assert _by_evaluation.setdefault(key, r) == r, (cut, key)
    finally:
        runner.close()
        b.close()


def test_saturation_nan_and_inf(na, models):
    """Rows 4 and 8 are nothing but the special inputs in turn -- NaN, +-inf, +-1e30, +-1, the neighbours of 1, -0.0, a subnormal, the
    samples around 1 / 32767 -- on top of a tone at a tenth of full scale: the readings are the restatement's (NaN reads 0, everything
    past +-1 reads +-32767) and the rows are the twin's, NaN for NaN."""
    total = 600
    x = signal(total, 3)
    for row in (4, 8):
        x[row] = np.float32(0.1) * x[row]
        x[row, ::2] = np.resize(T.SPECIAL, total // 2)
    assert np.array_equal(T.quantise(T.SPECIAL[:9]), [0, 32767, -32767, 32767, -32767, 32767, -32767, 32767, -32767])
    calls = [128, 172, 300]
    yt = np.concatenate(H.run_twin(na, models, x, calls, {}), axis=1)
    b = T.make_batch(na, models)
    runner = H.Runner(na, b, "process")
    try:
        y, refs, last = T.run_tuners(b, runner, x, calls, {0: [("tuner", 4, T.params(1, 100, 2, 64, 50, 0)), ("tuner", 8, T.params(2, 100, 2, 64, 50, 3))]})
    finally:
        runner.close()
        b.close()
    assert np.array_equal(y, yt, equal_nan=True)
    assert last[4]["evaluations"] == 12 and last[4]["e0"] > 20 * 32767 ** 2


def test_the_full_limit_case(na, models):
    """D 8, W 2048, maxLag 1024 on rows 4 and 9, a full-scale square of 8000 samples a period: 12296 bytes of ring values in LDS, 1026
    lags, sums next to 2^47 (e0 = 2048 * (8 * 32767)^2) -- in calls of 8192 samples and more, which the stage appends in pieces of 4096."""
    p = T.params(8, 2048, 2, 1024, 3100, 0, 922)
    total = 8 * 3100 + 5
    x = signal(total, 4)
    sq = np.where((np.arange(total) // 4000) % 2 == 0, np.float32(1.0), np.float32(-1.0)).astype(np.float32)
    x[4], x[9] = sq, -sq
    x[9, ::3] = np.inf
    calls = [8192, 8192, total - 16384]
    b = T.make_batch(na, models)
    runner = H.Runner(na, b, "process")
    try:
        _, refs, last = T.run_tuners(b, runner, x, calls, {0: [("tuner", 4, p), ("tuner", 9, p)]})
    finally:
        runner.close()
        b.close()
    assert last[4]["lag"] == 1000 and last[4]["e0"] == 2048 * (8 * 32767) ** 2 and last[4]["r"][1] == last[4]["e0"] and last[4]["e0"] > 1 << 46
    assert last[9]["evaluations"] == 1 and last[9]["position"] == 24800


def test_in_place(na, models):
    """NA_BatchProcessDevice with dIn == dOut on tuned streams: the stage has read the input before any model writes -- the readings
    are those of separate buffers (the restatement's), and so are the rows."""
    import torch
    dev = torch.device("cuda", 0)
    x = signal(sum(CALLS), 5)
    yt = np.concatenate(H.run_twin(na, models, x, CALLS, {}), axis=1)
    b = T.make_batch(na, models)
    refs = {}
    for s, p in TUNED.items():
        b.SetStreamTuner(s, p)
        refs[s] = T.TunerRef(p)
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
            ref.feed(x[s, pos:pos + n])
            assert b.ReadStreamTuner(s) == ref.latest(), (s, pos)
        pos += n
    assert all(ref.evaluations > 0 for ref in refs.values())
    b.close()


def test_on_a_resampling_batch_positions_count_external_samples(na, models):
    """A 44.1 kHz batch: the stage reads the external-rate rows the caller passed, and positions count the caller's samples."""
    x = signal(sum(CALLS), 6)
    b = T.make_batch(na, models, resample=44100)
    runner = H.Runner(na, b, "process")
    try:
        _, refs, last = T.run_tuners(b, runner, x, CALLS, tuner_ops())
    finally:
        runner.close()
        b.close()
    for s, p in TUNED.items():
        have = sum(CALLS) // p["decimation"]
        assert last[s]["evaluations"] == (have - p["phase"]) // p["hopSamples"] > 0
        assert last[s]["position"] == (p["phase"] + last[s]["evaluations"] * p["hopSamples"]) * p["decimation"]


# ================================================================================================ 3: the result path

def test_a_read_never_waits_and_says_which_evaluation_it_is(na, models):
    """ReadStreamTuner straight after ProcessDevice, no synchronise: whatever it returns is the restatement's reading for the
    evaluation it reports, never one ahead of the samples handed in; after a synchronise it is the newest."""
    import torch
    dev = torch.device("cuda", 0)
    calls = [64] * 12
    x = signal(sum(calls), 7)
    b = T.make_batch(na, models)
    p = T.params(1, 100, 2, 64, 48, 0)
    b.SetStreamTuner(4, p)
    ref = T.TunerRef(p)
    dx, dy = torch.from_numpy(x).to(dev), torch.zeros(H.ROWS, sum(calls), device=dev)
    torch.cuda.synchronize(dev)
    pos, arrived = 0, []
    for n in calls:
        b.ProcessDevice(dx.data_ptr() + 4 * pos, dy.data_ptr() + 4 * pos, n, sum(calls), sum(calls))
        ref.feed(x[4, pos:pos + n])
        r = b.ReadStreamTuner(4)
        if r is not None:
            assert 1 <= r["evaluations"] <= ref.evaluations and r == ref.reading(r["evaluations"] - 1), (pos, r)
            assert r["position"] <= pos + n
            arrived.append(r["evaluations"])
        pos += n
    b.Synchronize()
    assert b.ReadStreamTuner(4) == ref.latest() and ref.evaluations == 16
    assert arrived == sorted(arrived), "readings never go back"
    print("evaluations read without a wait, call by call:", arrived)
    b.close()


def test_nothing_from_before_a_restart_or_a_removal_is_read_again(na, models):
    """A restart inside a group of D and a hop: no reading until the new tuner's first evaluation ends, then that one's, made of the
    samples behind the restart alone -- also when the records of the earlier tuner are still on their way at the restart (no
    synchronise in front of it).  A removal makes Read return nothing; a tuner set again on the row starts from nothing."""
    x = signal(500, 8)
    b = T.make_batch(na, models)
    p = T.params(3, 32, 2, 20, 16, 5)  # the first evaluation ends with sample 63

    def call(lo, hi, sync=True):
        b.Process(np.ascontiguousarray(x[:, lo:hi]))
        if sync:
            b.Synchronize()

    def fresh(lo, hi):
        ref = T.TunerRef(p)
        ref.feed(x[4, lo:hi])
        return ref.latest()

    b.SetStreamTuner(4, p)
    call(0, 100)
    assert b.ReadStreamTuner(4) == fresh(0, 100) and fresh(0, 100)["evaluations"] == 1
    b.SetStreamTuner(4, p)  # position 100: one sample into a group of three
    assert b.ReadStreamTuner(4) is None and b.GetStreamTuner(4) == p
    call(100, 130)
    assert b.ReadStreamTuner(4) is None, "30 samples of the new tuner: no evaluation yet, and not the old tuner's"
    call(130, 170)
    assert b.ReadStreamTuner(4) == fresh(100, 170) and fresh(100, 170)["evaluations"] == 1
    # the device path leaves the records in flight: restart right behind the call
    import torch
    dev = torch.device("cuda", 0)
    dx = torch.from_numpy(np.ascontiguousarray(x[:, 170:270])).to(dev)
    dy = torch.zeros(H.ROWS, 100, device=dev)
    torch.cuda.synchronize(dev)
    b.ProcessDevice(dx.data_ptr(), dy.data_ptr(), 100, 100, 100)
    b.SetStreamTuner(4, p)
    assert b.ReadStreamTuner(4) is None
    call(270, 280)
    assert b.ReadStreamTuner(4) is None, "the earlier tuner's records have arrived by now and were dropped"
    call(280, 340)
    assert b.ReadStreamTuner(4) == fresh(270, 340) and fresh(270, 340)["evaluations"] == 1
    b.SetStreamTuner(4, None)
    assert b.ReadStreamTuner(4) is None and b.GetStreamTuner(4) is None and b.GetTunerInfo()["numTuners"] == 0
    b.SetStreamTuner(4, p)
    assert b.ReadStreamTuner(4) is None
    call(340, 500)
    assert b.ReadStreamTuner(4) == fresh(340, 500) and fresh(340, 500)["evaluations"] == 3
    b.close()


def test_rules(na, models):
    """Each refusal carries its text; every limit names its field; park, remove and the park that ends a hand-over drop the tuner;
    GetTunerInfo counts entries and bytes; save and load leave tuners alone; a broken batch refuses everything."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    b = H.make_batch(na, models, stage=True)  # (with the output stage, for the hand-over)
    p = T.params(1, 32, 2, 16, 32, 0)
    for call in (lambda: b.SetStreamTuner(0, p), lambda: b.SetStreamTuner(0, None), lambda: b.GetStreamTuner(0), lambda: b.ReadStreamTuner(0), lambda: b.GetTunerInfo()):
        with pytest.raises(na.NeuralAudioError, match=r"tuner stage not enabled \(NA_BatchEnableTunerStage\)"):
            call()
    assert lib.NA_BatchGetStreamTuner(b._h, 0, None) < 0 and lib.NA_BatchReadStreamTuner(b._h, 0, None) < 0
    b.EnableTunerStage()
    b.EnableTunerStage()
    info = b.GetTunerInfo()
    assert info["numTuners"] == 0 and info["deviceBytes"] >= 16 * (8 + 4 * 8192) + 4 * 16 * (72 + 88)
    with pytest.raises(na.NeuralAudioError, match="SetStreamTuner: stream 2 is parked"):
        b.SetStreamTuner(2, p)
    with pytest.raises(na.NeuralAudioError, match="SetStreamTuner: stream 12 is not a live stream of the batch"):
        b.SetStreamTuner(12, p)
    with pytest.raises(na.NeuralAudioError, match="GetStreamTuner: stream 12 is not a stream of the batch"):
        b.GetStreamTuner(12)
    with pytest.raises(na.NeuralAudioError, match="ReadStreamTuner: stream -1 is not a stream of the batch"):
        b.ReadStreamTuner(-1)
    for change, text in T.LIMITS:
        with pytest.raises(na.NeuralAudioError, match="SetStreamTuner: " + re.escape(text)):
            b.SetStreamTuner(0, T.params(**change))
    assert b.GetTunerInfo()["numTuners"] == 0 and b.GetStreamTuner(0) is None and b.ReadStreamTuner(0) is None
    b.SetStreamTuner(1, None)  # (no tuner: nothing to take away)
    for s in (0, 1, 4, 5, 8):
        b.SetStreamTuner(s, p)
    assert b.GetTunerInfo()["numTuners"] == 5 and b.GetStreamTuner(4) == p and b.GetTunerInfo()["deviceBytes"] == info["deviceBytes"]
    x = signal(64, 9)
    b.Process(x)
    b.Synchronize()
    assert b.ReadStreamTuner(0)["evaluations"] == 2
    b.ParkStream(0)
    assert b.GetTunerInfo()["numTuners"] == 4 and b.GetStreamTuner(0) is None and b.ReadStreamTuner(0) is None
    b.ActivateStream(0, 1.0)
    assert b.GetStreamTuner(0) is None and b.ReadStreamTuner(0) is None
    blob = b.SaveStreams([5])
    b.LoadStreams([4], blob)
    assert b.GetStreamTuner(4) == p and b.GetTunerInfo()["numTuners"] == 4
    b.Handover(4, 6, 1.0, 64)
    b.Process(x)
    assert b.GetStreamTuner(4) is not None and b.GetStreamTuner(6) is None
    b.Process(x)  # (parks row 4 in front of its launches)
    assert b.IsParked(4) and b.GetStreamTuner(4) is None and b.GetTunerInfo()["numTuners"] == 3
    # the stage grows with the batch, and the rows that exist keep what they hold
    first = b.ReserveStreams(models[H.LSTM], 30)
    b.ActivateStream(first + 29, 1.0)
    b.SetStreamTuner(first + 29, p)
    assert b.GetTunerInfo()["deviceBytes"] > info["deviceBytes"]
    b.Process(signal(64, 10)[np.arange(b.NumStreams()) % H.ROWS])
    b.Synchronize()
    assert b.ReadStreamTuner(first + 29)["evaluations"] == 2 and b.GetStreamTuner(1) is not None and b.ReadStreamTuner(1)["evaluations"] == 8
    # a broken batch refuses everything
    b.SetWaitLimitMs(20.0)
    b.DebugStallDevice(80.0)
    with pytest.raises(na.NeuralAudioError, match="did not answer within"):
        b.Synchronize()
    assert b.IsBroken()
    for call in (lambda: b.SetStreamTuner(1, p), lambda: b.SetStreamTuner(1, None), lambda: b.ReadStreamTuner(1), lambda: b.EnableTunerStage()):
        with pytest.raises(na.NeuralAudioError, match="broken"):
            call()
    assert lib.NA_BatchReadStreamTuner(b._h, 1, None) < 0
    b.close()


def test_remove_streams_drops_the_tuner(na, models):
    b = na.Batch(0)
    assert b.AddStreams(models[H.LSTM], 4) == 0
    b.EnableTunerStage()
    b.SetStreamTuner(1, T.params())
    b.SetStreamTuner(2, T.params())
    b.RemoveStreams(1, 1)
    assert b.GetTunerInfo()["numTuners"] == 1
    assert b.AddStreams(models[H.LSTM], 1) == 1 and b.GetStreamTuner(1) is None and b.GetStreamTuner(2) is not None
    b.close()


def test_set_read_and_processing_calls_are_real_time_safe(na, models, launches):
    """NA_DebugDeviceResourceCalls stays where it is across set, restart, remove and read calls and 21 processing calls with entries,
    over the blocking and the pipelined host path and device pointers (after three warm calls of each, which size the staging block
    and the pipeline slots); NA_DebugTunerLaunches moves by two per call: every tuner here has a hop of at most 128 samples."""
    import torch
    from neuralaudio_amd import capi
    lib = capi.load_library()
    dev = torch.device("cuda", 0)
    b = T.make_batch(na, models)
    n = 128
    x = signal(n, 11)
    dx, dy = torch.from_numpy(x).to(dev), torch.zeros(H.ROWS, n, device=dev)
    torch.cuda.synchronize(dev)

    def three():
        b.Process(x)
        b.ReadStreamTuner(0)
        b.Collect(b.Submit(x))
        b.ReadStreamTuner(0)
        b.ProcessDevice(dx.data_ptr(), dy.data_ptr(), n, n, n)
        b.ReadStreamTuner(0)
        b.Synchronize()

    b.SetStreamTuner(0, T.params(1, 100, 2, 64, 128, 0))
    for _ in range(3):
        three()
    before, count = lib.NA_DebugDeviceResourceCalls(), launches()
    b.SetStreamTuner(4, T.params(2, 32, 2, 16, 16, 0))
    b.SetStreamTuner(8, T.params(8, 257, 2, 130, 16, 3))
    for i in range(7):
        three()
        if i == 2:
            b.SetStreamTuner(0, T.params(1, 64, 2, 32, 64, 0))
            b.SetStreamTuner(8, None)
        if i == 4:
            b.SetStreamTuner(9, T.params(1, 2048, 2, 1024, 65536, 0))
            b.SetStreamTuner(4, None)
    assert b.GetStreamTuner(8) is None and b.GetTunerInfo()["numTuners"] == 2 and b.ReadStreamTuner(0)["evaluations"] == 24
    assert lib.NA_DebugDeviceResourceCalls() == before
    assert launches() - count == 2 * 21
    b.SetStreamTuner(0, None)
    b.SetStreamTuner(9, None)
    three()
    assert launches() - count == 2 * 21, "no entry: no launch"
    b.close()


def test_every_entry_gets_its_own_reading(na, models, launches):
    """70 BossLSTM-2x8 streams, every one with a tuner of its own hop and phase on a tone of its own period: more entries than a wave
    has lanes; the evaluate launch runs over a strict subset of the entries (counted from the restatement); every entry's reading is
    its own restatement's, and the rows are those of a batch without the stage."""
    S = 70
    calls = [130, 129, 20, 131, 140]
    x = np.stack([T.pitched(sum(calls), 17.0 + 0.9 * r, 4000 + r, level=0.1 + 0.01 * (r % 50)) for r in range(S)])
    batches = {}
    for stage in (False, True):
        b = na.Batch(0)
        assert b.AddStreams(models[H.LSTM], S) == 0
        if stage:
            b.EnableTunerStage()
        batches[stage] = b
    runner, twin = H.Runner(na, batches[True], "device-odd"), batches[False]
    try:
        ops = {0: [("tuner", r, T.params(1 + r % 3, 100 + r, 2, 60 + r, 40 + r, (7 * r) % 40)) for r in range(S)]}
        before = launches()
        y, refs, last = T.run_tuners(batches[True], runner, x, calls, ops)
        assert launches() - before == expected_launches(refs, calls)
        assert batches[True].GetTunerInfo()["numTuners"] == S
        pos = 0
        for n in calls:
            assert np.array_equal(y[:, pos:pos + n], twin.Process(np.ascontiguousarray(x[:, pos:pos + n])))
            pos += n
        per_call = [sum((ref.ends[i - 1] if i else 0) < ref.ends[i] for ref in refs.values()) for i in range(len(calls))]
        print("entries with an evaluation end, call by call:", per_call)
        assert all(0 < per_call[i] < S for i in (0, 1, 3, 4))
        assert all(r is not None for r in last.values()) and len({(r["lag"], r["e0"]) for r in last.values()}) == S
        assert sum(r["lag"] > 0 for r in last.values()) > S // 2
    finally:
        runner.close()
        for b in batches.values():
            b.close()
