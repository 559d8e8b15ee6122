"""GPU tests of the mix stage (NA_BatchEnableMixStage / NA_BatchSetMixGroup, csrc/mix_stage.h): per-session mix groups
behind the output stage and in front of the meter's OUT tap -- the one stage in which rows meet.

Everything goes through the C ABI.  The contract is bit-exact: every comparison is np.array_equal (of bit patterns where NaN and -0
matter) against MixRef, the numpy float32 restatement (tests/mix_cases.py).  Model cases apply MixRef to the rows of a twin batch
without the stage, as tests/test_gpu_gate.py does; arithmetic cases go through NA_DebugRunMixStage on given rows."""
import os
import re

import numpy as np
import pytest

import eq_cases as E
import gate_cases as G
import handover_cases as H
import meter_cases as MT
import mix_cases as M

FORCED = bool(os.environ.get("NA_WN_KERNEL") or os.environ.get("NA_WN_PACK") or os.environ.get("NA_WN_SPEC") or os.environ.get("NA_SP_T")
              or os.environ.get("NA_SP_GEN") or os.environ.get("NA_WN_PAD"))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(FORCED, reason="forced kernel family")]

F = np.float32
OUT, DRY = M.OUT, M.DRY


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
def lib():
    from neuralaudio_amd import capi
    return capi.load_library()


@pytest.fixture(scope="module")
def launches(lib):
    return lambda: (int(lib.NA_DebugMixLaunches()), int(lib.NA_DebugMixStashLaunches()))


def run_calls(na, b, x, calls, path="process", ops=None):
    """the batch through `path`, call by call; ops[i](b) runs in front of call i.  Returns the rows of every call."""
    runner, out, pos = H.Runner(na, b, path), [], 0
    try:
        for i, n in enumerate(calls):
            if ops and i in ops:
                ops[i](b)
            out.append(runner.call(x[:, pos:pos + n]))
            pos += n
    finally:
        runner.close()
    return out


_twins = {}


def twin_rows(na, models, x, calls, key):
    """the rows of the batch without the mix stage, call by call (kept per key: a reference is computed once)"""
    if key not in _twins:
        b = M.make_batch(na, models, mix=False)
        _twins[key] = run_calls(na, b, x, calls)
        b.close()
    return _twins[key]


def rand(shape, seed, scale=1.0):
    return (scale * np.random.default_rng(seed).standard_normal(shape)).astype(F)


# ================================================================================================ 1: off is off

def test_off_is_off(na, models, launches):
    """The stage is enabled and there is no group: process, submit / collect and device pointers give the twin's bits and none of the
    stage's kernels is launched."""
    calls = [128, 17, 300]
    x = H.signal(sum(calls), 31)
    yt = np.concatenate(twin_rows(na, models, x, calls, "off"), axis=1)
    before = launches()
    for path in ("process", "submit", "device", "device-odd"):
        b = M.make_batch(na, models, mix=True)
        y = np.concatenate(run_calls(na, b, x, calls, path), axis=1)
        info = b.GetMixInfo()
        assert (info["maxMembers"], info["numGroups"], info["drySamples"]) == (8, 0, 2048) and info["deviceBytes"] > 16 * (2048 + 128) * 4
        b.close()
        assert np.array_equal(y, yt), path
        assert np.any(y[0]) and np.any(y[4]) and np.any(y[8]) and not np.any(y[2])
    assert launches() == before


def test_off_is_off_for_the_half_batch_launches(na, models, launches):
    """512 A1 Standard streams on the batch's own stream, device pointers: with the stage enabled and no group the free-running mode
    engages as in the twin and the bits are the twin's; a group orders the launches; cleared, the mode comes back."""
    import torch
    dev = torch.device("cuda", 0)
    S, n, K = 512, 128, 5
    x = np.stack([H.noise(K * n, 70 + r) for r in range(5)])[np.arange(S) % 5]
    dx = torch.from_numpy(x).to(dev)
    torch.cuda.synchronize(dev)
    halves, outs = {}, {}
    gains = np.array([[0.5, -0.25], [0.75, 1.5]], F)
    for stage in (True, False):
        b = na.Batch(0)
        assert b.ReserveStreams(models[H.STD], S) == 0
        for s in range(S):
            b.ActivateStream(s, 1.0)
        if stage:
            b.EnableMixStage()
        dy = torch.zeros(S, K * n, device=dev)
        before = launches()
        for k in range(K):
            if stage and k == 2:
                b.SetMixGroup([7, 300], gains)
            if stage and k == 3:
                b.ClearMixGroup(300)
            b.ProcessDevice(dx.data_ptr() + 4 * k * n, dy.data_ptr() + 4 * k * n, n, K * n, K * n)
            b.Synchronize()
            halves[(stage, k)] = b.UsesHalfLaunches()
        assert launches() == ((before[0] + 1, before[1]) if stage else before), "one launch per call with a group"
        outs[stage] = dy.cpu().numpy()
        b.close()
    for k in (0, 1, 4):
        assert halves[(True, k)] == halves[(False, k)], k
    print("half-batch launches: twin %s, with a group %s, in the call behind the clear %s, behind it %s" % (halves[(False, 1)], halves[(True, 2)], halves[(True, 3)], halves[(True, 4)]))
    assert not halves[(True, 2)]
    expect = outs[False].copy()
    expect[:, 2 * n:3 * n] = M.MixRef([7, 300], gains).run(outs[False][:, 2 * n:3 * n])
    assert np.array_equal(outs[True], expect)


# ================================================================================================ 2: shapes, through the debug hook

SHAPES = {  # (M, D): the members' rows -- descending and interleaved orders: an output is then read as a source of a later output
    (1, 1): [6], (2, 1): [7, 1], (2, 2): [5, 2], (3, 2): [9, 0, 4], (8, 1): [12, 23, 10, 21, 14, 19, 16, 17], (8, 8): [22, 20, 18, 15, 13, 11, 8, 3]}
SHAPE_ROWS = 24
NS = (1, 3, 4, 5, 255, 256, 257, 1000)


def _shape_refs(seed, integer=False):
    rng = np.random.default_rng(seed)
    refs = []
    for (Mm, D), rows in SHAPES.items():
        g = rng.integers(-3, 4, (D, Mm)).astype(F) if integer else rng.standard_normal((D, Mm)).astype(F) * F(1.5)  # (mixed sign)
        if not integer and Mm > 1:
            g[0, 1] = 0.0  # (a member that is skipped in one output)
        refs.append(M.MixRef(rows, g, D))
    return refs


@pytest.fixture(scope="module")
def shape_batch(na, models):
    assert sorted(r for rows in SHAPES.values() for r in rows) == list(range(SHAPE_ROWS))
    b = M.lstm_batch(na, models, SHAPE_ROWS)
    for ref in _shape_refs(40):
        b.SetMixGroup(ref.streams, ref.g1)
    yield b
    b.close()


@pytest.mark.parametrize("n", NS)
def test_shapes_and_both_paths(shape_batch, launches, n):
    """Six groups at once -- (M, D) in (1,1) (2,1) (2,2) (3,2) (8,1) (8,8), gains of mixed sign -- on rows of n samples: stride n and
    n + 1, and a stride that is a multiple of 4 and one that is not (the float4 and the scalar path, whatever n is): every row equals
    the restatement, so the paths equal each other; the rows of no group's outputs and the padding are untouched."""
    rows = rand((SHAPE_ROWS, n), 41 + n)
    expect = M.run_groups(_shape_refs(40), rows)
    assert not np.array_equal(expect, rows)
    vec = (n + 3) // 4 * 4
    for stride in sorted({n, n + 1, vec, vec + 1}):
        before = launches()
        got = M.debug_run(shape_batch, rows, n, stride)
        assert launches() == (before[0] + 1, before[1]), "one launch over every group, no stash launch"
        assert M.same_bits(got, expect), (n, stride, int(np.count_nonzero(M.bits(got) != M.bits(expect))))


def test_integer_known_answer(na, models):
    """Integer-valued gains and samples: every product and sum is exact, so the outputs are the integer matrix products -- computed here
    in int64, without the restatement."""
    b = M.lstm_batch(na, models, SHAPE_ROWS)
    refs = _shape_refs(42, integer=True)
    for ref in refs:
        b.SetMixGroup(ref.streams, ref.g1)
    n = 261
    rows = np.random.default_rng(43).integers(-100, 101, (SHAPE_ROWS, n)).astype(F)
    expect = rows.astype(np.int64)
    for ref in refs:
        expect[ref.streams[:ref.D]] = ref.g1.astype(np.int64) @ rows[ref.streams].astype(np.int64)
    for stride in (n + 3, n + 4):
        got = M.debug_run(b, rows, n, stride)
        assert np.array_equal(got.astype(np.int64), expect) and np.all(got == np.round(got))
    assert M.same_bits(M.run_groups(refs, rows), M.debug_run(b, rows, n, n))
    b.close()


# ================================================================================================ 3: identity and zero

def test_identity_passes_bits_and_a_zero_gain_keeps_nan_out(na, models):
    rows = rand((6, 300), 44)
    rows[1, :7] = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-42, -3e-45], F)
    rows[3, :] = np.nan
    rows[4, 5] = np.inf
    b = M.lstm_batch(na, models, 6)
    b.SetMixGroup([1, 0], np.eye(2, dtype=F))
    b.SetMixGroup([2, 3, 4], [[1.0, 0.0, 0.0]], numOutputs=1)  # a NaN row and an Inf at gain 0
    for stride in (300, 301):
        assert M.same_bits(M.debug_run(b, rows, 300, stride), rows), "the identity passes its rows bit for bit"
    b.SetMixGroup([2, 3, 4], [[0.5, 0.0, -0.0]], numOutputs=1)
    got = M.debug_run(b, rows, 300, 300)
    assert np.all(np.isfinite(got[2])) and np.array_equal(got[2], rows[2] * F(0.5)) and M.same_bits(got[3:], rows[3:])
    b.SetMixGroup([2, 3, 4], [[0.0, 0.0, 0.0]], numOutputs=1)
    got = M.debug_run(b, rows, 300, 301)
    assert not np.any(M.bits(got[2])), "no member: +0.0"
    b.SetMixGroup([2, 3, 4], [[0.0, 1.0, 0.0]], numOutputs=1)
    assert np.all(np.isnan(M.debug_run(b, rows, 300, 300)[2])), "rows are not sanitised"
    b.close()


# ================================================================================================ 4: ramps

@pytest.mark.parametrize("R", [1, 2, 7, 128, 1000])
def test_ramps_do_not_depend_on_the_cut(na, models, R):
    """A new group ramps from the identity over R samples, then a gain change over R more: calls cut ragged against one call per
    stretch give the same bits, and both the restatement's."""
    total = 1100
    rows = rand((4, 2 * total), 45 + R)
    g1 = np.array([[0.3, -1.2, 0.0], [2.0, 0.4, -0.6]], F)
    g2 = np.array([[-0.8, 0.0, 1.1], [0.0, 0.0, 0.25]], F)
    ref = M.MixRef([3, 0, 2], g1, R=R)
    first = ref.gains(1)[0]
    want = (np.eye(2, 3, dtype=F) + (g1 - np.eye(2, 3, dtype=F)) * F(np.float64(1) / np.float64(R))) if R > 1 else g1
    assert np.array_equal(first, want), "a new group with R > 0 starts from the identity"
    expect = ref.run(rows[:, :total])
    ref.set(g2, R)
    expect = np.concatenate([expect, ref.run(rows[:, total:])], axis=1)
    b = M.lstm_batch(na, models, 4)
    outs = []
    for cuts in ([total], H.ragged(total)):
        b.ClearMixGroup(0)
        got, pos = [], 0
        for g in (g1, g2):
            b.SetMixGroup([3, 0, 2], g, rampSamples=R)
            assert b.MixRampRemaining(2) == R
            for n in cuts:
                got.append(M.debug_run(b, rows[:, pos:pos + n], n, n + (pos % 2)))
                pos += n
            assert b.MixRampRemaining(3) == 0
        outs.append(np.concatenate(got, axis=1))
    b.close()
    assert M.same_bits(outs[0], expect) and M.same_bits(outs[1], expect)


def test_a_set_call_in_the_middle_of_a_ramp_starts_from_the_reached_gains(na, models):
    """A ramp of 400, re-targeted after 150 samples (a ragged cut) with a ramp of 256: the rows equal the restatement, whose gain
    sequence has no step larger than one ramp increment (+ 4 ulp: three roundings per gain)."""
    rows = rand((3, 700), 50)
    ga, gb = np.array([[0.2, 1.5]], F), np.array([[-1.0, 0.5]], F)
    ref = M.MixRef([1, 2], ga, D=1, R=400)
    seq = [ref.reached()[None], ref.gains(150)]
    expect = ref.run(rows[:, :150])
    ref.set(gb, 256)
    seq.append(ref.gains(550))
    expect = np.concatenate([expect, ref.run(rows[:, 150:])], axis=1)
    seq = np.concatenate(seq)[:, 0, :].astype(np.float64)
    step = np.max(np.abs(np.diff(seq, axis=0)), axis=0)
    limit = np.maximum(np.abs(ga[0] - np.eye(1, 2)[0]) / 400, np.abs(gb[0].astype(np.float64) - seq[150]) / 256) + 4 * np.spacing(F(1.5))
    assert np.all(step <= limit), (step, limit)
    b = M.lstm_batch(na, models, 3)
    b.SetMixGroup([1, 2], ga, numOutputs=1, rampSamples=400)
    got = [M.debug_run(b, rows[:, :133], 133, 133), M.debug_run(b, rows[:, 133:150], 17, 20)]
    assert b.MixRampRemaining(1) == 250
    b.SetMixGroup([1, 2], gb, numOutputs=1, rampSamples=256)
    got += [M.debug_run(b, rows[:, 150:405], 255, 256), M.debug_run(b, rows[:, 405:], 295, 295)]
    assert M.same_bits(np.concatenate(got, axis=1), expect)
    assert np.array_equal(b.GetStreamMix(2)["gains"], gb.reshape(1, 2)) and b.MixRampRemaining(2) == 0
    b.close()


# ================================================================================================ 5: more groups than a wave's worth

def test_70_groups_in_one_launch(na, models, launches):
    """140 BossLSTM-2x8 streams, 70 groups of two with distinct gains, independent inputs: every row equals the restatement on the
    rows of the same batch without groups, and every call is ONE launch."""
    S, calls = 140, [64, 129]
    x = np.stack([H.noise(sum(calls), 500 + r) for r in range(S)])
    refs = [M.MixRef([2 * g + 1, 2 * g] if g % 2 else [2 * g, 2 * g + 1], rand((2, 2), 600 + g), R=100) for g in range(70)]
    outs = {}
    for mix in (False, True):
        b = M.lstm_batch(na, models, S, mix)
        if mix:
            for ref in refs:
                b.SetMixGroup(ref.streams, ref.g1, rampSamples=100)
            assert b.GetMixInfo()["numGroups"] == 70
        before = launches()
        outs[mix] = [b.Process(np.ascontiguousarray(x[:, :64])), b.Process(np.ascontiguousarray(x[:, 64:]))]
        assert launches() == ((before[0] + 2, before[1]) if mix else before)
        b.close()
    for i in range(2):
        assert np.array_equal(outs[True][i], M.run_groups(refs, outs[False][i])), i


# ================================================================================================ 6: the DRY tap

def _wet_dry_refs(R=0):
    return [M.MixRef([s, s], [[0.7, g]], D=1, taps=[OUT, DRY], R=R) for s, g in ((0, 0.5), (4, -0.25), (8, 1.25))]


def test_wet_dry_on_each_family(na, models, launches):
    """Row s OUT plus row s DRY, D = 1, on the packed nano, the Standard and the LSTM family: the rows equal the restatement on the
    twin's rows and the call's input; a call of 2049 grows the stash block (drySamples 2048 -> 4096) and stays exact; every call
    launches the stash kernel once and the mix kernel once."""
    calls = [128, 17, 2049, 300]
    x = H.signal(sum(calls), 32)
    yt = twin_rows(na, models, x, calls, "dry")
    b = M.make_batch(na, models, mix=True)
    refs = _wet_dry_refs(R=200)
    for ref in refs:
        b.SetMixGroup(ref.streams, ref.g1, numOutputs=1, taps=ref.taps, rampSamples=200)
    info = []
    before = launches()
    y = run_calls(na, b, x, calls, "process", ops={i: (lambda b: info.append(b.GetMixInfo())) for i in range(4)})
    info.append(b.GetMixInfo())
    assert launches() == (before[0] + 4, before[1] + 4)
    assert [i["drySamples"] for i in info] == [2048, 2048, 2048, 4096, 4096] and info[3]["deviceBytes"] > info[2]["deviceBytes"] and info[0]["numGroups"] == 3
    b.close()
    pos = 0
    for i, n in enumerate(calls):
        assert np.array_equal(y[i], M.run_groups(refs, yt[i], x[:, pos:pos + n])), i
        pos += n


def test_wet_dry_in_place(na, models):
    """NA_BatchProcessDevice with dIn == dOut: the stash kernel has kept the input rows of the DRY members before any model writes, so
    the bits are those of separate buffers (and the restatement's)."""
    import torch
    dev = torch.device("cuda", 0)
    calls = [128, 129, 300]
    x = H.signal(sum(calls), 33)
    yt = twin_rows(na, models, x, calls, "in-place")
    refs = _wet_dry_refs()
    b = M.make_batch(na, models, mix=True)
    for ref in refs:
        b.SetMixGroup(ref.streams, ref.g1, numOutputs=1, taps=ref.taps)
    pos = 0
    for i, n in enumerate(calls):
        buf = torch.from_numpy(np.ascontiguousarray(x[:, pos:pos + n])).to(dev)
        torch.cuda.synchronize(dev)
        b.ProcessDevice(buf.data_ptr(), buf.data_ptr(), n, n, n)
        b.Synchronize()
        rows = buf.cpu().numpy()
        rows[list(set(range(H.ROWS)) - set(H.LIVE))] = 0.0  # (device rows of parked streams are left alone: here, the input)
        assert np.array_equal(rows, M.run_groups(refs, yt[i], x[:, pos:pos + n])), i
        pos += n
    b.close()


def test_the_stash_kernel_runs_only_for_a_dry_member(na, models, launches):
    """Through the debug hook: a group of OUT taps launches no stash kernel (hostIn may be NULL); beside a group with a DRY member
    it launches once per call, and without hostIn the call is refused."""
    from neuralaudio_amd import capi
    rows, x = rand((5, 100), 51), rand((5, 100), 52)
    b = M.lstm_batch(na, models, 5)
    a = M.MixRef([0, 1], [[0.5, 0.5], [1.0, -1.0]])
    d = M.MixRef([3, 2, 3, 4], [[1.0, 0.5, -0.5, 0.25]], D=1, taps=[OUT, OUT, DRY, DRY])
    b.SetMixGroup(a.streams, a.g1)
    before = launches()
    assert M.same_bits(M.debug_run(b, rows, 100, 100), a.run(rows)) and launches() == (before[0] + 1, before[1])
    b.SetMixGroup(d.streams, d.g1, numOutputs=1, taps=d.taps)
    for stride in (100, 101):
        assert M.same_bits(M.debug_run(b, rows, 100, stride, x), M.run_groups([a, d], rows, x))
    assert launches() == (before[0] + 3, before[1] + 2)
    assert capi.load_library().NA_DebugRunMixStage(b._h, None, M.fp(rows.copy()), 100, 100) != 0 and "hostIn" in capi.last_error()
    b.ClearMixGroup(4)
    assert M.same_bits(M.debug_run(b, rows, 100, 100), a.run(rows)) and launches() == (before[0] + 4, before[1] + 2)
    b.close()


# ================================================================================================ 7: with the other stages

def test_the_mix_sees_the_chain_and_the_meter_sees_the_mix(na, models):
    """Row 4 carries a gate, a 3-section EQ, the IR {1, 0.5} and an output gain of 0.5; the group {4, 8} (stereo) mixes that row with
    row 8.  The rows equal the restatement on the rows of a batch with the same stages and no group -- the mix sits behind the whole
    chain -- and the OUT tap of a meter on row 4 reports the peak of the MIXED row."""
    calls = [128, 129, 300]
    x = np.stack([G.gate_signal(700 + r, sum(calls)) for r in range(H.ROWS)])
    gains = np.array([[0.6, -0.9], [0.3, 1.2]], F)
    outs, readings = {}, []
    for mix in (False, True):
        b = M.make_batch(na, models, mix=mix)
        b.EnableCabinetStage(64)
        b.EnableGateStage()
        b.EnableEqStage()
        b.EnableMeterStage()
        b.SetStreamGate(4, G.params(floorGain=0.1), True)
        b.SetStreamEq(4, E.cascade(3, 80), 0)
        b.SetStreamIR(4, b.LoadIR(np.array([1.0, 0.5], F)), 0)
        b.SetStreamGain(4, 0.5, 0)
        if mix:
            b.SetMixGroup([4, 8], gains, rampSamples=64)
        out, pos = [], 0
        for n in calls:
            if mix:
                b.SetStreamMeter(4, MT.params(window=n, clip_out=0.5))  # (restarts at position 0: one window per call)
            out.append(b.Process(np.ascontiguousarray(x[:, pos:pos + n])))
            pos += n
            if mix:
                b.Synchronize()
                readings.append(b.ReadStreamMeter(4))
        outs[mix] = out
        b.close()
    ref = M.MixRef([4, 8], gains, R=64)
    assert np.any(outs[False][0][4] != 0)
    for i in range(len(calls)):
        expect = ref.run(outs[False][i])
        assert np.array_equal(outs[True][i], expect), i
        assert readings[i] is not None and MT.bits(readings[i]["out"]["peak"]) == MT.bits(np.max(np.abs(expect[4]))), i
        assert MT.bits(np.max(np.abs(expect[4]))) != MT.bits(np.max(np.abs(outs[False][i][4])))


# ================================================================================================ 8: the hand-over recipe

def test_the_hand_over_recipe(na, models):
    """A dual-amp group {4, 8}.  Handover 4 -> 6 with a fade of 300 and, in front of the same call, clear + set {6, 8} at the same
    gains with rampSamples = 0: the rows equal the restatement applied to the rows of a batch that did the same hand-over without a
    group, through the fade and after the park, and the group survives the park of row 4."""
    calls = [128, 128, 129, 128, 64]
    x = H.signal(sum(calls), 34, same=[(4, 6)])
    gains = np.array([[0.8, -0.5]], F)
    outs, seen = {}, []
    for mix in (False, True):
        b = M.make_batch(na, models, mix=mix)
        if mix:
            b.SetMixGroup([4, 8], gains, numOutputs=1, rampSamples=100)

        def hand(b, mix=mix):
            b.Handover(4, 6, 1.0, 300)
            if mix:
                b.ClearMixGroup(4)
                b.SetMixGroup([6, 8], gains, numOutputs=1, rampSamples=0)

        outs[mix] = run_calls(na, b, x, calls, "process", ops={1: hand})
        seen.append((b.IsParked(4), b.HandoverRemaining(6)))
        if mix:
            got = b.GetStreamMix(8)
            assert got["streams"] == [6, 8] and got["numOutputs"] == 1 and b.GetStreamMix(4) is None and b.GetMixInfo()["numGroups"] == 1
        b.close()
    assert seen == [(True, 0), (True, 0)], "the fade is over and row 4 parked before the last call"
    first, second = M.MixRef([4, 8], gains, D=1, R=100), M.MixRef([6, 8], gains, D=1)
    for i in range(len(calls)):
        expect = first.run(outs[False][i]) if i == 0 else second.run(outs[False][i])
        assert np.array_equal(outs[True][i], expect), i
    assert np.any(outs[True][4][6]) and not np.any(outs[True][4][4])


# ================================================================================================ 9: rules

def test_rules_by_message(na, models, lib):
    from neuralaudio_amd import capi
    b = M.make_batch(na, models, mix=False)
    eye = np.eye(2, dtype=F)
    for call in (lambda: b.SetMixGroup([0, 1], eye), lambda: b.ClearMixGroup(0), lambda: b.GetStreamMix(0), lambda: b.MixRampRemaining(0), lambda: b.GetMixInfo()):
        with pytest.raises(na.NeuralAudioError, match=re.escape(M.NOT_ENABLED)):
            call()
    b.EnableMixStage()
    b.EnableMixStage()
    assert b.GetMixInfo()["numGroups"] == 0 and b.GetStreamMix(0) is None and b.MixRampRemaining(0) == 0
    b.ClearMixGroup(0)  # (no group: not an error)
    nine = list(H.LIVE) + [0, 1, 4]
    cases = [
        (lambda: b.SetMixGroup([0, 2], eye), "SetMixGroup: stream 2 is parked"),
        (lambda: b.SetMixGroup([0, 12], eye), "SetMixGroup: stream 12 is not a live stream of the batch"),
        (lambda: b.SetMixGroup([-1, 0], eye), "SetMixGroup: stream -1 is not a live stream of the batch"),
        (lambda: lib.NA_BatchSetMixGroup(b._h, (M.C.c_int * 9)(*nine), None, 9, 1, (M.C.c_float * 9)(), 0) and _raise(na), r"numMembers must lie in \[1, 8\]"),
        (lambda: lib.NA_BatchSetMixGroup(b._h, (M.C.c_int * 1)(0), None, 0, 1, (M.C.c_float * 1)(), 0) and _raise(na), r"numMembers must lie in \[1, 8\]"),
        (lambda: b.SetMixGroup([0, 1], np.zeros(6, F), numOutputs=3), r"numOutputs must lie in \[1, numMembers\]"),
        (lambda: b.SetMixGroup([0, 1], np.zeros(0, F), numOutputs=0), r"numOutputs must lie in \[1, numMembers\]"),
        (lambda: b.SetMixGroup([0, 1], eye, taps=[OUT, DRY]), "the outputs must be OUT taps of distinct streams"),
        (lambda: b.SetMixGroup([0, 0], eye), "the outputs must be OUT taps of distinct streams"),
        (lambda: b.SetMixGroup([0, 1, 1], [[1, 0, 0]], numOutputs=1), "duplicate member: stream 1 appears twice in the same tap"),
        (lambda: b.SetMixGroup([0, 1, 1], [[1, 0, 0]], numOutputs=1, taps=[OUT, DRY, DRY]), "duplicate member: stream 1 appears twice in the same tap"),
        (lambda: b.SetMixGroup([0, 1], [[1, 0]], numOutputs=1, taps=[OUT, 2]), "a tap must be NA_MIX_TAP_OUT or NA_MIX_TAP_DRY"),
        (lambda: b.SetMixGroup([0, 1], [[1.0, float("nan")], [0, 1]]), "every gain must be finite"),
        (lambda: b.SetMixGroup([0, 1], [[1.0, 0], [float("-inf"), 1]]), "every gain must be finite"),
        (lambda: b.SetMixGroup([0, 1], eye, rampSamples=-1), r"SetMixGroup: rampSamples must lie in \[0, 1 << 20\]"),
        (lambda: b.SetMixGroup([0, 1], eye, rampSamples=(1 << 20) + 1), r"SetMixGroup: rampSamples must lie in \[0, 1 << 20\]"),
        (lambda: b.GetStreamMix(12), "GetStreamMix: stream 12 is not a stream of the batch"),
        (lambda: b.MixRampRemaining(-1), "MixRampRemaining: stream -1 is not a stream of the batch"),
        (lambda: b.ClearMixGroup(12), "ClearMixGroup: stream 12 is not a stream of the batch"),
    ]
    for call, text in cases:
        with pytest.raises(na.NeuralAudioError, match=text):
            call()
    assert b.GetMixInfo()["numGroups"] == 0
    # one group per stream; the exact member list is a gain change; anything else names the stream that is taken
    b.SetMixGroup([0, 1, 0], [[1, 0, 0.5], [0, 1, 0.5]], taps=[OUT, OUT, DRY], rampSamples=1 << 20)
    b.SetMixGroup([4, 8], eye)
    b.SetMixGroup([0, 1, 0], [[1, 0, 0.25], [0, 1, 0.25]], taps=[OUT, OUT, DRY], rampSamples=0)
    assert b.GetMixInfo()["numGroups"] == 2
    got = b.GetStreamMix(1)
    assert (got["streams"], got["taps"], got["numOutputs"]) == ([0, 1, 0], [0, 0, 1], 2) and np.array_equal(got["gains"], np.array([[1, 0, 0.25], [0, 1, 0.25]], F))
    for streams, taken, kw in (([1, 0], 1, {}), ([0, 1], 0, {}), ([0, 1, 0], 0, dict(taps=[OUT, OUT, DRY], numOutputs=1)), ([5, 8], 8, {}), ([9, 5, 4], 4, {}),
                               ([5, 9, 1], 1, dict(taps=[OUT, OUT, DRY]))):
        with pytest.raises(na.NeuralAudioError, match="SetMixGroup: stream %d is already in another mix group" % taken):
            b.SetMixGroup(streams, np.eye(kw.get("numOutputs", 2), len(streams), dtype=F), **kw)
    # park dissolves the group at once, and the next call's rows are the twin's
    x = H.signal(128, 35)
    yt = twin_rows(na, models, x, [128], "rules")[0]
    b.ParkStream(8)
    assert b.GetStreamMix(4) is None and b.GetStreamMix(8) is None and b.GetMixInfo()["numGroups"] == 1
    b.ClearMixGroup(1)
    b.ActivateStream(8, 1.0)
    assert b.GetStreamMix(8) is None and np.array_equal(b.Process(x), yt)
    # a broken batch refuses everything
    b.SetWaitLimitMs(20.0)
    b.DebugStallDevice(80.0)
    with pytest.raises(na.NeuralAudioError, match="did not answer within"):
        b.Synchronize()
    assert b.IsBroken()
    for call in (lambda: b.SetMixGroup([0, 1], eye), lambda: b.ClearMixGroup(0), lambda: b.EnableMixStage()):
        with pytest.raises(na.NeuralAudioError, match="broken"):
            call()
    b.close()


def _raise(na):
    from neuralaudio_amd import capi
    raise na.NeuralAudioError(capi.last_error())


def test_remove_streams_dissolves_the_group(na, models):
    b = M.lstm_batch(na, models, 6)
    b.SetMixGroup([1, 2], np.eye(2, dtype=F) * F(0.5))
    b.SetMixGroup([4, 5, 3], [[1.0, 0.5, 0.5]], numOutputs=1)
    b.RemoveStreams(2, 1)
    assert b.GetMixInfo()["numGroups"] == 1 and b.GetStreamMix(1) is None
    assert b.AddStreams(models[H.LSTM], 1) == 2 and b.GetStreamMix(2) is None and b.GetStreamMix(3)["streams"] == [4, 5, 3]
    b.SetMixGroup([2, 1], np.eye(2, dtype=F))
    x = np.stack([H.noise(64, 800 + r) for r in range(6)])
    twin = M.lstm_batch(na, models, 6, mix=False)
    assert np.array_equal(b.Process(x), M.MixRef([4, 5, 3], [[1.0, 0.5, 0.5]], D=1).run(twin.Process(x)))
    twin.close()
    b.close()


def test_a_dry_tap_and_resampling_refuse_each_other(na, models):
    b = na.Batch(0)
    b.SetResampling(44100)
    assert b.AddStreams(models[H.LSTM], 3) == 0
    b.EnableMixStage()
    with pytest.raises(na.NeuralAudioError, match="SetMixGroup: a DRY tap is refused on a resampling batch"):
        b.SetMixGroup([0, 1, 0], [[1, 0.5, 0.5]], numOutputs=1, taps=[OUT, OUT, DRY])
    b.SetMixGroup([0, 1], [[1, 0.5]], numOutputs=1)  # (OUT taps are fine: the stage acts on the external-rate rows)
    assert b.GetMixInfo()["numGroups"] == 1
    b.close()
    b = M.lstm_batch(na, models, 3)
    b.SetMixGroup([0, 1, 0], [[1, 0.5, 0.5]], numOutputs=1, taps=[OUT, OUT, DRY])
    with pytest.raises(na.NeuralAudioError, match="SetResampling: a mix group with a DRY tap exists"):
        b.SetResampling(44100)
    b.close()


# ================================================================================================ 10: real-time safety

def test_set_clear_and_processing_with_groups_are_real_time_safe(na, models, lib):
    """NA_DebugDeviceResourceCalls stays where it is across set, gain-change and clear calls and 21 processing calls with groups (a
    DRY member among them), over the blocking and the pipelined host path and device pointers (after three warm calls of each,
    which size the staging block and the pipeline slots).  The one exception is the first call longer than drySamples."""
    import torch
    dev = torch.device("cuda", 0)
    b = M.make_batch(na, models, mix=True)
    n = 128
    x = H.signal(n, 36)
    dx, dy = torch.from_numpy(x).to(dev), torch.zeros(H.ROWS, n, device=dev)
    torch.cuda.synchronize(dev)

    def three():
        b.Process(x)
        b.Collect(b.Submit(x))
        b.ProcessDevice(dx.data_ptr(), dy.data_ptr(), n, n, n)
        b.Synchronize()

    b.SetMixGroup([0, 1], np.eye(2, dtype=F) * F(0.5), rampSamples=100)
    for _ in range(3):
        three()
    before = lib.NA_DebugDeviceResourceCalls()
    b.SetMixGroup([4, 8, 4], [[0.5, 0.5, 0.25]], numOutputs=1, taps=[OUT, OUT, DRY], rampSamples=300)
    for i in range(7):
        three()
        if i == 2:
            b.SetMixGroup([0, 1], [[0.2, 0.8], [0.8, 0.2]], rampSamples=64)
            b.ClearMixGroup(8)
        if i == 4:
            b.SetMixGroup([9, 5, 5], [[1.0, -1.0, 0.5]], numOutputs=1, taps=[OUT, OUT, DRY])
            b.ClearMixGroup(0)
    assert b.GetMixInfo()["numGroups"] == 1 and b.GetStreamMix(5)["streams"] == [9, 5, 5]
    assert lib.NA_DebugDeviceResourceCalls() == before
    b.Process(H.signal(2049, 37))
    assert lib.NA_DebugDeviceResourceCalls() > before and b.GetMixInfo()["drySamples"] == 4096
    b.close()
