"""GPU tests of the compressor stage (NA_BatchEnableCompressorStage / NA_BatchSetStreamCompressor, csrc/compressor_stage.h, DESIGN.md
2.19): a per-stream feed-forward compressor -- a level follower on the row's own samples, a gain curve of 513 knots, a multiplication --
behind the cabinet stage and in front of the delay stage.

Everything goes through the C ABI, beside a twin batch without the stage (tests/compressor_cases.py, as tests/test_gpu_gate.py does).
The contract is bit-exact: the expected row of a compressed stream is fl(twin_row * g_ref) with g_ref from the numpy float32
restatement run on the twin's row, of any other stream the twin's row, and every comparison is np.array_equal."""
import os

import numpy as np
import pytest

import compressor_cases as K
import gate_cases as G
import handover_cases as H

FORCED = bool(os.environ.get("NA_WN_KERNEL") or os.environ.get("NA_WN_PACK") or os.environ.get("NA_WN_SPEC") or os.environ.get("NA_SP_T")
              or os.environ.get("NA_SP_GEN") or os.environ.get("NA_WN_PAD"))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(FORCED, reason="forced kernel family")]

F = np.float32
PATHS = ("process", "registered", "submit", "device", "device-odd")
GROUP = 16  # entries of one workgroup of the kernel (kCompGroupEntries)
INF = float("inf")
# packed nano, Standard, and both live LSTM rows (as GATED of tests/test_gpu_gate.py): a soft-knee compressor with makeup, a limiter
# with an instant attack, a gentle wide-knee one, and a curve of the caller's own that lifts quiet levels and squashes loud ones
COMPRESSED = {0: K.params(0.3, 0.25, threshold_db=-60.0, ratio=4.0, knee_db=6.0, makeup_db=3.0),
              4: K.params(1.0, 0.3, threshold_db=-50.0, ratio=INF, knee_db=0.0),
              8: K.params(0.05, 0.3, threshold_db=-70.0, ratio=2.0, knee_db=12.0),
              9: K.params(0.7, 0.5, curve=np.minimum(4.0, 0.003 / np.maximum(K.LEVELS, 1e-9)) ** 0.5)}


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
    return capi.load_library().NA_DebugCompressorLaunches


def signal(total, seed=0, lead=0):
    """[ROWS, total]: every row alternates noise bursts at 0.25 and quiet stretches, each from its own noise (the gate tests' signal)"""
    return np.stack([G.gate_signal(300 * seed + r, total, lead) for r in range(H.ROWS)])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ================================================================================================ 1: off is off

def test_off_is_off(na, models, launches):
    """The stage is enabled and no stream has a compressor: every path gives the twin's bits and launches nothing of the stage."""
    calls = [128, 17, 300, 128]
    x = signal(sum(calls), 1)
    before = launches()
    for path in PATHS:
        y, yt, _ = K.run_scenario(na, models, x, calls, {}, path=path)
        assert np.array_equal(y, yt), path
        assert np.any(y[0]) and np.any(y[4]) and np.any(y[8]) and not np.any(y[2])
    assert launches() == before


def test_off_is_off_for_the_half_batch_launches(na, models, launches):
    """512 A1 Standard streams on the batch's own stream, device pointers: with the stage enabled and no compressor the free-running
    mode engages as in the twin and the bits are the twin's; a compressor on one stream orders the launches; taken away again (a fade
    of 32 samples ends inside the next call), the mode comes back with the call after.  One launch per call with an entry."""
    import torch
    dev = torch.device("cuda", 0)
    S, n, calls = 512, 128, 5
    x = np.stack([G.gate_signal(60 + r, calls * n) for r in range(5)])[np.arange(S) % 5]
    dx = torch.from_numpy(x).to(dev)
    torch.cuda.synchronize(dev)
    halves, outs = {}, {}
    p = K.params(0.3, 0.02, threshold_db=-50.0, ratio=4.0, knee_db=6.0)
    for stage in (True, False):
        b = na.Batch(0)
        assert b.ReserveStreams(models[H.STD], S) == 0
        for s in range(S):
            b.ActivateStream(s, 1.0)
        if stage:
            b.EnableCompressorStage()
        dy = torch.zeros(S, calls * n, device=dev)
        before = launches()
        for k in range(calls):
            if stage and k == 2:
                b.SetStreamCompressor(7, p, 0)
            if stage and k == 3:
                b.SetStreamCompressor(7, None, 32)
            b.ProcessDevice(dx.data_ptr() + 4 * k * n, dy.data_ptr() + 4 * k * n, n, calls * n, calls * n)
            b.Synchronize()
            halves[(stage, k)] = b.UsesHalfLaunches()
        assert launches() - before == (2 if stage else 0), "one launch per call with an entry"
        outs[stage] = dy.cpu().numpy()
        b.close()
    for k in (0, 1, 4):
        assert halves[(True, k)] == halves[(False, k)], k
    print("half-batch launches: twin %s, with a compressor %s, in the removal's fade %s, behind it %s" % (halves[(False, 1)], halves[(True, 2)], halves[(True, 3)], halves[(True, 4)]))
    assert not halves[(True, 2)] and not halves[(True, 3)]
    ref = K.CompRef()
    ref.set(p, 0)
    g = ref.run(outs[False][7, 2 * n:3 * n])
    ref.set(None, 32)
    g = np.concatenate([g, ref.run(outs[False][7, 3 * n:4 * n])])
    expect = outs[False].copy()
    expect[7, 2 * n:4 * n] = outs[False][7, 2 * n:4 * n] * g
    assert not ref.has and np.any(g < 1) and np.array_equal(outs[True], expect)


# ================================================================================================ 2: one stream of each family

def _gates_in_front(b):
    """what twin and batch under test share: a noise gate that starts closed, with a floor of 0, on the rows that get a compressor --
    so that the rows the compressor listens to hold exact zeros before the first burst and in the long gaps, whatever the models make
    of silence: the follower starts at zero and falls back through the subnormals"""
    b.EnableGateStage()
    for s in COMPRESSED:
        b.SetStreamGate(s, G.params(), False)


def _conditions(contract):
    for s in COMPRESSED:
        K.assert_inputs_reach_every_case(contract.comp[s], contract.gains[s], ("row", s))


@pytest.mark.parametrize("path", PATHS)
def test_compressors_on_one_stream_of_each_family(na, models, launches, path):
    """Compressors on rows 0 (packed nano), 4 (Standard), 8 and 9 (LSTM), one kind each, over 1700 samples of the burst signal.  Call
    lengths: the RAGGED list, 127, 128, 129 and the rest.  Every row of every call is checked (run_scenario): the compressed rows equal
    fl(twin_row * g_ref), all others -- the packed neighbours of row 0 among them -- the twin's.  The condition on the inputs is
    asserted on the restatement alone, on the twin's rows and before the batch under test exists: every compressed row takes both
    branches of c, has levels below knot 0 (zero and subnormal ones among them), crosses at least three octaves of knots and has g < 1
    on at least a quarter of its samples."""
    total = 1700
    x = signal(total, 2, lead=60)
    calls = list(H.RAGGED) + [127, 128, 129]
    calls.append(total - sum(calls))
    assert calls[-1] > 0
    ops = {0: [("comp", s, p, 0) for s, p in COMPRESSED.items()]}
    seen = {}

    def hook(b, expected, i):
        seen[i] = b.GetCompressorInfo()

    before = launches()
    y, yt, contract = K.run_scenario(na, models, x, calls, ops, path=path, before=_gates_in_front, check=_conditions, hook=hook)
    assert launches() - before == len(calls), "one launch per call, whatever n"
    assert seen[0]["numCompressors"] == 4 and seen[0]["curvePoints"] == 513 and seen[0]["deviceBytes"] >= 16 * 4232
    g9 = np.concatenate(contract.gains[9])
    assert np.any(g9 > 1) and np.any(g9 < 1), "the caller's own curve lifts and squashes"
    for s in (1, 5):
        assert np.array_equal(y[s], yt[s])
    for s in COMPRESSED:
        assert not np.array_equal(y[s], yt[s])


# ================================================================================================ 3: the cut never shows

CUTS = ([128, 17, 300, 128], [573], [1] * 573, [127, 129, 1, 316])


def test_the_cut_into_calls_never_shows(na, models):
    """The same 573 samples in four calls, in one, in calls of one sample and in cuts around the tile's length, on the device-odd path
    (an odd row stride, rows that are not 16-byte aligned): the same bits, each the reference's.  Row 4 changes its curve over a fade
    of 200 samples from sample 128 on where the cut allows a set call there: the fade's weight is a matter of position too."""
    x = signal(573, 3)
    ops = {0: [("comp", s, p, 0) for s, p in COMPRESSED.items()]}
    outs = []
    for calls in CUTS:
        assert sum(calls) == 573
        y, _, contract = K.run_scenario(na, models, x, calls, ops, path="device-odd")
        outs.append(y)
    for y in outs[1:]:
        assert np.array_equal(outs[0], y)
    g = np.concatenate(contract.gains[4])
    assert np.all(g < 1) and len(np.unique(g)) > 100, "the limiter works on every sample, and the gain moves"
    # ... and a fade that starts at sample 128 and runs across the cuts behind it
    fading = []
    for calls in (CUTS[0], [128] + [1] * 445, [128, 127, 129, 189]):
        at = {0: ops[0], 1: [("comp", 4, COMPRESSED[0], 200), ("comp", 8, None, 333)]}
        y, _, contract = K.run_scenario(na, models, x, calls, at, path="device-odd")
        fading.append(y)
    assert np.array_equal(fading[0], fading[1]) and np.array_equal(fading[0], fading[2]) and not np.array_equal(fading[0], outs[0])
    assert not contract.comp[8].has, "faded to none and retired"


def test_in_place(na, models):
    """NA_BatchProcessDevice with dIn == dOut on compressed streams: the bits of separate buffers."""
    import torch
    dev = torch.device("cuda", 0)
    calls = CUTS[0]
    x = signal(sum(calls), 4)
    outs = {}
    for in_place in (False, True):
        b = K.make_batch(na, models, stage=True)
        for s, p in COMPRESSED.items():
            b.SetStreamCompressor(s, p, 0)
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
    yt = np.concatenate(H.run_twin(na, models, x, calls, {}), axis=1)
    ref = K.CompRef()
    ref.set(COMPRESSED[4], 0)
    assert np.array_equal(outs[True][4], (yt[4] * ref.run(yt[4])).astype(np.float32)) and not np.array_equal(outs[True][4], yt[4])


# ================================================================================================ 4: more entries than one workgroup

def _distinct(r):
    return K.params(0.05 + 0.02 * r, 0.5 / (1 + r), threshold_db=-60.0 + r, ratio=[2.0, 4.0, INF][r % 3], knee_db=[0.0, 3.0, 12.0, 6.0][r % 4], makeup_db=0.25 * (r % 5))


@pytest.mark.parametrize("path", ["process", "device-odd"])
def test_more_entries_than_one_workgroup_owns(na, models, launches, path):
    """40 BossWN-nano streams (four to a virtual stream), independent inputs, distinct curves and coefficients: 1 entry, then
    GROUP + 1 = 17 -- one more than a workgroup owns, the last workgroup with a single entry --, then 2 * GROUP + 1 = 33, then 32
    once one compressor has been taken away at once.  device-odd: an odd row stride and rows that are not 16-byte aligned."""
    S = 40
    comp = [r for r in range(S) if r not in (0, 5, 13, 22, 31, 36, 39)]
    assert len(comp) == 2 * GROUP + 1
    calls = [130, 129, 300, 127]
    x = np.stack([G.gate_signal(800 + r, sum(calls), lead=(7 * r) % 90) for r in range(S)])
    ops = {0: comp[:1], 1: comp[1:GROUP + 1], 2: comp[GROUP + 1:]}
    batches = {}
    for stage in (False, True):
        b = na.Batch(0)
        assert b.AddStreams(models[H.NANO], S) == 0
        if stage:
            b.EnableCompressorStage()
        batches[stage] = b
    runner, twin = H.Runner(na, batches[True], path), batches[False]
    refs, pos, counts = {}, 0, []
    before = launches()
    try:
        for i, n in enumerate(calls):
            for r in ops.get(i, ()):
                batches[True].SetStreamCompressor(r, _distinct(r), 0 if r % 2 else 40)
                refs[r] = K.CompRef()
                refs[r].set(_distinct(r), 0 if r % 2 else 40)
            if i == 3:
                batches[True].SetStreamCompressor(comp[0], None, 0)
                refs[comp[0]].set(None, 0)
            counts.append(batches[True].GetCompressorInfo()["numCompressors"])
            xs = np.ascontiguousarray(x[:, pos:pos + n])
            yt, y = twin.Process(xs), runner.call(xs)
            for r in range(S):
                e = yt[r]
                if r in refs and refs[r].has:
                    e = (yt[r] * refs[r].run(yt[r])).astype(np.float32)
                assert np.array_equal(y[r], e), (path, "call", i, "row", r)
            pos += n
        assert counts == [1, GROUP + 1, 2 * GROUP + 1, 2 * GROUP] and launches() - before == len(calls)
        assert batches[True].GetStreamCompressor(comp[0]) is None
        for r in (comp[0], comp[GROUP], comp[-1]):
            want = 1.0 if r == comp[0] else float(refs[r].last_g)
            assert batches[True].StreamCompressorGain(r) == want, r
        assert any(np.any(np.concatenate(refs[r].levels) > 0) and refs[r].last_g < 1 for r in comp[1:])
    finally:
        runner.close()
        for b in batches.values():
            b.close()


# ================================================================================================ 5: levels at the edges

def test_levels_at_the_edges(na, models):
    """NA_DebugRunCompressorStage on host rows, the stage alone.  Row 0: exact zeros, then subnormal samples under a slow attack (a
    subnormal follower), then zeros again.  Row 1: a row at 300.0 with aA = 1 -- clamped to 255, the last segment, i = 511, f = 0.875.
    Row 4: NaN and +-inf samples between ordinary ones: they pass (NaN stays NaN, inf stays inf with its sign), the follower sees 0 and
    255 and does not become NaN.  Row 5: a row stepping exactly on the knots (aA = aR = 1, f = 0): the gains are the table's own
    values.  Two calls of 200 and 313 samples (the second carries the state), rows of stride 517."""
    b = H.make_batch(na, models, stage=False)
    b.EnableCompressorStage()
    n, stride = 513, 517
    rng = np.random.default_rng(5)
    rows = np.zeros((H.ROWS, stride), np.float32)
    rows[0, 100:300] = (rng.integers(1, 4000, 200) * 2.0 ** -149 * rng.choice([-1.0, 1.0], 200)).astype(np.float32)
    rows[1, :n] = 300.0
    rows[1, 400:n] = -300.0
    rows[4, :n] = (0.3 * rng.standard_normal(n)).astype(np.float32)
    rows[4, [10, 50, 51, 120, 260, 261, 400]] = [np.nan, np.inf, -np.inf, np.nan, -np.inf, np.nan, np.inf]
    rows[5, :n] = K.LEVELS[::-1].astype(np.float32)
    rows[5, 0] = 255.0  # (level 256 is beyond the clamp)
    rows[5, 1::2] *= -1.0
    rows[:, n:] = 7.0   # (beyond the row: must stay)
    curve = (0.5 + np.arange(K.POINTS) / 1024.0).astype(np.float32)  # (every knot its own value, none of them 0: inf * g stays inf)
    setting = {0: dict(attackCoeff=2.0 ** -12, releaseCoeff=0.5, curve=curve), 1: dict(attackCoeff=1.0, releaseCoeff=1.0, curve=curve),
               4: dict(attackCoeff=0.4, releaseCoeff=0.1, curve=curve), 5: dict(attackCoeff=1.0, releaseCoeff=1.0, curve=curve)}
    refs = {}
    for s, p in setting.items():
        b.SetStreamCompressor(s, p, 0)
        refs[s] = K.CompRef()
        refs[s].set(p, 0)
    x = rows.copy()
    got = np.zeros_like(rows)
    for lo, hi in ((0, 200), (200, n)):
        piece = np.ascontiguousarray(np.pad(rows[:, lo:hi], ((0, 0), (0, stride - (hi - lo))), constant_values=7.0))
        b.DebugRunCompressorStage(piece, hi - lo)
        assert np.all(piece[:, hi - lo:] == 7.0), "the stage wrote past the end of a row"
        got[:, lo:hi] = piece[:, :hi - lo]
    gains = {s: np.concatenate([refs[s].run(x[s, :200]), refs[s].run(x[s, 200:n])]) for s in refs}
    for s in refs:
        with np.errstate(invalid="ignore"):
            want = (x[s, :n] * gains[s]).astype(np.float32)
        nan = np.isnan(x[s, :n])
        assert np.array_equal(np.isnan(got[s, :n]), nan), s
        assert np.array_equal(_bits(got[s, :n])[~nan], _bits(want)[~nan]), (s, int(np.flatnonzero(_bits(got[s, :n]) != _bits(want))[0]))
        assert b.StreamCompressorGain(s) == float(gains[s][-1])
    for s in (8, 9):
        assert np.array_equal(got[s, :n], x[s, :n])
    lev0 = np.concatenate(refs[0].levels)
    assert np.all(lev0[:100] == 0) and np.any((lev0 > 0) & (lev0 < F(2.0 ** -126))) and np.all(gains[0] == curve[0]) and np.all(np.isfinite(lev0))
    assert np.all(np.concatenate(refs[1].levels) == 255.0) and np.all(gains[1] == F(curve[511] + F(F(0.875) * F(curve[512] - curve[511]))))
    lev4 = np.concatenate(refs[4].levels)
    assert np.all(np.isfinite(lev4)) and lev4[50] > 100 and np.all(np.isinf(got[4, [50, 51, 260, 400]])) and got[4, 51] < 0 < got[4, 50]
    assert np.array_equal(np.concatenate(refs[5].levels)[1:], K.LEVELS[::-1].astype(np.float32)[1:]) and np.array_equal(gains[5][1:], curve[::-1][1:])
    b.close()


# ================================================================================================ 6: set, change and remove

def test_set_change_and_remove(na, models, launches):
    """Row 4: set with fadeSamples 0, changed with a fade of 1, then of 100 (ends inside a call), then of 300 (spans three calls);
    row 9: faded in over 64, new coefficients alone on the kept e (the same curve, fadeSamples 0), then taken away over 150 samples:
    the entry retires with the call that holds the fade's last sample and the row carries the twin's bits behind it.  A set call during
    a fade is refused with the samples left.  NA_BatchStreamCompressorGain equals the reference's last g after every call,
    NA_BatchStreamCompressorFadeRemaining the reference's count."""
    calls = [100, 128, 128, 128, 128, 128, 100, 128, 64]
    x = signal(sum(calls), 5)
    a, b_, c, d = COMPRESSED[0], COMPRESSED[4], COMPRESSED[8], COMPRESSED[9]
    faster = dict(attackCoeff=0.9, releaseCoeff=0.01, curve=c["curve"])
    ops = {0: [("comp", 4, a, 0), ("comp", 9, c, 64)], 1: [("comp", 4, b_, 1), ("comp", 9, faster, 0)], 2: [("comp", 4, d, 100)],
           3: [("comp", 4, a, 300), ("comp", 9, None, 150)], 7: [("comp", 4, None, 0)]}
    count, refusals = {}, []

    def hook(b, expected, i):
        count[i] = launches()
        _, entries, rows = expected
        assert b.GetCompressorInfo()["numCompressors"] == entries, i
        for s in (4, 9):
            last_g, left, has = rows[s]
            assert b.StreamCompressorGain(s) == float(last_g), (i, s)
            assert b.StreamCompressorFadeRemaining(s) == left, (i, s)
            assert (b.GetStreamCompressor(s) is not None) == has, (i, s)
        if i == 3:
            assert rows[4][1] == 172 and rows[9][1] == 22
            for s, left in ((4, 172), (9, 22)):
                with pytest.raises(na.NeuralAudioError, match=r"SetStreamCompressor: a compressor fade of stream %d is running \(%d samples left\)" % (s, left)):
                    b.SetStreamCompressor(s, d, 0)
                with pytest.raises(na.NeuralAudioError, match=r"is running \(%d samples left\)" % left):
                    b.SetStreamCompressor(s, None, 10)
                refusals.append(s)
        if i == 1:
            got = b.GetStreamCompressor(9)
            assert got["attackCoeff"] == float(F(0.9)) and np.array_equal(got["curve"], c["curve"])

    before = launches()
    y, yt, contract = K.run_scenario(na, models, x, calls, ops, hook=hook)
    assert refusals == [4, 9]
    assert not contract.comp[9].has and not contract.comp[4].has
    done9 = sum(calls[:5])  # (150 samples from the start of call 3: the fade ends inside call 4)
    assert np.array_equal(y[9, done9:], yt[9, done9:]) and not np.array_equal(y[9, :done9], yt[9, :done9])
    assert count[6] - count[5] == 1 and count[7] == count[6] and count[8] == count[7], "the counter stops with the last entry"
    assert count[8] - before == 7
    assert np.array_equal(y[4, sum(calls[:7]):], yt[4, sum(calls[:7]):])


# ================================================================================================ 7: rules

def test_rules(na, models):
    """Each refusal carries its text; park, remove and the park that ends a hand-over drop the compressor; an activated stream has
    none; save and load leave compressors alone; a broken batch refuses everything."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    b = H.make_batch(na, models, stage=True)  # (with the output stage, for the hand-over)
    p = COMPRESSED[0]
    for call in (lambda: b.SetStreamCompressor(0, p), lambda: b.SetStreamCompressor(0, None), lambda: b.GetStreamCompressor(0), lambda: b.StreamCompressorGain(0),
                 lambda: b.StreamCompressorFadeRemaining(0), lambda: b.GetCompressorInfo(), lambda: b.DebugRunCompressorStage(np.zeros((H.ROWS, 8), np.float32))):
        with pytest.raises(na.NeuralAudioError, match=r"compressor stage not enabled \(NA_BatchEnableCompressorStage\)"):
            call()
    assert lib.NA_BatchGetStreamCompressor(b._h, 0, None) < 0 and lib.NA_BatchStreamCompressorGain(b._h, 0) < 0
    b.EnableCompressorStage()
    b.EnableCompressorStage()
    info = b.GetCompressorInfo()
    assert info["curvePoints"] == 513 and info["numCompressors"] == 0 and info["deviceBytes"] >= 16 * 4232
    with pytest.raises(na.NeuralAudioError, match="SetStreamCompressor: stream 2 is parked"):
        b.SetStreamCompressor(2, p)
    with pytest.raises(na.NeuralAudioError, match="SetStreamCompressor: stream 12 is not a live stream of the batch"):
        b.SetStreamCompressor(12, p)
    with pytest.raises(na.NeuralAudioError, match="GetStreamCompressor: stream 12 is not a stream of the batch"):
        b.GetStreamCompressor(12)
    with pytest.raises(na.NeuralAudioError, match="StreamCompressorGain: stream -1 is not a stream of the batch"):
        b.StreamCompressorGain(-1)
    with pytest.raises(na.NeuralAudioError, match="StreamCompressorFadeRemaining: stream 40 is not a stream of the batch"):
        b.StreamCompressorFadeRemaining(40)

    def changed(**fields):
        q = dict(p)
        q["curve"] = p["curve"].copy()
        for name, v in fields.items():
            if name.startswith("curve"):
                q["curve"][int(name[5:])] = v
            else:
                q[name] = v
        return q

    nan = float("nan")
    for change, text in ((dict(attackCoeff=nan), "attackCoeff must be finite"), (dict(releaseCoeff=INF), "releaseCoeff must be finite"),
                         (dict(attackCoeff=0.0), r"attackCoeff must lie in \(0, 1\]"), (dict(attackCoeff=1.5), r"attackCoeff must lie in \(0, 1\]"),
                         (dict(releaseCoeff=-0.1), r"releaseCoeff must lie in \(0, 1\]"), (dict(releaseCoeff=1.0001), r"releaseCoeff must lie in \(0, 1\]"),
                         (dict(curve0=nan), r"curve\[0\] must be finite"), (dict(curve512=INF), r"curve\[512\] must be finite"),
                         (dict(curve100=-1e-9), r"curve\[100\] must lie in \[0, 65536\]"), (dict(curve511=65537.0), r"curve\[511\] must lie in \[0, 65536\]")):
        with pytest.raises(na.NeuralAudioError, match="SetStreamCompressor: " + text):
            b.SetStreamCompressor(0, changed(**change))
    for fade in (-1, (1 << 20) + 1):
        with pytest.raises(na.NeuralAudioError, match=r"SetStreamCompressor: fadeSamples must lie in \[0, 1 << 20\]"):
            b.SetStreamCompressor(0, p, fade)
    with pytest.raises(na.NeuralAudioError, match="a compressor curve has 513 values"):
        b.SetStreamCompressor(0, dict(attackCoeff=1.0, releaseCoeff=1.0, curve=np.ones(512, np.float32)))
    assert b.GetCompressorInfo()["numCompressors"] == 0 and b.GetStreamCompressor(0) is None and b.StreamCompressorGain(0) == 1.0
    b.SetStreamCompressor(0, changed(attackCoeff=1.0, releaseCoeff=2.0 ** -149, curve0=0.0, curve512=65536.0), 1 << 20)
    assert b.StreamCompressorGain(0) == 1.0 and b.StreamCompressorFadeRemaining(0) == 1 << 20, "nothing produced yet"
    b.SetStreamCompressor(1, None, 100)  # (no compressor: nothing to take away)
    assert b.GetCompressorInfo()["numCompressors"] == 1
    b.ParkStream(0)
    assert b.GetCompressorInfo()["numCompressors"] == 0
    b.ActivateStream(0, 1.0)
    assert b.GetStreamCompressor(0) is None and b.StreamCompressorGain(0) == 1.0 and b.StreamCompressorFadeRemaining(0) == 0
    # park, remove and the end of a hand-over drop the compressor at once; an activated stream has none
    for s in (0, 1, 4, 5, 8):
        b.SetStreamCompressor(s, p, 0)
    assert b.GetCompressorInfo()["numCompressors"] == 5 and np.array_equal(b.GetStreamCompressor(4)["curve"], p["curve"])
    b.ParkStream(0)
    assert b.GetCompressorInfo()["numCompressors"] == 4 and b.GetStreamCompressor(0) is None
    b.ActivateStream(0, 1.0)
    assert b.GetStreamCompressor(0) is None
    blob = b.SaveStreams([5])
    b.LoadStreams([4], blob)
    assert b.GetStreamCompressor(4) is not None and b.GetCompressorInfo()["numCompressors"] == 4
    b.Handover(4, 6, 1.0, 64)
    x = signal(64, 7)
    b.Process(x)
    assert b.GetStreamCompressor(4) is not None and b.GetStreamCompressor(6) is None
    b.Process(x)  # (parks row 4 in front of its launches)
    assert b.IsParked(4) and b.GetStreamCompressor(4) is None and b.GetCompressorInfo()["numCompressors"] == 3
    # the stage grows with the batch
    first = b.ReserveStreams(models[H.LSTM], 30)
    b.ActivateStream(first + 29, 1.0)
    b.SetStreamCompressor(first + 29, p, 10)
    y = b.Process(signal(64, 8)[np.arange(b.NumStreams()) % H.ROWS])
    assert np.any(y[first + 29]) and np.all(np.isfinite(y)) and b.GetStreamCompressor(1) is not None
    # a broken batch refuses everything
    b.SetWaitLimitMs(20.0)
    b.DebugStallDevice(80.0)
    with pytest.raises(na.NeuralAudioError, match="did not answer within"):
        b.Synchronize()
    assert b.IsBroken()
    for call in (lambda: b.SetStreamCompressor(1, p), lambda: b.SetStreamCompressor(1, None), lambda: b.StreamCompressorGain(1), lambda: b.EnableCompressorStage()):
        with pytest.raises(na.NeuralAudioError, match="broken"):
            call()
    b.close()


def test_remove_streams_drops_the_compressor(na, models):
    b = na.Batch(0)
    assert b.AddStreams(models[H.LSTM], 4) == 0
    b.EnableCompressorStage()
    b.SetStreamCompressor(1, COMPRESSED[0], 0)
    b.SetStreamCompressor(2, COMPRESSED[4], 50)
    b.RemoveStreams(1, 1)
    assert b.GetCompressorInfo()["numCompressors"] == 1
    assert b.AddStreams(models[H.LSTM], 1) == 1 and b.GetStreamCompressor(1) is None and b.GetStreamCompressor(2) is not None
    b.close()


# ================================================================================================ 8: real-time safety

def test_set_calls_and_processing_with_compressors_are_real_time_safe(na, models):
    """NA_DebugDeviceResourceCalls stays where it is across set, change and remove calls and 21 processing calls with entries, over the
    blocking and the pipelined host path and device pointers (after three warm calls of each, which size the staging block and the
    pipeline slots)."""
    import torch
    from neuralaudio_amd import capi
    lib = capi.load_library()
    dev = torch.device("cuda", 0)
    b = K.make_batch(na, models, stage=True)
    n = 128
    x = signal(n, 9)
    dx, dy = torch.from_numpy(x).to(dev), torch.zeros(H.ROWS, n, device=dev)
    torch.cuda.synchronize(dev)

    def three():
        b.Process(x)
        b.Collect(b.Submit(x))
        b.ProcessDevice(dx.data_ptr(), dy.data_ptr(), n, n, n)
        b.Synchronize()

    b.SetStreamCompressor(0, COMPRESSED[0], 0)
    for _ in range(3):
        three()
    before = lib.NA_DebugDeviceResourceCalls()
    b.SetStreamCompressor(4, COMPRESSED[4], 200)
    b.SetStreamCompressor(8, COMPRESSED[8], 0)
    for i in range(7):
        three()
        if i == 2:
            b.SetStreamCompressor(0, COMPRESSED[9], 100)
            b.SetStreamCompressor(8, None, 64)
        if i == 4:
            b.SetStreamCompressor(9, COMPRESSED[9], 0)
            b.SetStreamCompressor(4, None, 0)
    assert b.GetStreamCompressor(8) is None and b.GetStreamCompressor(4) is None and b.GetCompressorInfo()["numCompressors"] == 2
    assert lib.NA_DebugDeviceResourceCalls() == before
    b.close()


# ================================================================================================ 9: position in the chain

@pytest.mark.parametrize("resample", [None, 44100])
def test_the_compressor_sits_between_the_cabinet_and_the_delay(na, models, resample):
    """Rows 4 and 9 have a gate, an EQ, an IR, a compressor, a delay and an output gain of 0.5.  The twin chain: a batch with gate, EQ
    and IR alone gives the rows behind the cabinet; the restatement compresses them; a batch with nothing but the delay stage runs its
    stage on those rows (NA_DebugRunDelayStage); times 0.5, exactly.  The row must carry those bits -- and not those of a compressor
    behind the delay.  Once more on a 44.1 kHz resampling batch, where the stages act on the external-rate rows."""
    calls = [128, 129, 300, 443]
    total = sum(calls)
    x = signal(total, 10)
    rng = np.random.default_rng(5)
    taps = (rng.standard_normal(40) * np.exp(-np.arange(40) / 8.0) * 0.3).astype(np.float32)
    rate = resample or 48000
    eq = [na.eq_section("lowshelf", rate, 200.0, gain_db=4.0), na.eq_section("peaking", rate, 1500.0, 1.2, -3.0)]
    echo = na.delay_params_from_ms(rate, 2.5, feedback=0.4)
    p = COMPRESSED[4]

    def chain(b, whole):
        b.EnableGateStage()
        b.EnableEqStage()
        b.EnableCabinetStage(64)
        if whole:
            b.EnableCompressorStage()
            b.EnableDelayStage(4096)
            b.EnableOutputStage()
        ir = b.LoadIR(taps)
        for s in (4, 9):
            b.SetStreamGate(s, G.params(floorGain=0.1), True)
            b.SetStreamEq(s, eq, 0)
            b.SetStreamIR(s, ir, 0)
            if whole:
                b.SetStreamCompressor(s, p, 0)
                b.SetStreamDelay(s, echo, 0)
                b.SetStreamGain(s, 0.5, 0)

    def run(whole):
        b = H.make_batch(na, models, stage=False, resample=resample)
        chain(b, whole)
        out, pos = [], 0
        for n in calls:
            out.append(b.Process(np.ascontiguousarray(x[:, pos:pos + n])))
            pos += n
        b.close()
        return np.concatenate(out, axis=1)

    y, cab = run(True), run(False)

    def delayed(rows):
        d = H.make_batch(na, models, stage=False)
        d.EnableDelayStage(4096)
        for s in (4, 9):
            d.SetStreamDelay(s, echo, 0)
        out = d.DebugRunDelayStage(np.ascontiguousarray(rows))
        d.close()
        return out

    def compressed(rows):
        out = rows.copy()
        for s in (4, 9):
            ref = K.CompRef()
            ref.set(p, 0)
            g = ref.run(rows[s])
            assert np.any(g < 1) and np.any(g[1:] != g[:-1])
            out[s] = (rows[s] * g).astype(np.float32)
        return out

    expect, wrong = delayed(compressed(cab)), compressed(delayed(cab))
    for s in (4, 9):
        assert np.array_equal(y[s], (expect[s] * F(0.5)).astype(np.float32)), s
        assert not np.array_equal(y[s], (wrong[s] * F(0.5)).astype(np.float32)), "the test can tell the two orders apart"
    for s in (0, 1, 5, 8):
        assert np.array_equal(y[s], cab[s])
