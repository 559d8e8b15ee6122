"""GPU tests of the EQ stage (NA_BatchEnableEqStage / NA_BatchSetStreamEq, csrc/eq_stage.h): a cascade of up to 8 biquad
sections per stream in f64, behind the gate's apply and in front of the cabinet stage.

Everything goes through the C ABI.  The contract is bit-exact: the expected row of a stream with a cascade is the Python restatement
(tests/eq_cases.py) run on the row a twin batch without the stage produced -- or, through NA_DebugRunEqStage, on the rows the test
chose -- the expected row of any other stream is that row itself, and every comparison is on the bits.  The models are BossLSTM-1x16
(rows 0-3) and BossWN-standard (rows 4-7), from NA_BatchReserveStreams; rows 0, 1, 2, 4, 5 are live."""
import os

import numpy as np
import pytest

import cabinet_cases as CAB
import eq_cases as E
import gate_cases as G
import na_oracle as O

FORCED = bool(os.environ.get("NA_WN_KERNEL") or os.environ.get("NA_WN_PACK") or os.environ.get("NA_WN_SPEC") or os.environ.get("NA_SP_T")
              or os.environ.get("NA_SP_GEN") or os.environ.get("NA_WN_PAD"))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(FORCED, reason="forced kernel family")]

LSTM, STD = "BossLSTM-1x16.nam", "BossWN-standard.nam"
ROWS, LIVE = 8, (0, 1, 2, 4, 5)
PATHS = ("process", "device-odd", "submit")
F = np.float32


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


@pytest.fixture(scope="module")
def models(na):
    loader = na.NeuralModelLoader()
    out = {name: loader.CreateFromFile(os.path.join(O.MODELS_DIR, name), doPrewarm=False) for name in (LSTM, STD)}
    assert all(m is not None for m in out.values())
    out["loader"] = loader
    return out


@pytest.fixture(scope="module")
def launches():
    from neuralaudio_amd import capi
    return capi.load_library().NA_DebugEqLaunches


def make_batch(na, models, eq=True, resample=None, out_stage=False):
    b = na.Batch(0)
    if resample:
        b.SetResampling(resample)
    assert b.ReserveStreams(models[LSTM], 4) == 0 and b.ReserveStreams(models[STD], 4) == 4
    for s in LIVE:
        b.ActivateStream(s, 1.0)
    if out_stage:
        b.EnableOutputStage()
    if eq:
        b.EnableEqStage()
    return b


def signal(total, seed=0):
    return np.stack([E.noise(total, 1000 * seed + 17 * r + 3) for r in range(ROWS)])


_twins = {}


@pytest.fixture(scope="module")
def twin(na, models):
    """the rows of a batch without the stage, call by call: computed once per (signal, cut, rate) and shared"""
    def rows(x, calls, resample=None, key=None):
        key = (key, tuple(calls), resample)
        if key[0] is None or key not in _twins:
            b = make_batch(na, models, eq=False, resample=resample)
            out, pos = [], 0
            for n in calls:
                out.append(b.Process(np.ascontiguousarray(x[:, pos:pos + n])))
                pos += n
            b.close()
            _twins[key] = np.concatenate(out, axis=1)
            _twins[key].setflags(write=False)
        return _twins[key]
    return rows


class Runner:
    """Feeds a batch call by call through one entry point; every call returns host rows [rows, n].  device-odd: device pointers, an odd
    row stride and a base that is 4 bytes past a 16-byte boundary."""

    def __init__(self, batch, path):
        self.b, self.path = batch, path

    def call(self, x):
        b = self.b
        x = np.ascontiguousarray(x)
        rows, n = x.shape
        if self.path == "process":
            return b.Process(x)
        if self.path == "submit":
            return b.Collect(b.Submit(x))
        import torch
        dev = torch.device("cuda", 0)
        stride = n + (3 if n % 2 == 0 else 4)
        assert stride % 2 == 1
        dx = torch.from_numpy(x).to(dev)
        dy = torch.zeros(1 + rows * stride, device=dev)
        torch.cuda.synchronize(dev)
        assert dy.data_ptr() % 16 == 0
        b.ProcessDevice(dx.data_ptr(), dy.data_ptr() + 4, n, n, stride)
        b.Synchronize()
        flat = dy.cpu().numpy()
        out = flat[1:].reshape(rows, stride)
        assert flat[0] == 0.0 and not np.any(out[:, n:]), "the stage wrote outside a row"
        return out[:, :n].copy()


def assert_rows(y, expect, what):
    for s in range(y.shape[0]):
        if not E.same_bits(y[s], expect[s]):
            bad = np.flatnonzero(y[s].view(np.uint32) != np.ascontiguousarray(expect[s]).view(np.uint32))
            raise AssertionError((what, "row", s, len(bad), "samples differ, first at", int(bad[0]), float(y[s][bad[0]]), float(expect[s][bad[0]])))


# ================================================================================================ off is off

def test_off_is_off(na, models, launches, twin):
    """The stage is enabled and no stream has an EQ: every path gives the twin's bits and launches nothing of the stage."""
    calls = [128, 17, 300, 128]
    x = signal(sum(calls), 1)
    yt = twin(x, calls, key="off")
    before = launches()
    for path in PATHS:
        b = make_batch(na, models)
        run, pos = Runner(b, path), 0
        for n in calls:
            y = run.call(x[:, pos:pos + n])
            assert_rows(y, yt[:, pos:pos + n], (path, pos))
            pos += n
        assert b.GetEqInfo()["numEntries"] == 0
        b.close()
    assert np.any(yt[0]) and np.any(yt[4]) and not np.any(yt[3])
    assert launches() == before


def test_off_is_off_for_the_half_batch_launches(na, models, launches):
    """512 A1 Standard streams on the batch's own stream, device pointers: with the stage enabled and no EQ the free-running mode
    engages as in the twin and the bits are the twin's; an EQ on one stream orders the launches; flat again (N = 0: the entry retires
    with the set call), the mode is back with the next call."""
    import torch
    dev = torch.device("cuda", 0)
    S, n, K = 512, 128, 5
    x = np.stack([E.noise(K * n, 60 + r) for r in range(5)])[np.arange(S) % 5]
    dx = torch.from_numpy(x).to(dev)
    torch.cuda.synchronize(dev)
    halves, outs = {}, {}
    sections = E.cascade(3, 1)
    for stage in (True, False):
        b = na.Batch(0)
        assert b.ReserveStreams(models[STD], S) == 0
        for s in range(S):
            b.ActivateStream(s, 1.0)
        if stage:
            b.EnableEqStage()
        dy = torch.zeros(S, K * n, device=dev)
        before = launches()
        for k in range(K):
            if stage and k == 2:
                b.SetStreamEq(7, sections, 0)
            if stage and k == 3:
                b.SetStreamEq(7, None, 0)
            b.ProcessDevice(dx.data_ptr() + 4 * k * n, dy.data_ptr() + 4 * k * n, n, K * n, K * n)
            b.Synchronize()
            halves[(stage, k)] = b.UsesHalfLaunches()
        assert launches() - before == (1 if stage else 0), "one launch per call with an entry"
        outs[stage] = dy.cpu().numpy()
        b.close()
    for k in (0, 1, 3, 4):
        assert halves[(True, k)] == halves[(False, k)], k
    print("half-batch launches: twin %s, with an EQ %s, behind it %s" % (halves[(False, 1)], halves[(True, 2)], halves[(True, 3)]))
    assert not halves[(True, 2)]
    ref = E.EqRef()
    ref.set(sections)
    expect = outs[False].copy()
    expect[7, 2 * n:3 * n] = ref.run(outs[False][7, 2 * n:3 * n])
    assert not E.same_bits(expect[7], outs[False][7])
    assert_rows(outs[True], expect, "half")


# ================================================================================================ bit-exact against the restatement

@pytest.mark.parametrize("S", E.SECTION_COUNTS)
@pytest.mark.parametrize("path", PATHS)
def test_bit_exact_against_the_restatement(na, models, launches, twin, path, S):
    """Cascades of S sections on row 0 (LSTM) and row 4 (Standard) and one of another length on row 1, over calls of 1, 2, 7, 8, 9, 127,
    128, 129 and 300 samples -- the tile edge, and calls shorter than the pipeline is deep, with state carried between them.  Every row
    of every call is checked; the rows without an EQ carry the twin's bits."""
    calls = list(E.CALL_SIZES)
    x = signal(sum(calls), 2)
    yt = twin(x, calls, key="exact")
    b = make_batch(na, models)
    cascades = {0: E.cascade(S, 10), 4: E.cascade(S, 11), 1: E.cascade(S % 8 + 1, 12)}
    refs = {}
    for s, sec in cascades.items():
        b.SetStreamEq(s, sec, 0)
        refs[s] = E.EqRef()
        refs[s].set(sec)
        got = b.GetStreamEq(s)
        assert got == [dict(zip(E.FIELDS, t)) for t in E.tuples(sec)]
    info = b.GetEqInfo()
    assert (info["maxSections"], info["numEntries"]) == (8, 3) and info["deviceBytes"] >= 16 * (640 + 512), "two slots per row: 2 x 320 + 2 x 256 bytes"
    run, pos = Runner(b, path), 0
    before = launches()
    for n in calls:
        y = run.call(x[:, pos:pos + n])
        expect = yt[:, pos:pos + n].copy()
        for s, ref in refs.items():
            expect[s] = ref.run(yt[s, pos:pos + n])
        assert_rows(y, expect, (path, S, "call at", pos, "n", n))
        pos += n
    assert launches() - before == len(calls), "one launch per call, whatever n"
    b.close()


def _hook_batch(na, models, rows):
    b = na.Batch(0)
    assert b.AddStreams(models[LSTM], rows, doPrewarm=False) == 0
    b.EnableEqStage()
    return b


def _hook_run(b, x, calls):
    """the stage alone over x[rows, total] cut into `calls`: blocks with an odd row stride and a sentinel behind every row"""
    out, pos = [], 0
    for n in calls:
        block = np.full((x.shape[0], n + (3 if n % 2 == 0 else 4)), F(7.0))
        block[:, :n] = x[:, pos:pos + n]
        b.DebugRunEqStage(block, n)
        assert np.all(block[:, n:] == F(7.0)), "the stage wrote past the end of a row"
        out.append(block[:, :n].copy())
        pos += n
    return np.concatenate(out, axis=1)


def test_the_cut_into_calls_never_shows(na, models):
    """1000 samples in one call equal the same samples in ragged cuts and in calls of 1, bit for bit, and each the restatement."""
    total, rows = 1000, 4
    x = np.stack([E.noise(total, 300 + r, 0.5) for r in range(rows)])
    outs = []
    for calls in ([total], E.ragged(total), [1] * 40 + [total - 40]):
        b = _hook_batch(na, models, rows)
        for s, S in enumerate((1, 3, 8)):
            b.SetStreamEq(s, E.cascade(S, 20 + s), 0)
        outs.append(_hook_run(b, x, calls))
        b.close()
    expect = x.copy()
    for s, S in enumerate((1, 3, 8)):
        ref = E.EqRef()
        ref.set(E.cascade(S, 20 + s))
        expect[s] = ref.run(x[s])
    assert_rows(outs[0], expect, "one call")
    assert_rows(outs[1], expect, "ragged")
    assert_rows(outs[2], expect, "ones")


# ================================================================================================ more entries than a wave and than a workgroup

def test_more_entries_than_a_wave_and_than_a_workgroup(na, models, launches):
    """150 rows, 70 of them with an entry on scattered rows, section counts 1 .. 8, a third of them mid-fade (from flat, from a longer and
    from a shorter cascade, fades that end inside a call and fades that cross calls): every entry's row is exact, every row without an
    entry is untouched bit for bit -- NaN payloads, infinities and subnormals included."""
    rows, calls = 150, [130, 129, 300]
    rng = np.random.default_rng(7)
    picked = sorted(int(r) for r in rng.choice(rows, 70, replace=False))
    x = np.stack([E.noise(sum(calls), 700 + r, 0.3) for r in range(rows)])
    idle = [r for r in range(rows) if r not in picked]
    odd = np.array([0x7fc01234, 0xffc00001, 0x7f800000, 0xff800000, 0x00000001, 0x80000007, 0x7f7fffff, 0x80000000], np.uint32).view(np.float32)
    for j, r in enumerate(idle):
        x[r, j % 100:j % 100 + 8] = odd
    b = _hook_batch(na, models, rows)
    refs = {r: E.EqRef() for r in picked}
    S_of = {r: 1 + j % 8 for j, r in enumerate(picked)}
    out, pos = [], 0
    before = launches()
    for i, n in enumerate(calls):
        for j, r in enumerate(picked):
            if i == 0 and j % 3 != 2:
                op = (E.cascade(S_of[r], r), 0)
            elif i == 0:
                op = (E.cascade(S_of[r], r), (5, 200, 129)[j % 9 // 3])       # from flat
            elif i == 1 and j % 3 == 0:
                op = (E.cascade(1 + (S_of[r] + 3) % 8, r + 1), (1, 128, 400)[j % 9 // 3])  # to a longer or a shorter cascade
            elif i == 2 and j % 9 == 1:
                op = (None, 64)
            else:
                continue
            if refs[r].fading:
                with pytest.raises(na.NeuralAudioError, match="an EQ fade of stream %d is running" % r):
                    b.SetStreamEq(r, *op)
                continue
            b.SetStreamEq(r, *op)
            refs[r].set(*op)
        if i == 1:
            fading = [r for r in picked if refs[r].fading]
            assert len(fading) >= 20 and b.GetEqInfo()["numEntries"] == 70
        block = x[:, pos:pos + n]
        y = _hook_run(b, block, [n])
        expect = block.copy()
        for r in picked:
            expect[r] = refs[r].run(block[r])
            assert b.StreamEqFadeRemaining(r) == refs[r].remaining, r
        assert_rows(y, expect, ("call", i))
        out.append(y)
        pos += n
    assert launches() - before == len(calls)
    assert b.GetEqInfo()["numEntries"] == sum(ref.is_entry for ref in refs.values()) < 70
    b.close()


# ================================================================================================ fades

@pytest.mark.parametrize("N", E.FADES)
def test_fades(na, models, launches, twin, N):
    """flat -> EQ, EQ -> EQ with more and with fewer sections, EQ -> flat, each over N samples in calls of 128 (N = 200 crosses a call
    boundary): the restatement's bits; FadeRemaining counts down; a set call during a fade is refused; the entry retires and the
    launch counter stops with the last entry."""
    n, K = 128, 9
    x = signal(n * K, 3)
    yt = twin(x, [n] * K, key="fades")
    b = make_batch(na, models)
    steps = {0: E.cascade(3, 30), 2: E.cascade(8, 31), 4: E.cascade(1, 32), 6: None}
    refs = {0: E.EqRef(), 4: E.EqRef()}
    before = launches()
    ran = 0
    for k in range(K):
        if k in steps:
            for s, ref in refs.items():
                b.SetStreamEq(s, steps[k], N)
                ref.set(steps[k], N)
                assert b.StreamEqFadeRemaining(s) == (N if ref.is_entry else 0) and len(b.GetStreamEq(s)) == len(steps[k] or [])
        entries = sum(ref.is_entry for ref in refs.values())
        assert b.GetEqInfo()["numEntries"] == entries
        y = b.Process(np.ascontiguousarray(x[:, k * n:(k + 1) * n]))
        ran += 1 if entries else 0
        expect = yt[:, k * n:(k + 1) * n].copy()
        for s, ref in refs.items():
            expect[s] = ref.run(expect[s])
            assert b.StreamEqFadeRemaining(s) == ref.remaining == max(0, N - n if k in steps else 0), (k, s)
        assert_rows(y, expect, ("N", N, "call", k))
        if k in steps and N > n:
            with pytest.raises(na.NeuralAudioError, match="SetStreamEq: an EQ fade of stream 4 is running"):
                b.SetStreamEq(4, E.cascade(2, 33), 0)
    assert launches() - before == ran == (6 if N == 0 else (7 if N <= n else 8)), "the counter stops with the last entry"
    assert b.GetEqInfo()["numEntries"] == 0 and b.GetStreamEq(0) == []
    b.close()


# ================================================================================================ bad samples

def test_bad_samples(na, models):
    """NaN reads as 0, +-inf as +-1e18; the stream recovers: finite output afterwards, and the restatement's bits throughout."""
    total = 600
    x = np.stack([E.noise(total, 400 + r) for r in range(2)])
    x[0, 100:104] = [np.nan, np.inf, -np.inf, np.nan]
    x[1, 5] = np.inf
    x[1, 300:310] = -np.inf
    b = _hook_batch(na, models, 2)
    ident = dict(b0=1.0, b1=0.0, b2=0.0, a1=0.0, a2=0.0)
    cascades = {0: [ident], 1: E.cascade(3, 40)}
    expect = x.copy()
    for s, sec in cascades.items():
        b.SetStreamEq(s, sec, 0)
        ref = E.EqRef()
        ref.set(sec)
        expect[s] = ref.run(x[s])
    y = _hook_run(b, x, [128, 129, 343])
    b.close()
    assert_rows(y, expect, "bad samples")
    assert E.same_bits(y[0, 100:104], np.array([0.0, 1e18, -1e18, 0.0], F))
    # the stream recovers: finite output afterwards (how fast the 1e18 rings down is the cascade's own decay, not the stage's doing);
    # the identity section, which has no memory of its outputs, is back to the input at once
    assert np.all(np.isfinite(y[0])) and np.all(np.isfinite(y[1, 6:300])) and np.all(np.isfinite(y[1, 310:]))
    assert E.same_bits(y[0, 104:], x[0, 104:])


# ================================================================================================ rules and lifecycle

def test_rules(na, models):
    """Each refusal carries its text; park, remove and the park that ends a hand-over make the stream flat; an activated stream is
    flat; a broken batch refuses everything."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    b = make_batch(na, models, eq=False, out_stage=True)
    c3 = E.cascade(3, 50)
    for call in (lambda: b.SetStreamEq(0, c3), lambda: b.SetStreamEq(0, None), lambda: b.GetStreamEq(0), lambda: b.StreamEqFadeRemaining(0), lambda: b.GetEqInfo(),
                 lambda: b.DebugRunEqStage(np.zeros((ROWS, 8), F))):
        with pytest.raises(na.NeuralAudioError, match=r"eq stage not enabled \(NA_BatchEnableEqStage\)"):
            call()
    assert lib.NA_BatchGetStreamEq(b._h, 0, None, 0) < 0 and lib.NA_BatchStreamEqFadeRemaining(b._h, 0) < 0
    b.EnableEqStage()
    b.EnableEqStage()
    assert b.GetEqInfo()["numEntries"] == 0 and b.GetEqInfo()["maxSections"] == 8
    with pytest.raises(na.NeuralAudioError, match="SetStreamEq: stream 3 is parked"):
        b.SetStreamEq(3, c3)
    with pytest.raises(na.NeuralAudioError, match="SetStreamEq: stream 12 is not a live stream of the batch"):
        b.SetStreamEq(12, c3)
    with pytest.raises(na.NeuralAudioError, match="GetStreamEq: stream 12 is not a stream of the batch"):
        b.GetStreamEq(12)
    with pytest.raises(na.NeuralAudioError, match="StreamEqFadeRemaining: stream -1 is not a stream of the batch"):
        b.StreamEqFadeRemaining(-1)
    ok = dict(b0=1.0, b1=0.0, b2=0.0, a1=0.0, a2=0.0)
    for sections, fade, text in (([ok] * 9, 0, r"numSections must lie in \[0, 8\]"),
                                 ([ok, dict(ok, b1=float("nan"))], 0, "section 1: every coefficient must be finite"),
                                 ([dict(ok, a2=float("inf"))], 0, "section 0: every coefficient must be finite"),
                                 ([ok, ok, dict(ok, a2=1.0)], 0, r"section 2: must be stable \(\|a2\| < 1 and \|a1\| < 1 \+ a2\)"),
                                 ([ok, dict(ok, a2=0.5, a1=1.5)], 0, "section 1: must be stable"),
                                 ([ok, dict(ok, a2=-0.5, a1=-0.5)], 0, "section 1: must be stable"),
                                 ([ok], -1, r"fadeSamples must lie in \[0, 1 << 20\]"), ([ok], (1 << 20) + 1, r"fadeSamples must lie in \[0, 1 << 20\]")):
        with pytest.raises(na.NeuralAudioError, match="SetStreamEq: " + text):
            b.SetStreamEq(0, sections, fade)
    assert lib.NA_BatchSetStreamEq(b._h, 0, None, 3, 0) != 0 and "numSections" in capi.last_error()
    assert b.GetEqInfo()["numEntries"] == 0 and b.GetStreamEq(0) == [] and b.StreamEqFadeRemaining(0) == 0
    b.SetStreamEq(0, [dict(ok, a2=1.0 - 2.0 ** -40, a1=1.9)] * 8, 1 << 20)
    with pytest.raises(na.NeuralAudioError, match="SetStreamEq: an EQ fade of stream 0 is running"):
        b.SetStreamEq(0, None, 0)
    assert b.StreamEqFadeRemaining(0) == 1 << 20 and len(b.GetStreamEq(0)) == 8
    # the capacity of NA_BatchGetStreamEq bounds what it writes, not what it returns
    out = (capi.NA_EqSection * 8)()
    assert lib.NA_BatchGetStreamEq(b._h, 0, out, 2) == 8 and out[1].a1 == 1.9 and out[2].a1 == 0.0
    b.SetStreamEq(1, None, 64)  # (flat to flat: nothing)
    assert b.GetEqInfo()["numEntries"] == 1
    # park, remove and the end of a hand-over make the stream flat at once; an activated stream is flat
    for s in (1, 2, 4, 5):
        b.SetStreamEq(s, c3, 0)
    assert b.GetEqInfo()["numEntries"] == 5
    b.ParkStream(0)
    assert b.GetEqInfo()["numEntries"] == 4 and b.GetStreamEq(0) == [] and b.StreamEqFadeRemaining(0) == 0
    b.ActivateStream(0, 1.0)
    assert b.GetStreamEq(0) == []
    blob = b.SaveStreams([5])
    b.LoadStreams([4], blob)
    assert len(b.GetStreamEq(4)) == 3 and b.GetEqInfo()["numEntries"] == 4, "the EQ is not part of a snapshot"
    b.Handover(4, 6, 1.0, 64)
    x = signal(64, 7)
    y = b.Process(x)
    assert len(b.GetStreamEq(4)) == 3 and b.GetStreamEq(6) == [] and np.all(np.isfinite(y))
    b.Process(x)  # (parks row 4 in front of its launches)
    assert b.IsParked(4) and b.GetStreamEq(4) == [] and b.GetEqInfo()["numEntries"] == 3
    # the stage grows with the batch
    first = b.ReserveStreams(models[LSTM], 30)
    b.ActivateStream(first + 29, 1.0)
    b.SetStreamEq(first + 29, E.cascade(8, 51), 16)
    y = b.Process(signal(64, 8)[np.arange(b.NumStreams()) % ROWS])
    assert np.any(y[first + 29]) and np.all(np.isfinite(y)) and len(b.GetStreamEq(1)) == 3 and b.GetEqInfo()["numEntries"] == 4
    # a broken batch refuses everything
    b.SetWaitLimitMs(20.0)
    b.DebugStallDevice(80.0)
    with pytest.raises(na.NeuralAudioError, match="did not answer within"):
        b.Synchronize()
    assert b.IsBroken()
    for call in (lambda: b.SetStreamEq(1, c3), lambda: b.SetStreamEq(1, None), lambda: b.EnableEqStage(), lambda: b.DebugRunEqStage(np.zeros((b.NumStreams(), 8), F))):
        with pytest.raises(na.NeuralAudioError, match="broken"):
            call()
    b.close()


def test_remove_streams_drops_the_eq(na, models):
    b = na.Batch(0)
    assert b.AddStreams(models[LSTM], 4) == 0
    b.EnableEqStage()
    b.SetStreamEq(1, E.cascade(2, 60), 0)
    b.SetStreamEq(2, E.cascade(5, 61), 100)
    b.RemoveStreams(1, 1)
    assert b.GetEqInfo()["numEntries"] == 1
    assert b.AddStreams(models[LSTM], 1) == 1 and b.GetStreamEq(1) == [] and len(b.GetStreamEq(2)) == 5 and b.StreamEqFadeRemaining(2) == 100
    b.close()


def test_set_calls_and_processing_with_entries_are_real_time_safe(na, models):
    """NA_DebugDeviceResourceCalls stays where it is across set calls -- new cascades, coefficient changes, fades, fades to flat -- and 21
    processing calls with entries, over the blocking and the pipelined host path and device pointers (after three warm calls of each,
    which size the staging block and the pipeline slots)."""
    import torch
    from neuralaudio_amd import capi
    lib = capi.load_library()
    dev = torch.device("cuda", 0)
    b = make_batch(na, models)
    n = 128
    x = signal(n, 9)
    dx, dy = torch.from_numpy(x).to(dev), torch.zeros(ROWS, n, device=dev)
    torch.cuda.synchronize(dev)

    def three():
        b.Process(x)
        b.Collect(b.Submit(x))
        b.ProcessDevice(dx.data_ptr(), dy.data_ptr(), n, n, n)
        b.Synchronize()

    b.SetStreamEq(0, E.cascade(3, 70), 0)
    for _ in range(3):
        three()
    before = lib.NA_DebugDeviceResourceCalls()
    b.SetStreamEq(4, E.cascade(8, 71), 300)
    b.SetStreamEq(1, E.cascade(1, 72), 0)
    for i in range(7):
        three()
        if i == 2:
            b.SetStreamEq(0, E.cascade(5, 73), 0)
            b.SetStreamEq(1, None, 200)
        if i == 4:
            b.SetStreamEq(5, E.cascade(2, 74), 64)
            b.SetStreamEq(4, None, 0)
    assert b.GetStreamEq(1) == [] and b.GetStreamEq(4) == [] and b.GetEqInfo()["numEntries"] == 2
    assert lib.NA_DebugDeviceResourceCalls() == before
    b.close()


# ================================================================================================ order with the other stages

def _chain(x_row, yt_row, gate_p, sections, taps, gain, eq_first=True):
    """gate -> EQ -> cabinet -> output gain on one row: the composition of the four restatements (eq_first = False: the cabinet in
    front of the EQ, the order the library must NOT have)"""
    g = G.GateRef(gate_p, True).run(x_row)
    y = (yt_row * g).astype(F)
    ref = E.EqRef()
    ref.set(sections)
    y = CAB.sequential_f32(taps, ref.run(y)) if eq_first else ref.run(CAB.sequential_f32(taps, y))
    return (y * F(gain)).astype(F), g


@pytest.mark.parametrize("variant", ["plain", "resample", "in-place"])
def test_gate_eq_cabinet_and_gain_compose_in_that_order(na, models, twin, variant):
    """Rows 0 and 4 carry all four stages: a gate, a 3-section EQ, the IR {1, 0.5} -- fl(y[t] + 0.5 * y[t-1]) by the cabinet's own rule:
    one rounding, so the order of EQ and cabinet shows in the bits -- and an output gain of 0.5.  The row equals the composition
    gate -> EQ -> cabinet -> gain of the four restatements on the twin's row; also on a 44.1 kHz resampling batch, where the stages act
    on the external-rate rows, and in place, with input rows = output rows."""
    import torch
    dev = torch.device("cuda", 0)
    calls = [128, 129, 300, 443]
    total = sum(calls)
    resample = 44100 if variant == "resample" else None
    x = np.stack([G.gate_signal(900 + r, total) for r in range(ROWS)])
    yt = twin(x, calls, resample=resample, key="order")
    b = make_batch(na, models, resample=resample, out_stage=True)
    b.EnableCabinetStage(64)
    b.EnableGateStage()
    taps = np.array([1.0, 0.5], F)
    ir = b.LoadIR(taps)
    p = G.params(floorGain=0.1)
    sections = {0: E.cascade(3, 80), 4: E.cascade(3, 81)}
    for s in (0, 4):
        b.SetStreamGate(s, p, True)
        b.SetStreamEq(s, sections[s], 0)
        b.SetStreamIR(s, ir, 0)
        b.SetStreamGain(s, 0.5, 0)
    b.SetStreamEq(5, E.cascade(8, 82), 0)  # (an EQ alone)
    y, pos = [], 0
    for n in calls:
        xs = np.ascontiguousarray(x[:, pos:pos + n])
        if variant == "in-place":
            buf = torch.from_numpy(xs).to(dev)
            torch.cuda.synchronize(dev)
            b.ProcessDevice(buf.data_ptr(), buf.data_ptr(), n, n, n)
            b.Synchronize()
            rows = buf.cpu().numpy()
            rows[list(set(range(ROWS)) - set(LIVE))] = 0.0  # (device rows of parked streams are left alone: here, the input)
        else:
            rows = b.Process(xs)
        y.append(rows)
        pos += n
    y = np.concatenate(y, axis=1)
    b.close()
    expect = yt.copy()
    for s in (0, 4):
        expect[s], g = _chain(x[s], yt[s], p, sections[s], taps, 0.5)
        assert np.any(g == 1.0) and np.any(g < 1.0)
        wrong, _ = _chain(x[s], yt[s], p, sections[s], taps, 0.5, eq_first=False)
        assert not E.same_bits(wrong, expect[s]), "the test can tell the two orders apart"
    ref = E.EqRef()
    ref.set(E.cascade(8, 82))
    expect[5] = ref.run(yt[5])
    assert_rows(y, expect, variant)
