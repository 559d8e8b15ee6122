"""GPU tests of the modulation stage (NA_BatchEnableModStage / SetStreamMod, csrc/mod_stage.h): per-stream chorus,
flanger, vibrato and tremolo behind the compressor stage and in front of the delay stage.

The contract states every f32 operation and its order, so the expected value is the numpy float32 restatement of tests/mod_cases.py
and every comparison is on the bits.  Part 1 drives the stage through its hook (NA_DebugRunModStage) on rows that stand in for model
outputs, on streams of the smallest committed model that never run; part 2 runs the twelve-row batch of tests/handover_cases.py beside
its twin without the stage."""
import os

import numpy as np
import pytest

import compressor_cases as CK
import delay_cases as D
import handover_cases as H
import mod_cases as K

FORCED = bool(os.environ.get("NA_WN_KERNEL") or os.environ.get("NA_WN_PACK") or os.environ.get("NA_WN_SPEC") or os.environ.get("NA_SP_T")
              or os.environ.get("NA_SP_GEN") or os.environ.get("NA_WN_PAD"))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(FORCED, reason="forced kernel family")]

F = np.float32
NOT_ENABLED = r"modulation stage not enabled \(NA_BatchEnableModStage\)"


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
    return capi.load_library().NA_DebugModLaunches


def odd(n):
    return n + 3


def pieces(calls):
    """launches of calls with an entry: one per piece of 2048 samples"""
    return sum((n + K.PIECE - 1) // K.PIECE for n in calls)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_same(y, e, what=()):
    for row in range(y.shape[0]):
        diff = np.flatnonzero(bits(y[row]) != bits(e[row]))
        assert len(diff) == 0, what + ("row", row, "first at", int(diff[0]), float(y[row][diff[0]]), float(e[row][diff[0]]), "of", len(diff))


def expect_rows(refs, x, calls):
    """the restatements of `refs` {row: ModRef} over x cut into `calls`; the other rows keep their bits"""
    e, pos = x.copy(), 0
    for n in calls:
        for row, ref in refs.items():
            e[row, pos:pos + n] = ref.run(x[row, pos:pos + n])
        pos += n
    return e


class HookBatch:
    """`rows` rows (BossWN-nano streams that never run) with the stage enabled: the hook runs the stage on host rows."""

    def __init__(self, na, nano, rows, max_delay):
        self.b = na.Batch(0)
        assert self.b.AddStreams(nano, rows, doPrewarm=False) == 0
        self.b.EnableModStage(max_delay)
        self.rows = rows

    def set(self, refs, row, p, fade=0):
        self.b.SetStreamMod(row, p, fade)
        assert refs.setdefault(row, K.ModRef()).set(p, fade) is True

    def run(self, x, calls=None, stride=lambda n: n):
        """the stage over x[rows, total], cut into `calls`; every call's block has rows stride(n) floats apart"""
        calls = [x.shape[1]] if calls is None else calls
        assert sum(calls) == x.shape[1]
        out, pos = [], 0
        for n in calls:
            block = np.full((self.rows, stride(n)), F(7.0))
            block[:, :n] = x[:, pos:pos + n]
            self.b.DebugRunModStage(block, n)
            assert np.all(block[:, n:] == F(7.0)), "the stage wrote past the end of a row"
            out.append(block[:, :n].copy())
            pos += n
        return np.concatenate(out, axis=1)

    def close(self):
        self.b.close()


def noise_rows(rows, total, seed=0):
    return np.stack([K.signal(seed + r, total) for r in range(rows)])


# ================================================================================================ 1: through the hook

def test_the_known_answers(na, models, launches):
    """depth 0, base 5, one voice of gain 1, wet 1, dry 0, fb 0.5: an impulse gives exact powers of two at the multiples of 5, down
    through the subnormals to 2^-149 and then +0 -- a build that flushes to zero ends at 2^-126.  base 5.5, fb 0: exactly 0.5 at 5 and
    at 6.  td 1, wet 0, dry 1 on a constant 1: y = fl(1 - s_0).  wet 0, dry 1, td 0: the row is x' bit for bit.  The fifth row has no
    entry and keeps its bits, NaN included."""
    n = 5 * 152
    hb = HookBatch(na, models[H.NANO], 5, 512)
    x = np.zeros((5, n), F)
    x[0, 0] = x[1, 0] = 1.0
    x[2] = 1.0
    x[3], x[4] = K.signal(3, n), K.signal(4, n)
    hb.b.SetStreamMod(0, K.params(5.0, 0.0, K.phase_inc(3.0), K.SINE, 1, feedback=0.5, wet=1.0, dry=0.0))
    hb.b.SetStreamMod(1, K.params(5.5, 0.0, 0, K.TRIANGLE, 1, wet=1.0, dry=0.0))
    hb.b.SetStreamMod(2, K.params(9.0, 2.0, K.phase_inc(100.0), K.SINE, 1, wet=0.0, dry=1.0, tremolo=1.0))
    hb.b.SetStreamMod(3, dict(K.chorus(), wet=0.0, dry=1.0))
    before = launches()
    y = hb.run(x, [300, n - 300], stride=odd)
    assert launches() - before == 2
    e0 = np.zeros(n, F)
    m = np.arange(1, 152)
    e0[5 * m] = np.ldexp(1.0, -(m - 1)).astype(F)
    assert e0[5 * 150] == 2.0 ** -149 and e0[5 * 151] == 0.0 and 0 < e0[5 * 130] < np.finfo(F).tiny
    e1 = np.zeros(n, F)
    e1[5] = e1[6] = 0.5
    s0 = K.shape_of(K.SINE, K.tri_of(np.arange(n, dtype=np.uint64) * np.uint64(K.phase_inc(100.0))))
    assert_same(y, np.stack([e0, e1, (F(1.0) - s0).astype(F), K.x_prime(x[3]), x[4]]))
    hb.close()


def test_a_three_voice_chorus_without_feedback(na, models, launches):
    """Three voices a third of a cycle apart around 7 ms, both shapes, one call of 3000 samples (two pieces) against the restatement:
    the feedback-free form, every sample independent of the others of its piece."""
    rows, total = 3, 3000
    hb = HookBatch(na, models[H.NANO], rows, 512)
    info = hb.b.GetModInfo()
    assert (info["maxDelaySamples"], info["ringSamples"], info["pieceSamples"], info["numMods"]) == (512, 4096, 2048, 0)
    assert info["deviceBytes"] >= 16 * 4096 * 4
    x = noise_rows(rows, total, 10)
    refs = {}
    hb.set(refs, 0, K.chorus(rate_hz=30.0))
    hb.set(refs, 1, K.chorus(shape=K.TRIANGLE, rate_hz=7.0, depth=100.5, base=300.25))
    assert hb.b.GetStreamMod(0) == K.chorus(rate_hz=30.0) and hb.b.GetStreamMod(2) is None and hb.b.GetModInfo()["numMods"] == 2
    before = launches()
    y = hb.run(x, [total], stride=odd)
    assert launches() - before == 2, "one launch per piece"
    assert_same(y, expect_rows(refs, x, [total]))
    assert not np.array_equal(bits(y[0]), bits(K.x_prime(x[0])))
    hb.close()


@pytest.mark.parametrize("base,depth", K.FLANGERS)
def test_flangers_at_every_chunk_length(na, models, base, depth):
    """fb = +0.7 and -0.7 at base 2 (the serial extreme: chunks of 1), 5.5 (4), 48 (47), 70 + 30 (69) and 300 + 60 (capped by the
    workgroup's 256 lanes); rows 2 and 3 fade the same settings in from none over 100 samples (the ramp may undershoot base: the - 1
    of the chunk rule) and row 0 glides to a longer base in the second call."""
    hb = HookBatch(na, models[H.NANO], 4, 512)
    x = noise_rows(4, 900, 20)
    refs = {}
    hb.set(refs, 0, K.flanger(base, depth, 0.7))
    hb.set(refs, 1, K.flanger(base, depth, -0.7, shape=K.SINE))
    hb.set(refs, 2, K.flanger(base, depth, 0.7), 100)
    hb.set(refs, 3, K.flanger(base, depth, -0.7, rate_hz=300.0), 100)
    y0 = hb.run(x[:, :450], stride=odd)
    e0 = expect_rows(refs, x[:, :450], [450])
    hb.set(refs, 0, K.flanger(base + 1.75, depth, 0.5), 200)
    y1 = hb.run(x[:, 450:])
    assert_same(np.concatenate([y0, y1], axis=1), np.concatenate([e0, expect_rows(refs, x[:, 450:], [450])], axis=1), (base, depth))
    hb.close()


def test_the_cut_into_calls_never_shows(na, models, launches):
    """A chorus, two flangers and a tremolo: one call, and cuts of 1, 7, 64, 65, 128 and one sample more than a piece, with an odd
    stride; both equal the restatement (which is evaluated in one run), so the cut does not show in the bits."""
    total = sum(K.CUTS)
    ps = [K.chorus(rate_hz=11.0), K.flanger(5.5, 4.25, 0.7), K.flanger(48.0, 20.0, -0.7, shape=K.SINE),
          K.params(24.0, 0.0, K.phase_inc(3.0), K.SINE, 1, wet=0.0, dry=1.0, tremolo=1.0)]
    x = noise_rows(4, total, 30)
    e = K.run_cuts(ps, x, [total])
    for calls, stride in (([total], lambda n: n), (K.CUTS, odd)):
        hb = HookBatch(na, models[H.NANO], 4, 512)
        for row, p in enumerate(ps):
            hb.b.SetStreamMod(row, p)
        before = launches()
        y = hb.run(x, calls, stride)
        assert launches() - before == pieces(calls)
        assert_same(y, e, (len(calls),))
        hb.close()


def test_the_ring_wraps_at_every_offset(na, models):
    """maxDelaySamples = 64: a ring of 4096 and the longest reach the line allows (62).  3 * 4096 + 1500 samples in calls of odd
    lengths, so the ring's wrap falls inside windows and pieces at many offsets; a flanger (chunks of 39) and a two-voice vibrato."""
    hb = HookBatch(na, models[H.NANO], 3, 64)
    assert hb.b.GetModInfo()["ringSamples"] == 4096
    total = 3 * 4096 + 1500
    calls = D.cuts(total, [2049, 777, 1, 1301, 63, 2048, 129])
    x = noise_rows(3, total, 40)
    refs = {}
    hb.set(refs, 0, K.flanger(40.0, 22.0, 0.7, rate_hz=5.0))
    hb.set(refs, 2, K.params(30.0, 32.0, K.phase_inc(2.5), K.SINE, 2, (0, 0x80000000, 0, 0), [0.6, 0.4, 0, 0], 0.0, 1.0, 0.0))
    y = hb.run(x, calls, stride=odd)
    assert_same(y, expect_rows(refs, x, calls))
    hb.close()


def test_one_five_and_seventeen_entries(na, models, launches):
    """A workgroup owns one entry, so every count is a whole number of workgroups; 1, 5 and 17 entries of an 18-row batch (its tables
    hold 18), each with its own setting -- choruses and flangers of both signs --, the rows without an entry keep their bits, and an
    entry's bits do not depend on the others: rows 0 .. 4 go on from call to call."""
    rows, n = 18, 333
    hb = HookBatch(na, models[H.NANO], rows, 256)
    x = noise_rows(rows, 3 * n, 50)
    refs, out, exp = {}, [], []
    for k, upto in enumerate((1, 5, 17)):
        for row in range(upto):
            if row not in refs:
                p = K.chorus(base=40.0 + 3.5 * row, depth=20.0 + row, rate_hz=3.0 + row) if row % 3 == 0 else K.flanger(2.0 + 2.25 * row, 1.5 * row, (-1) ** row * 0.05 * row)
                hb.set(refs, row, p)
        assert hb.b.GetModInfo()["numMods"] == upto
        before = launches()
        out.append(hb.run(x[:, k * n:(k + 1) * n], stride=odd))
        assert launches() - before == 1
        exp.append(expect_rows(refs, x[:, k * n:(k + 1) * n], [n]))
    assert_same(np.concatenate(out, axis=1), np.concatenate(exp, axis=1))
    hb.close()


def test_fades_and_a_retired_loud_line(na, models, launches):
    """None -> A -> B -> none on row 0 with base, depth, rate and shape changing and voices coming and going; a set call during a fade
    is refused with the samples left, a changed voicePhase of a sounding voice by name; the call in which the fade to none ends leaves
    the rest of its row untouched and retires the entry; row 1 runs a loud line (inputs of 1e20 are clamped to 1e18, feedback 0.9),
    is removed at once and set again: the new entry reads +0, not what the ring holds."""
    hb = HookBatch(na, models[H.NANO], 3, 128)
    x = noise_rows(3, 1400, 60)
    with np.errstate(over="ignore"):
        x[1, :500] *= F(1e20)
    a = K.params(20.5, 10.5, K.phase_inc(40.0), K.TRIANGLE, 2, (0, 0x80000000, 0, 0), [0.75, 0.0, 0, 0], 0.9, 0.8, 1.0)
    b = K.params(60.0, 66.0, K.phase_inc(90.0), K.SINE, 3, (0, 0x12345678, 0x9ABCDEF0, 0), [0.5, 0.5, -0.5, 0], -0.6, 1.0, 0.5, 0.3)
    refs, out, exp = {}, [], []

    def call(lo, hi):
        out.append(hb.run(x[:, lo:hi], stride=odd))
        exp.append(expect_rows({r: ref for r, ref in refs.items() if ref.has}, x[:, lo:hi], [hi - lo]))

    hb.set(refs, 0, a, 100)
    hb.set(refs, 1, K.flanger(3.0, 2.0, 0.9))
    call(0, 64)
    assert hb.b.StreamModFadeRemaining(0) == 36
    with pytest.raises(na.NeuralAudioError, match=r"SetStreamMod: a modulation fade of stream 0 is running \(36 samples left\)"):
        hb.b.SetStreamMod(0, b, 10)
    with pytest.raises(na.NeuralAudioError, match=r"SetStreamMod: a modulation fade of stream 0 is running \(36 samples left\)"):
        hb.b.SetStreamMod(0, None, 0)
    call(64, 300)
    with pytest.raises(na.NeuralAudioError, match=r"SetStreamMod: voicePhase\[0\] of a sounding voice must not change \(stream 0\)"):
        hb.b.SetStreamMod(0, dict(b, voicePhase=[1, 0x12345678, 0x9ABCDEF0, 0]))
    hb.set(refs, 0, b, 300)  # (voice 1 is silent in A: its phase may change)
    call(300, 500)
    hb.set(refs, 1, None)     # the loud line retires at once ...
    assert hb.b.GetModInfo()["numMods"] == 1 and hb.b.GetStreamMod(1) is None
    hb.set(refs, 1, K.params(3.0, 2.0, K.phase_inc(9.0), K.SINE, 1, wet=1.0, dry=0.0))  # ... and a new entry starts on the same ring
    call(500, 700)
    assert np.all(np.abs(out[-1][1][:3]) == 0.0) and np.max(np.abs(out[-1][1])) < 10.0, "nothing of the loud line leaks"
    hb.set(refs, 0, None, 70)
    assert hb.b.GetStreamMod(0) is None and hb.b.StreamModFadeRemaining(0) == 70 and hb.b.GetModInfo()["numMods"] == 2
    before = launches()
    call(700, 1000)
    assert launches() - before == 1 and hb.b.GetModInfo()["numMods"] == 1 and hb.b.StreamModFadeRemaining(0) == 0
    assert np.array_equal(bits(out[-1][0][70:]), bits(x[0, 770:1000])), "the retiring call leaves the rest of its row untouched"
    call(1000, 1400)
    assert_same(np.concatenate(out, axis=1), np.concatenate(exp, axis=1))
    hb.close()


# ================================================================================================ 2: in the batch

def run_batch(na, models, x, calls, ops, path="process", prepare=None):
    """The batch under test through `path`, call by call; ops: {call index: [(stream, params or None, N)]}.  Returns its rows."""
    b = H.make_batch(na, models, stage=False)
    b.EnableModStage(1024)
    if prepare:
        prepare(b)
    runner, out, pos = H.Runner(na, b, path), [], 0
    try:
        for i, n in enumerate(calls):
            for s, p, N in ops.get(i, ()):
                b.SetStreamMod(s, p, N)
            out.append(runner.call(x[:, pos:pos + n]))
            pos += n
    finally:
        runner.close()
        b.close()
    return np.concatenate(out, axis=1)


def twin_rows(na, models, x, calls):
    return np.concatenate(H.run_twin(na, models, x, calls, {}), axis=1)


def test_off_is_off(na, models, launches):
    """The stage is enabled and no stream has an entry: every path gives the twin's bits and launches none of the stage's kernels, and
    512 A1 Standard streams on device pointers use the half-batch launches exactly where the batch without the stage does."""
    import torch
    calls = [128, 17, 300]
    x = H.signal(sum(calls), 31)
    yt = twin_rows(na, models, x, calls)
    before = launches()
    for path in ("process", "submit", "device", "device-odd"):
        assert np.array_equal(run_batch(na, models, x, calls, {}, path), yt), path
    dev = torch.device("cuda", 0)
    S, n = 512, 128
    dx = torch.from_numpy(np.stack([H.noise(3 * n, 300 + r) for r in range(4)])[np.arange(S) % 4]).to(dev)
    torch.cuda.synchronize(dev)
    halves, outs = {}, {}
    for stage in (True, False):
        b = na.Batch(0)
        assert b.ReserveStreams(models[H.STD], S) == 0
        for s in range(S):
            b.ActivateStream(s, 1.0)
        if stage:
            b.EnableModStage(4096)
        dy = torch.zeros(S, 3 * n, device=dev)
        for k in range(3):
            b.ProcessDevice(dx.data_ptr() + 4 * k * n, dy.data_ptr() + 4 * k * n, n, 3 * n, 3 * n)
            b.Synchronize()
            halves[(stage, k)] = b.UsesHalfLaunches()
        outs[stage] = dy.cpu().numpy()
        b.close()
    assert launches() == before, "NA_DebugModLaunches stays where it was"
    assert [halves[(True, k)] for k in range(3)] == [halves[(False, k)] for k in range(3)]
    assert np.array_equal(outs[True], outs[False]) and np.any(outs[True])


MODS = {0: K.chorus(rate_hz=9.0), 4: K.flanger(48.0, 20.0, 0.7), 8: K.flanger(2.0, 3.0, -0.7, shape=K.SINE),
        9: K.params(30.0, 10.0, K.phase_inc(6.0), K.SINE, 1, wet=0.5, dry=1.0, tremolo=0.8)}
FAMILY = {}


@pytest.mark.parametrize("path", ["process", "device", "device-odd"])
def test_mods_on_one_stream_of_each_family(na, models, launches, path):
    """Entries on rows 0 (packed nano), 4 (Standard), 8 and 9 (LSTM) from the second call on, through the blocking host path and device
    pointers with aligned and odd row strides (unaligned rows); calls around the workgroup's width and one longer than a piece.  Every
    row of every call: the restatement on the twin's row, or the twin's bits."""
    calls = list(H.RAGGED) + [255, 256, 257, 2049]
    x = H.signal(sum(calls), 32)
    if "twin" not in FAMILY:  # (the twin and the restatement on it: computed once, shared by the three paths)
        yt = twin_rows(na, models, x, calls)
        refs = {s: K.ModRef() for s in MODS}
        for s, p in MODS.items():
            refs[s].set(p, 0)
        e = yt.copy()
        e[:, calls[0]:] = expect_rows(refs, yt[:, calls[0]:], calls[1:])
        FAMILY["twin"], FAMILY["expected"] = yt, e
    yt, e = FAMILY["twin"], FAMILY["expected"]
    before = launches()
    y = run_batch(na, models, x, calls, {1: [(s, p, 0) for s, p in MODS.items()]}, path)
    assert launches() - before == pieces(calls[1:])
    assert_same(y, e, (path,))
    assert all(not np.array_equal(y[s], yt[s]) for s in MODS)


def test_in_place(na, models):
    """NA_BatchProcessDevice with dIn == dOut on streams with an entry: the bits are those of separate buffers."""
    import torch
    dev = torch.device("cuda", 0)
    calls = [128, 300, 129]
    x = H.signal(sum(calls), 33)
    outs = {}
    for in_place in (False, True):
        b = H.make_batch(na, models, stage=False)
        b.EnableModStage(1024)
        for s, p in MODS.items():
            b.SetStreamMod(s, p, 100)
        y, pos = [], 0
        for n in calls:
            buf = torch.from_numpy(np.ascontiguousarray(x[:, pos:pos + n])).to(dev)
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
    assert np.array_equal(bits(outs[True]), bits(outs[False])) and np.any(outs[True][4])


def test_the_order_is_compressor_modulation_delay(na, models):
    """Row 4 gets a compressor in front of call 1, a modulation in front of call 2 and a delay in front of call 3: the row equals the
    three restatements composed in chain order on the twin's row, and differs from the composition with modulation and delay swapped."""
    calls = [128, 100, 300, 257, 300]
    x = H.signal(sum(calls), 34)
    yts = H.run_twin(na, models, x, calls, {})
    cp = CK.params(0.3, 0.05, threshold_db=-40.0, ratio=4.0, knee_db=6.0, makeup_db=6.0)
    mp = K.flanger(48.0, 20.0, 0.7, rate_hz=20.0)
    dp = D.filtered(90, 0.7)
    b = H.make_batch(na, models, stage=False)
    b.EnableCompressorStage()
    b.EnableModStage(512)
    b.EnableDelayStage(300)
    comp, mod, delay = CK.CompRef(), K.ModRef(), D.DelayRef()
    swapped_mod, swapped_delay = K.ModRef(), D.DelayRef()
    pos, differs = 0, False
    for i, n in enumerate(calls):
        if i == 1:
            b.SetStreamCompressor(4, cp, 0)
            comp.set(cp, 0)
        if i == 2:
            b.SetStreamMod(4, mp, 0)
            mod.set(mp, 0)
            swapped_mod.set(mp, 0)
        if i == 3:
            b.SetStreamDelay(4, dp, 0)
            delay.set(dp)
            swapped_delay.set(dp)
        y = b.Process(np.ascontiguousarray(x[:, pos:pos + n]))
        z = yts[i][4]
        if i >= 1:
            z = (z * comp.run(z)).astype(F)
        c = z
        if i >= 2:
            z = mod.run(z)
        if i >= 3:
            z = delay.process(z)
            differs = differs or not np.array_equal(bits(swapped_mod.run(swapped_delay.process(c))), bits(z))
        elif i >= 2:
            swapped_mod.run(c)
        assert np.array_equal(bits(y[4]), bits(z)), (i, int(np.flatnonzero(bits(y[4]) != bits(z))[0]))
        for s in (0, 1, 5, 8, 9):
            assert np.array_equal(y[s], yts[i][s]), (i, s)
        pos += n
    b.close()
    assert differs, "the test can tell the two orders apart"


def test_rules(na, models):
    """Each refusal carries its text; park, activate, remove and the park that ends a hand-over drop the entry; a larger maximum is
    refused while a stream has an entry; entries are not part of a snapshot; the stage grows with the batch and keeps a playing line."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    b = H.make_batch(na, models, stage=True)  # (with the output stage, for the hand-over)
    p = K.chorus()
    for call in (lambda: b.SetStreamMod(0, p), lambda: b.SetStreamMod(0, None), lambda: b.GetStreamMod(0), lambda: b.StreamModFadeRemaining(0),
                 lambda: b.GetModInfo(), lambda: b.DebugRunModStage(np.zeros((H.ROWS, 8), F))):
        with pytest.raises(na.NeuralAudioError, match=NOT_ENABLED):
            call()
    assert lib.NA_BatchGetStreamMod(b._h, 0, None) < 0 and lib.NA_BatchStreamModFadeRemaining(b._h, 0) < 0
    for bad in (7, 4097, -5):
        with pytest.raises(na.NeuralAudioError, match=r"EnableModStage: maxDelaySamples must lie in \[8, 4096\]"):
            b.EnableModStage(bad)
    b.EnableModStage(1000)
    b.EnableModStage(1000)
    b.EnableModStage(10)  # idempotent for an equal or smaller maximum
    info = b.GetModInfo()
    assert (info["maxDelaySamples"], info["ringSamples"], info["pieceSamples"], info["numMods"]) == (1000, 4096, 2048, 0)
    with pytest.raises(na.NeuralAudioError, match="SetStreamMod: stream 2 is parked"):
        b.SetStreamMod(2, p)
    with pytest.raises(na.NeuralAudioError, match="SetStreamMod: stream 12 is not a live stream of the batch"):
        b.SetStreamMod(12, p)
    with pytest.raises(na.NeuralAudioError, match="GetStreamMod: stream 12 is not a stream of the batch"):
        b.GetStreamMod(12)
    with pytest.raises(na.NeuralAudioError, match="StreamModFadeRemaining: stream -1 is not a stream of the batch"):
        b.StreamModFadeRemaining(-1)
    nan, inf = float("nan"), float("inf")
    for change, text in ((dict(baseSamples=1.5), "baseSamples must be finite and at least 2"), (dict(baseSamples=nan), "baseSamples must be finite and at least 2"),
                         (dict(depthSamples=-1.0), "depthSamples must be finite and at least 0"),
                         (dict(baseSamples=900.0), r"baseSamples \+ depthSamples must be at most maxDelaySamples - 2 \(maxDelaySamples = 1000\)"),
                         (dict(shape=2), "shape must be NA_MOD_TRIANGLE or NA_MOD_SINE"), (dict(numVoices=0), r"numVoices must lie in \[1, 4\]"),
                         (dict(numVoices=5), r"numVoices must lie in \[1, 4\]"), (dict(voiceGain=[0.1, -4.5, 0.1, 0.0]), r"voiceGain\[1\] must be finite and at most 4 in magnitude"),
                         (dict(feedback=0.96), r"feedback must lie in \[-0.95, 0.95\]"), (dict(feedback=nan), r"feedback must lie in \[-0.95, 0.95\]"),
                         (dict(wet=inf), "wet must be finite and at most 1e6 in magnitude"), (dict(dry=-2e6), "dry must be finite and at most 1e6 in magnitude"),
                         (dict(tremoloDepth=1.01), r"tremoloDepth must lie in \[0, 1\]"), (dict(tremoloDepth=nan), r"tremoloDepth must lie in \[0, 1\]")):
        with pytest.raises(na.NeuralAudioError, match="SetStreamMod: " + text):
            b.SetStreamMod(0, dict(p, **change))
    for fade in (-1, (1 << 20) + 1):
        with pytest.raises(na.NeuralAudioError, match=r"SetStreamMod: fadeSamples must lie in \[0, 1 << 20\]"):
            b.SetStreamMod(0, p, fade)
    assert b.GetModInfo()["numMods"] == 0 and b.GetStreamMod(0) is None
    b.SetStreamMod(1, None)  # (no entry: nothing to take away)
    b.SetStreamMod(0, p, 1 << 20)
    with pytest.raises(na.NeuralAudioError, match="a larger maxDelaySamples is refused while a stream has a modulation"):
        b.EnableModStage(2000)
    assert b.StreamModFadeRemaining(0) == 1 << 20 and b.GetStreamMod(0) == p and b.StreamModFadeRemaining(1) == 0
    # park, remove and the end of a hand-over drop the entry at once; an activated stream has none
    for s in (1, 4, 5, 8):
        b.SetStreamMod(s, p, 0 if s != 5 else 300)
    assert b.GetModInfo()["numMods"] == 5
    b.ParkStream(0)
    assert b.GetModInfo()["numMods"] == 4 and b.GetStreamMod(0) is None and b.StreamModFadeRemaining(0) == 0
    b.ActivateStream(0, 1.0)
    assert b.GetStreamMod(0) is None
    blob = b.SaveStreams([5])
    b.LoadStreams([4], blob)
    assert b.GetStreamMod(4) == p and b.StreamModFadeRemaining(4) == 0 and b.GetModInfo()["numMods"] == 4, "entries are not part of a snapshot"
    b.Handover(4, 6, 1.0, 64)
    x = H.signal(64, 35)
    b.Process(x)
    assert b.GetStreamMod(4) is not None and b.GetStreamMod(6) is None
    b.Process(x)  # (parks row 4 in front of its launches)
    assert b.IsParked(4) and b.GetStreamMod(4) is None and b.GetModInfo()["numMods"] == 3
    for s in (1, 5, 8):
        b.ParkStream(s)
    b.EnableModStage(4096)
    assert b.GetModInfo()["ringSamples"] == 8192 and b.GetModInfo()["numMods"] == 0
    b.close()
    # RemoveStreams drops the entry; a recycled id has none
    b = na.Batch(0)
    assert b.AddStreams(models[H.LSTM], 4) == 0
    b.EnableModStage(300)
    b.SetStreamMod(1, K.flanger(10.0, 5.0, 0.5))
    b.SetStreamMod(2, K.flanger(20.0, 5.0, 0.5), 500)
    b.RemoveStreams(1, 1)
    assert b.GetModInfo()["numMods"] == 1
    assert b.AddStreams(models[H.LSTM], 1) == 1 and b.GetStreamMod(1) is None and b.GetStreamMod(2) is not None
    b.close()


def test_growth_keeps_the_lines(na, models):
    """Four Standard streams, a flanger on row 1, two calls; sixteen more streams take the rows past the stage's first capacity of 16,
    so its rings move; two more calls.  Row 1 is the restatement on the whole history (row 0 runs the same input without an entry)."""
    n = 128
    x = np.stack([H.noise(4 * n, 3300 + r) for r in range(20)])
    x[1] = x[0]
    b = na.Batch(0)
    assert b.AddStreams(models[H.STD], 4) == 0
    b.EnableModStage(300)
    p = K.flanger(150.0, 100.0, 0.8, rate_hz=4.0)
    b.SetStreamMod(1, p)
    before = b.GetModInfo()["deviceBytes"]
    out = []
    for k in range(4):
        if k == 2:
            assert b.AddStreams(models[H.STD], 16) == 4
            assert b.GetModInfo()["deviceBytes"] > before
        out.append(b.Process(x[:b.NumStreams(), k * n:(k + 1) * n])[:4])
    y = np.concatenate(out, axis=1)
    ref = K.ModRef()
    ref.set(p, 0)
    e = ref.run(y[0])
    assert np.array_equal(bits(y[1]), bits(e)), int(np.flatnonzero(bits(y[1]) != bits(e))[0])
    b.close()
