"""GPU tests of the reverb stage (NA_BatchEnableReverbStage / LoadReverbIR / SetStreamReverb, csrc/reverb_stage.h):
partitioned FFT convolution of a row with a long impulse response, behind the cabinet stage and in front of the output stage.

The contract states every f32 operation and its order, so the expected value is the numpy float32 restatement of tests/reverb_cases.py
fed with the library's own twiddle table (NA_DebugReverbTwiddles), and the comparison is bit for bit.  Part 1 drives the stage through
its hook (NA_DebugRunReverbStage) on rows that stand in for model outputs, on a Nano batch of five rows; part 2 runs the twelve-row
batch of tests/handover_cases.py beside its twin without the stage."""
import copy
import os

import numpy as np
import pytest

import handover_cases as H
import reverb_cases as R

FORCED = bool(os.environ.get("NA_WN_KERNEL") or os.environ.get("NA_WN_PACK") or os.environ.get("NA_WN_SPEC") or os.environ.get("NA_SP_T")
              or os.environ.get("NA_SP_GEN") or os.environ.get("NA_WN_PAD"))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(FORCED, reason="forced kernel family")]

ROWS = 5
EDGE_K = [1, 2, 127, 128, 129, 255, 256, 257, 1000]
F = np.float32


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
    return capi.load_library().NA_DebugReverbLaunches


@pytest.fixture(scope="module")
def tw(na):
    return R.library_twiddles()


def odd(n):
    return n + 3


def bits_differ(a, b):
    return np.flatnonzero(np.ascontiguousarray(a, F).view(np.uint32) != np.ascontiguousarray(b, F).view(np.uint32))


# ================================================================================================ 1: through the hook

def test_the_librarys_twiddles_are_the_rounded_values(tw):
    """The table the transform uses, computed on the host in double and rounded: within one f32 ulp of numpy's."""
    mine = R.twiddles_numpy()
    assert tw.shape == (256,) and tw[0] == 1.0 and tw[2 * 64 + 1] == -1.0
    assert np.all(np.abs(tw.astype(np.float64) - mine.astype(np.float64)) <= np.spacing(np.maximum(np.abs(tw), np.abs(mine))))


@pytest.mark.parametrize("max_taps", [1024, 4096])
def test_edges_of_head_and_partitions(na, models, launches, tw, max_taps):
    """K around the head's and the partitions' edges, 700 samples as calls of 300, 1 and 399 with an odd stride: rows 0 and 3 share an
    IR (wet 0.75, dry 0.5), row 2 has another (the convolution alone), rows 1 and 4 have none and keep their bits, a -0.0 included.
    Every K on the same batch, each from a row without a reverb (T0 = the set call).  The same seeds at maxTaps = 1024 and 4096: both
    equal the restatement's bits, so maxTaps does not show."""
    rng = np.random.default_rng(31)
    hb = R.HookBatch(na, models[H.NANO], ROWS, max_taps)
    info = hb.b.ReverbInfo()
    assert info["maxTaps"] == max_taps and info["partitionSamples"] == 128 and info["pieceSamples"] == R.PIECE
    assert info["slots"] >= max_taps // 128 - 1 + info["pieceSamples"] // 128 and info["deviceBytes"] >= 16 * info["slots"] * 2048
    calls = [300, 1, 399]
    for taps in EDGE_K:
        h1, h2 = R.decaying(rng, taps), R.decaying(rng, taps)
        h1[-1], h2[-1] = 0.3, -0.2  # (the last tap counts)
        a, b = hb.b.LoadReverbIR(h1), hb.b.LoadReverbIR(h2)
        x = rng.standard_normal((ROWS, 700)).astype(F)
        x[1, 5] = F(-0.0)
        for s, ir, wet, dry in ((0, a, 0.75, 0.5), (2, b, 1.0, 0.0), (3, a, 0.75, 0.5)):
            hb.b.SetStreamReverb(s, ir, wet, dry, 0)
            got = hb.b.GetStreamReverb(s)
            assert got == (ir, wet, dry), got
        before = launches()
        y = hb.run(x, calls, stride=odd)
        assert launches() - before == R.expected_launches(0, calls) == 10
        for s, h, wet, dry in ((0, h1, 0.75, 0.5), (2, h2, 1.0, 0.0), (3, h1, 0.75, 0.5)):
            e = R.reverb_f32(h, x[s], tw, wet, dry)
            assert R.same_bits(y[s], e), (taps, s, bits_differ(y[s], e)[:5])
        assert R.same_bits(y[1], x[1]) and R.same_bits(y[4], x[4]), taps
        for s in (0, 2, 3):
            hb.b.SetStreamReverb(s, -1, 0.0, 0.0, 0)
        hb.b.UnloadReverbIR(a)
        hb.b.UnloadReverbIR(b)
    assert hb.b.ReverbInfo()["numIRs"] == 0
    hb.close()


def test_integer_case_on_the_device(na, models, tw):
    """Integer taps in [-4, 4] and samples in [-8, 8], K = 1000, 3000 samples: np.rint equals the exact integers, the largest error
    is below 0.01, and the bits are the restatement's."""
    rng = np.random.default_rng(7)
    h, x = R.integers(rng, 1000, 4), R.integers(rng, (ROWS, 3000), 8)
    hb = R.HookBatch(na, models[H.NANO], ROWS, 1024)
    hb.b.SetStreamReverb(1, hb.b.LoadReverbIR(h), 1.0, 0.0, 0)
    y = hb.run(x, [3000])
    ref = R.conv64(h, x[1])
    print("integers on the device: largest error %.3g" % float(np.max(np.abs(y[1] - ref))))
    assert np.array_equal(np.rint(y[1]), ref) and np.max(np.abs(y[1] - ref)) < 0.01
    assert R.same_bits(y[1], R.reverb_f32(h, x[1], tw)) and R.same_bits(y[0], x[0])
    hb.close()


def test_ring_wrap_and_cuts(na, models, tw):
    """maxTaps = K = 512, 4000 samples (31 blocks through a ring of 12 spectra): calls of 128 on block boundaries, 300 one-sample calls
    followed by ragged calls, and calls of 2500 and 1500, longer than a piece.  The three outputs are equal in bits to one another
    and to the restatement."""
    rng = np.random.default_rng(32)
    h = R.decaying(rng, 512)
    x = rng.standard_normal((ROWS, 4000)).astype(F)
    cuts = ([128] * 31 + [32], [1] * 300 + H.ragged(3700), [2500, 1500])
    outs = []
    for calls in cuts:
        hb = R.HookBatch(na, models[H.NANO], ROWS, 512)
        assert hb.b.ReverbInfo()["slots"] < 31 and max(cuts[2]) > hb.b.ReverbInfo()["pieceSamples"]
        ir = hb.b.LoadReverbIR(h)
        hb.b.SetStreamReverb(0, ir, 0.5, 1.0, 0)
        hb.b.SetStreamReverb(4, ir, 1.0, 0.0, 0)
        outs.append(hb.run(x, calls, stride=odd))
        hb.close()
    e0, e4 = R.reverb_f32(h, x[0], tw, 0.5, 1.0), R.reverb_f32(h, x[4], tw)
    for y in outs:
        assert R.same_bits(y[0], e0) and R.same_bits(y[4], e4), (bits_differ(y[0], e0)[:5], bits_differ(y[4], e4)[:5])
        assert R.same_bits(y[1:4], x[1:4])
    assert R.rel_rms(outs[0][4], R.conv64(h, x[4])) <= 1e-6


def test_delta_irs(na, models, tw):
    """e_k for k < 128 is an exact delay on random floats (a subnormal among them: nothing is flushed); for k >= 128 the row equals the
    restatement."""
    rng = np.random.default_rng(33)
    hb = R.HookBatch(na, models[H.NANO], ROWS, 1024)
    x = rng.standard_normal((ROWS, 900)).astype(F)
    x[:, 40] = F(3e-41)
    delays = {0: 0, 1: 1, 2: 127, 3: 128, 4: 600}
    for s, d in delays.items():
        e = np.zeros(d + 1, F)
        e[d] = 1.0
        hb.b.SetStreamReverb(s, hb.b.LoadReverbIR(e), 1.0, 0.0, 0)
    y = hb.run(x, [129, 471, 300], stride=odd)
    for s, d in delays.items():
        e = np.zeros(d + 1, F)
        e[d] = 1.0
        if d < 128:
            assert np.array_equal(y[s], np.concatenate([np.zeros(d, F), x[s]])[:900]), (s, d)
            assert y[s, 40 + d] == F(3e-41) and y[s, 40 + d] != 0.0
        else:
            expect = R.reverb_f32(e, x[s], tw)
            assert R.same_bits(y[s], expect), (s, d, bits_differ(y[s], expect)[:5])
            assert np.allclose(y[s, d:], x[s, :900 - d], atol=2e-5) and np.max(np.abs(y[s, :d])) < 2e-5
    hb.close()


def _drive(hb, cab, ids, x, pos, n, stride=odd):
    """one call of n samples on both sides; returns (rows, expected, exact)"""
    xs = x[:, pos:pos + n]
    y = hb.run(xs, [n], stride=stride)
    e, exact = cab.step(xs)
    return y, e, exact


def test_switches_without_a_fade(na, models, tw):
    """N = 0 between two IRs, set mid-block: B from the first sample after the call, on the history A saw.  To no reverb and back: a
    new T0."""
    rng = np.random.default_rng(34)
    irs = {"A": R.decaying(rng, 700), "B": R.decaying(rng, 300)}
    x = rng.standard_normal((ROWS, 1400)).astype(F)
    hb = R.HookBatch(na, models[H.NANO], ROWS, 1024)
    ids = {k: hb.b.LoadReverbIR(v) for k, v in irs.items()}
    c = R.RevContract(ROWS, irs, tw)
    pos = 0
    for op, n in ((("A", 1.0, 0.0), 450), (("B", 0.5, 0.5), 333), ((None, 0.0, 0.0), 100), (("A", 1.0, 0.0), 300), (("A", 0.25, 1.0), 217)):
        hb.b.SetStreamReverb(2, -1 if op[0] is None else ids[op[0]], op[1], op[2], 0)
        c.set(2, *op)
        assert hb.b.GetStreamReverb(2)[0] == (-1 if op[0] is None else ids[op[0]]) and hb.b.ReverbFadeRemaining(2) == 0
        y, e, exact = _drive(hb, c, ids, x, pos, n)
        assert R.same_bits(y, e), (op, bits_differ(y[2], e[2])[:5])
        assert exact[2] == (op[0] is None)
        pos += n
    # B continued on A's history: the convolution of the whole history since T0 with B, from the switch on
    assert R.same_bits(hb.run(x[:, :1], [1]), c.step(x[:, :1])[0])
    hb.close()


@pytest.mark.parametrize("N", [50, 128, 300])
def test_fades(na, models, tw, N):
    """dry -> A, A -> B, a wet / dry change on B, B -> dry: every set call falls mid-block, the fade is shorter than, equal to and longer
    than a block, and is cut by the calls.  Every sample equals the restatement's blend of the two whole outputs; FadeRemaining counts
    down; UnloadReverbIR is refused while a fade holds the IR, and works after it."""
    rng = np.random.default_rng(35 + N)
    irs = {"A": R.decaying(rng, 700), "B": R.decaying(rng, 260)}
    seg = N + 203  # (not a multiple of 128: the next set call falls mid-block)
    x = rng.standard_normal((ROWS, 4 * seg)).astype(F)
    hb = R.HookBatch(na, models[H.NANO], ROWS, 1024)
    ids = {k: hb.b.LoadReverbIR(v) for k, v in irs.items()}
    c = R.RevContract(ROWS, irs, tw)
    hb.b.SetStreamReverb(3, ids["B"], 1.0, 0.0, 0)  # (row 3: B all along, on another input)
    c.set(3, "B")
    pos = 0
    steps = [("A", 1.0, 0.0, ["A"]), ("B", 0.5, 1.0, ["A", "B"]), ("B", 1.0, 0.25, ["B"]), (None, 0.0, 0.0, ["B"])]
    for ir, wet, dry, held in steps:
        hb.b.SetStreamReverb(0, -1 if ir is None else ids[ir], wet, dry, N)
        c.set(0, ir, wet, dry, N)
        assert hb.b.ReverbFadeRemaining(0) == N and hb.b.ReverbFadeRemaining(3) == 0
        with pytest.raises(na.NeuralAudioError, match="a reverb fade of stream 0 is running"):
            hb.b.SetStreamReverb(0, ids["A"], 1.0, 0.0, 0)
        for name in held:
            with pytest.raises(na.NeuralAudioError, match="in use"):
                hb.b.UnloadReverbIR(ids[name])
        done = 0
        for n in H.ragged(seg):
            y, e, exact = _drive(hb, c, ids, x, pos, n)
            assert R.same_bits(y, e), (ir, done, bits_differ(y[0], e[0])[:5])
            done += n
            pos += n
            assert hb.b.ReverbFadeRemaining(0) == max(N - done, 0) == c.remaining(0)
        assert hb.b.GetStreamReverb(0)[0] == (-1 if ir is None else ids[ir])
    hb.b.UnloadReverbIR(ids["A"])
    with pytest.raises(na.NeuralAudioError, match="in use"):
        hb.b.UnloadReverbIR(ids["B"])  # (row 3 has it)
    hb.b.SetStreamReverb(3, -1, 0.0, 0.0, 0)
    hb.b.UnloadReverbIR(ids["B"])
    assert hb.b.ReverbInfo()["numIRs"] == 0
    hb.close()


def test_one_long_ir(na, models, tw):
    """K = maxTaps = 16384 (128 partitions), two rows, three calls of 2048: the restatement's bits, and a relative RMS error against
    float64 of at most 1e-6."""
    rng = np.random.default_rng(36)
    h = R.decaying(rng, 16384)
    x = rng.standard_normal((2, 3 * 2048)).astype(F)
    b = na.Batch(0)
    assert b.AddStreams(models[H.NANO], 2, doPrewarm=False) == 0
    b.EnableReverbStage(16384)
    ir = b.LoadReverbIR(h)
    b.SetStreamReverb(0, ir, 1.0, 0.0, 0)
    b.SetStreamReverb(1, ir, 0.3, 1.0, 0)
    out = []
    for k in range(3):
        block = np.ascontiguousarray(x[:, k * 2048:(k + 1) * 2048])
        b.DebugRunReverbStage(block, 2048)
        out.append(block)
    y = np.concatenate(out, axis=1)
    e0, e1 = R.reverb_f32(h, x[0], tw), R.reverb_f32(h, x[1], tw, 0.3, 1.0)
    assert R.same_bits(y[0], e0) and R.same_bits(y[1], e1), (bits_differ(y[0], e0)[:5], bits_differ(y[1], e1)[:5])
    err = R.rel_rms(y[0], R.conv64(h, x[0]))
    print("K=16384: relative rms error %.3g" % err)
    assert err <= 1e-6
    b.close()


# ================================================================================================ 2: with models

def _irs():
    rng = np.random.default_rng(130)
    return {"room": (0.3 * R.decaying(rng, 600)).astype(F), "hall": (0.3 * R.decaying(rng, 1500)).astype(F)}


def test_off_is_off(na, models, launches):
    """The stage is enabled, IRs are loaded and no stream has a reverb: every row has the twin's bits and none of the stage's kernels
    is launched."""
    calls = [128, 17, 300, 128]
    x = H.signal(sum(calls), 41)
    yts = H.run_twin(na, models, x, calls, {})
    b = H.make_batch(na, models, stage=False)
    b.EnableReverbStage(2048)
    for taps in _irs().values():
        b.LoadReverbIR(taps)
    before, pos = launches(), 0
    for i, n in enumerate(calls):
        y = b.Process(np.ascontiguousarray(x[:, pos:pos + n]))
        assert np.array_equal(y, yts[i]), i
        pos += n
    assert launches() == before and np.any(yts[0][0]) and np.any(yts[0][4]) and np.any(yts[0][8])
    b.close()


def test_the_order_is_cabinet_reverb_gain(na, models, tw):
    """Row 4 (Standard) of the twelve-row batch gets a cabinet IR in front of call 1, a reverb in front of call 2 and a gain ramp in
    front of call 3.  The cabinet IR is 0.5 e_2, exact in any order of summation, so the reverb's input is known bit for bit: up to
    the ramp the row equals the restatement on the twin's delayed and halved row -- with samples from before the reverb's T0 in it,
    which only the order cabinet -> reverb gives -- and from the ramp on it lies within the output stage's tolerance of its contract
    applied to that restatement (the reverb of a ramped row is far from it).  Rows without a reverb keep the twin's bits."""
    calls = [128, 100, 300, 128, 17, 300]
    x = H.signal(sum(calls), 42)
    yts = H.run_twin(na, models, x, calls, {})
    room = _irs()["room"]
    b = H.make_batch(na, models, stage=True)
    b.EnableCabinetStage(256)
    b.EnableReverbStage(2048)
    cab, rev = b.LoadIR(np.array([0.0, 0.0, 0.5], F)), b.LoadReverbIR(room)
    cab_in, rev_in, outc, pos = [], [], H.Contract(), 0
    for i, n in enumerate(calls):
        if i == 1:
            b.SetStreamIR(4, cab, 0)
        if i == 2:
            b.SetStreamReverb(4, rev, 0.6, 1.0, 0)
        if i == 3:
            b.SetStreamGain(4, 0.3, 200)
            outc.apply(("gain", 4, 0.3, 200))
        y = b.Process(np.ascontiguousarray(x[:, pos:pos + n]))
        if i >= 1:
            cab_in.append(yts[i][4])
        hist = np.concatenate(cab_in) if cab_in else np.zeros(0, F)
        c = (F(0.5) * np.concatenate([np.zeros(2, F), hist]))[:len(hist)][len(hist) - n:] if i >= 1 else yts[i][4]
        z = c
        if i >= 2:
            rev_in.append(c)
            z = R.reverb_f32(room, np.concatenate(rev_in), tw, 0.6, 1.0, start=sum(len(r) for r in rev_in) - n)
        rows = yts[i].copy()
        rows[4] = z
        gain = copy.deepcopy(outc).step(np.ones_like(rows))[0][4]
        e, bound, exact = outc.step(rows)
        if exact[4]:
            assert R.same_bits(y[4], z), (i, bits_differ(y[4], z)[:5])
        else:
            err, limit = np.abs(y[4].astype(np.float64) - e[4]), H.REL * bound[4] + H.ABS
            assert np.all(err <= limit), (i, float(np.max(err / limit)))
            if i == 3:  # the other order: the reverb of the ramped row
                ramped = np.concatenate(rev_in[:-1] + [(gain * c).astype(F)])
                other = R.reverb_f32(room, ramped, tw, 0.6, 1.0, start=len(ramped) - n)
                assert np.max(np.abs(other - e[4])) > 100 * np.max(limit)
        for s in (0, 1, 5, 8, 9):
            assert np.array_equal(y[s], yts[i][s]), (i, s)
        pos += n
    assert i == 5 and not exact[4] and b.GetStreamGain(4) == pytest.approx(0.3)
    b.close()


def test_set_calls_and_processing_with_fades_are_real_time_safe(na, models):
    """NA_DebugDeviceResourceCalls stays where it is across set calls and 21 processing calls with fades running, over the blocking and
    the pipelined host path and device pointers (after three warm calls of each, which size the staging block and the pipeline slots)."""
    import torch
    from neuralaudio_amd import capi
    lib = capi.load_library()
    dev = torch.device("cuda", 0)
    b = H.make_batch(na, models, stage=False)
    b.EnableReverbStage(2048)
    ids = {name: b.LoadReverbIR(taps) for name, taps in _irs().items()}
    n = 128
    x = H.signal(n, 45)
    dx, dy = torch.from_numpy(x).to(dev), torch.zeros(H.ROWS, n, device=dev)
    torch.cuda.synchronize(dev)

    def three():
        b.Process(x)
        b.Collect(b.Submit(x))
        b.ProcessDevice(dx.data_ptr(), dy.data_ptr(), n, n, n)
        b.Synchronize()

    b.SetStreamReverb(0, ids["room"], 0.5, 1.0, 0)
    for _ in range(3):
        three()
    before = lib.NA_DebugDeviceResourceCalls()
    b.SetStreamReverb(0, ids["hall"], 0.5, 1.0, 5000)
    b.SetStreamReverb(4, ids["room"], 0.3, 1.0, 4000)
    b.SetStreamReverb(8, ids["hall"], 1.0, 0.0, 100)
    for i in range(7):
        three()
        if i == 3:
            b.SetStreamReverb(8, -1, 0.0, 0.0, 2000)
            b.SetStreamReverb(9, ids["room"], 1.0, 1.0, 0)
    assert b.ReverbFadeRemaining(0) == 5000 - 21 * n and b.ReverbFadeRemaining(8) == 2000 - 9 * n
    assert lib.NA_DebugDeviceResourceCalls() == before
    assert np.all(np.isfinite(dy.cpu().numpy()))
    b.close()


def test_park_and_remove_drop_the_history(na, models, tw):
    """A parked stream comes back without a reverb and its IR is free; a reverb set again starts from an empty history (the new T0).
    A removed stream's id comes back without a reverb too."""
    calls = [128, 200, 64, 128, 300]
    x = H.signal(sum(calls), 43)
    twin_ops = {2: [("park", 4)], 3: [("activate", 4)]}
    yts = H.run_twin(na, models, x, calls, twin_ops)
    room = _irs()["room"]
    b = H.make_batch(na, models, stage=False)
    b.EnableReverbStage(2048)
    rev = b.LoadReverbIR(room)
    pos, since = 0, []
    for i, n in enumerate(calls):
        if i == 1:
            b.SetStreamReverb(4, rev, 1.0, 0.5, 3000)
        if i == 2:
            b.ParkStream(4)
            b.UnloadReverbIR(rev)  # (the park took the stream's hold on it away, fade and all)
            rev = b.LoadReverbIR(room)
        if i == 3:
            b.ActivateStream(4, 1.0)
            assert b.GetStreamReverb(4)[0] == -1 and b.ReverbFadeRemaining(4) == 0
        if i == 4:
            b.SetStreamReverb(4, rev, 1.0, 0.5, 0)
        y = b.Process(np.ascontiguousarray(x[:, pos:pos + n]))
        if i == 1:
            hist = yts[i][4]
            e = R.blend_f32(R.weight32(3000, np.arange(n)), hist, R.reverb_f32(room, hist, tw, 1.0, 0.5))
            assert R.same_bits(y[4], e)
        elif i == 4:
            assert R.same_bits(y[4], R.reverb_f32(room, yts[i][4], tw, 1.0, 0.5)), "the history starts empty at the new T0"
        else:
            assert np.array_equal(y[4], yts[i][4]), i
        assert np.array_equal(y[5], yts[i][5])
        pos += n
    b.close()
    b = na.Batch(0)
    assert b.AddStreams(models[H.NANO], 3, doPrewarm=False) == 0
    b.EnableReverbStage(512)
    rev = b.LoadReverbIR(room[:512])
    b.SetStreamReverb(1, rev, 1.0, 1.0, 0)
    b.RemoveStreams(1, 1)
    b.UnloadReverbIR(rev)
    assert b.AddStreams(models[H.NANO], 1, doPrewarm=False) == 1 and b.GetStreamReverb(1)[0] == -1
    b.close()


def test_growth_keeps_the_histories(na, models, tw):
    """Four Standard streams, a reverb on row 1, two calls of 128; sixteen more streams take the rows past the stage's first capacity
    of 16, so its blocks move; two more calls.  Row 1 is, bit for bit, the restatement on the whole history (row 0 runs the same input
    without a reverb), the samples from before the move included."""
    n, hall = 128, _irs()["hall"]
    x = np.stack([H.noise(4 * n, 3100 + r) for r in range(20)])
    x[1] = x[0]
    b = na.Batch(0)
    assert b.AddStreams(models[H.STD], 4) == 0
    b.EnableReverbStage(2048)
    b.SetStreamReverb(1, b.LoadReverbIR(hall), 0.8, 1.0, 0)
    before = b.ReverbInfo()["deviceBytes"]
    out = []
    for k in range(4):
        if k == 2:
            assert b.AddStreams(models[H.STD], 16) == 4
            info = b.ReverbInfo()
            assert info["deviceBytes"] > before and info["deviceBytes"] >= 20 * info["slots"] * 2048
        out.append(b.Process(x[:b.NumStreams(), k * n:(k + 1) * n])[:4])
    y = np.concatenate(out, axis=1)
    e = R.reverb_f32(hall, y[0], tw, 0.8, 1.0)
    assert R.same_bits(y[1], e), bits_differ(y[1], e)[:5]
    b.close()


def test_rules(na, models):
    """Every rule fails with a message that names it."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    b = H.make_batch(na, models, stage=False)
    for call in (lambda: b.SetStreamReverb(0, -1, 0.0, 0.0, 0), lambda: b.GetStreamReverb(0), lambda: b.ReverbFadeRemaining(0),
                 lambda: b.LoadReverbIR(np.ones(4, F)), lambda: b.UnloadReverbIR(0), lambda: b.ReverbInfo(),
                 lambda: b.DebugRunReverbStage(np.zeros((H.ROWS, 8), F))):
        with pytest.raises(na.NeuralAudioError, match="reverb stage not enabled"):
            call()
    assert lib.NA_BatchGetStreamReverb(b._h, 0, None, None) <= -2 and lib.NA_BatchStreamReverbFadeRemaining(b._h, 0) < 0
    for bad in (0, 131073, -5):
        with pytest.raises(na.NeuralAudioError, match=r"maxTaps must lie in \[1, 131072\]"):
            b.EnableReverbStage(bad)
    b.EnableReverbStage(256)
    b.EnableReverbStage(256)
    b.EnableReverbStage(100)  # idempotent for an equal or smaller maxTaps
    assert b.ReverbInfo()["maxTaps"] == 256
    with pytest.raises(na.NeuralAudioError, match=r"numTaps must lie in \[1, maxTaps\]"):
        b.LoadReverbIR(np.ones(257, F))
    with pytest.raises(na.NeuralAudioError, match=r"numTaps must lie in \[1, maxTaps\]"):
        b.LoadReverbIR(np.ones(0, F))
    with pytest.raises(na.NeuralAudioError, match="taps must be finite"):
        b.LoadReverbIR(np.array([1.0, np.inf], F))
    a, c = b.LoadReverbIR(np.ones(256, F)), b.LoadReverbIR(np.ones(2, F))
    assert (a, c) == (0, 1) and b.ReverbInfo()["numIRs"] == 2
    b.UnloadReverbIR(a)
    assert b.LoadReverbIR(np.ones(7, F)) == a, "ids of unloaded IRs are recycled"
    with pytest.raises(na.NeuralAudioError, match="IR 5 is not loaded"):
        b.SetStreamReverb(0, 5, 1.0, 1.0, 0)
    with pytest.raises(na.NeuralAudioError, match="IR 5 is not loaded"):
        b.UnloadReverbIR(5)
    with pytest.raises(na.NeuralAudioError, match="stream 2 is parked"):
        b.SetStreamReverb(2, a, 1.0, 1.0, 0)
    with pytest.raises(na.NeuralAudioError, match="stream 12 is not a live stream"):
        b.SetStreamReverb(12, a, 1.0, 1.0, 0)
    with pytest.raises(na.NeuralAudioError, match="wet and dry must be finite"):
        b.SetStreamReverb(0, a, np.inf, 1.0, 0)
    for fade in (-1, (1 << 20) + 1):
        with pytest.raises(na.NeuralAudioError, match=r"fadeSamples must lie in \[0, 1 << 20\]"):
            b.SetStreamReverb(0, a, 1.0, 1.0, fade)
    b.SetStreamReverb(0, a, 0.5, 0.25, 1 << 20)
    with pytest.raises(na.NeuralAudioError, match="a reverb fade of stream 0 is running"):
        b.SetStreamReverb(0, c, 1.0, 1.0, 0)
    with pytest.raises(na.NeuralAudioError, match="in use"):
        b.UnloadReverbIR(a)
    with pytest.raises(na.NeuralAudioError, match="a larger maxTaps is refused while a stream has a reverb"):
        b.EnableReverbStage(512)
    assert b.GetStreamReverb(0) == (a, 0.5, 0.25) and b.ReverbFadeRemaining(0) == 1 << 20 and b.GetStreamReverb(1)[0] == -1
    b.ParkStream(0)  # no reverb at once: the IR is free, the stage may grow
    b.UnloadReverbIR(a)
    b.EnableReverbStage(512)
    assert b.ReverbInfo()["maxTaps"] == 512
    y = b.Process(H.signal(64, 44))
    assert np.all(np.isfinite(y))
    b.close()
