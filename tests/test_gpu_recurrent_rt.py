"""The runtime-shaped recurrent kernel (lstm_kernels.hip RecurrentWaveRtKernel) in batches and at its edges, through the C ABI.

Every LSTM / GRU that is not one of the small LDS-free layouts runs on this kernel: gate weights in LDS or streamed transposed from L2,
one wave per stream or a workgroup of 2 .. 16 waves, 1 .. 8 gate rows per lane, the head after the block or inside the sample loop.
The shapes (tests/recurrent_cases.py) sit on both sides of every edge of the library's own plan function, and every case first asserts
through NA_DebugRecurrentPlan that it runs in the regime it is named for (not under a tuning knob: a forced run keeps the parity
assertions only).

Checkers: the C oracle (float32, the reference's term order) for every shape; up to 256 units also the float64 restatement
(tests/ref_np.py).  Tolerance: the project's 5e-6 RMS as 5e-6 * max(1, rms(want)).  tests/test_host_cpu.py proves without a GPU that
the oracle itself stays a factor 10 under that bound against float64 (a factor 4 at amplitude 1000).

Every test prints the distance it measured beside its bound before it asserts (`-s` / `-rP` shows them)."""
import json
import os

import numpy as np
import pytest

import na_oracle as O
import recurrent_cases as RC
import ref_np as R

pytestmark = pytest.mark.gpu

NANO = "BossWN-nano.nam"
DPP_LSTM = "BossLSTM-1x16.nam"


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


_built = {}


def built(c):
    """Model document and references of a case, shared between the tests of this file (the large documents are not kept)."""
    key = RC.case_id(c)
    if key in _built:
        return _built[key]
    b = RC.Built(c)
    if c["hidden"] <= 256:
        _built[key] = b
    return b


_wants = {}


def oracle_output(c, b, x):
    """The C oracle's output for the case's own signal: computed once, shared, never changed."""
    key = RC.case_id(c)
    if key not in _wants:
        want = b.oracle().process(x)
        want.setflags(write=False)
        _wants[key] = want
    return _wants[key]


def assert_regime(m, c):
    if RC.knob_set():
        return
    p = m.RecurrentPlan()
    assert p["runs"], (RC.case_id(c), p)
    assert {f: int(p[f]) for f in RC.FIELDS} == c["regime"], (RC.case_id(c), p, c["regime"])


def bit_equal(got, want, what):
    assert np.array_equal(got, want), (what, int(np.argmax(got != want)), int(np.count_nonzero(got != want)), O.rms(got - want))


def run_batch(batch, x, sizes):
    return RC.run_in_calls(lambda chunk: batch.Process(np.ascontiguousarray(chunk)), x, sizes)


# ---------------------------------------------------------------------------------------------------------------- (a) edge shapes

@pytest.mark.parametrize("c", RC.edge_cases(), ids=RC.case_id)
def test_edge_shape_matches_the_oracle(na, c):
    """One stream through ragged calls (n = 1 first, one call above LSTM_MAX_FRAMES) against the C oracle, and up to 256 units against
    the float64 restatement as well."""
    b = built(c)
    m = b.load(na)
    assert_regime(m, c)
    x = RC.signal(c)
    y = RC.run_in_calls(m.Process, x, RC.call_sizes(c["samples"], c["seed"]))
    assert np.all(np.isfinite(y))
    want = oracle_output(c, b, x)
    err = O.rms(y - want)
    print("%-22s %-34s regime %s: GPU-oracle rms %.3g, bound %.3g" % (RC.case_id(c), c["why"], c["regime"], err, RC.bound(want)))
    assert err <= RC.bound(want), (RC.case_id(c), err, RC.bound(want))
    if c["hidden"] <= 256:
        w64 = b.f64(x)
        e64 = O.rms(y - w64)
        print("%-22s GPU-float64 rms %.3g" % (RC.case_id(c), e64))
        assert e64 <= RC.bound(w64), (RC.case_id(c), e64, RC.bound(w64))
    m.close()


# ---------------------------------------------------------------------------------------------------------------- (b) call sizes

CALL_SIZE_SHAPES = [("lstm", 3, 16), ("lstm", 1, 65), ("gru", 1, 86), ("lstm", 2, 64), ("lstm", 1, 129), ("gru", 2, 171), ("lstm", 1, 257),
                    ("gru", 1, 342), ("lstm", 1, 613)]


@pytest.mark.parametrize("kind,layers,hidden", CALL_SIZE_SHAPES, ids=lambda v: str(v))
def test_output_does_not_depend_on_the_call_sizes(na, kind, layers, hidden):
    """Per sample the kernel's arithmetic does not depend on n: the same model and signal through ragged calls, through one call of the
    whole signal (chunks of 128) and through calls of 64 | 65 | 1 | rest give the same bits."""
    c = RC.small_case(kind, layers, hidden, prewarm=False, samples=300 if hidden <= 256 else 150)
    b = built(c)
    x = RC.signal(c)
    outs = []
    for sizes in (RC.call_sizes(c["samples"], 5), [c["samples"]], [64, 65, 1, c["samples"] - 130]):
        m = b.load(na)
        outs.append(RC.run_in_calls(m.Process, x, sizes))
        m.close()
    bit_equal(outs[1], outs[0], (kind, layers, hidden, "one call"))
    bit_equal(outs[2], outs[0], (kind, layers, hidden, "64|65|1|rest"))


# ---------------------------------------------------------------------------------------------------------------- (c) batches

def _alone(na, m, x, sizes, prewarm):
    one = na.Batch(0)
    one.AddStreams(m, 1, doPrewarm=prewarm)
    y = run_batch(one, x[None, :], sizes)[0]
    one.close()
    return y


@pytest.mark.parametrize("kind,layers,hidden", RC.BATCH_SHAPES, ids=lambda v: str(v))
def test_batch_with_recycled_slots_matches_the_oracle_and_the_stream_alone(na, kind, layers, hidden):
    """Seven streams, a block, streams 1 and 4 removed, three added one by one (ids 1, 4 and a new row 7: state slots are recycled and
    rows[] is no longer the identity), then ragged blocks.  Every stream equals its own oracle to the tolerance and the same model run
    alone on the same inputs and call sizes bit for bit."""
    c = RC.small_case(kind, layers, hidden, prewarm=hidden <= 256)
    b = built(c)
    m = b.load(na)
    assert_regime(m, c)
    pw = c["prewarm"]
    first, later = [100], [1, 3, 129, 64, 65, 38]
    n1, n2 = sum(first), sum(later)
    x = np.stack([O.signal_noise(n1 + n2, 500 + r) for r in range(8)])
    batch = na.Batch(0)
    assert batch.AddStreams(m, 7, doPrewarm=pw) == 0
    y1 = run_batch(batch, x[:7, :n1], first)
    batch.RemoveStreams(1)
    batch.RemoveStreams(4)
    assert [batch.AddStreams(m, 1, doPrewarm=pw) for _ in range(3)] == [1, 4, 7]
    assert batch.NumStreams() == 8 and batch.StreamKernelName(7) == "RecurrentWaveRtKernel"
    y2 = run_batch(batch, x[:, n1:], later)
    batch.close()
    worst = 0.0
    for r in range(8):
        if r in (1, 4, 7):  # joined after the first block
            got, xin, sizes = y2[r], x[r, n1:], later
        else:
            got, xin, sizes = np.concatenate([y1[r], y2[r]]), x[r], first + later
        want = b.oracle().process(xin)
        err = O.rms(got - want)
        worst = max(worst, err)
        assert err <= RC.bound(want), (kind, layers, hidden, r, err)
        bit_equal(got, _alone(na, m, xin, sizes, pw), (kind, layers, hidden, r))
    print("%s %dx%d batch: worst GPU-oracle rms %.3g" % (kind, layers, hidden, worst))


def test_batch_of_two_runtime_shaped_models_beside_a_dpp_lstm_and_a_wavenet(na):
    """LSTM 1x65 and GRU 1x86 beside the LDS-free LSTM 1x16 and a Nano WaveNet in one batch, two streams each, interleaved rows."""
    loader = na.NeuralModelLoader()
    cl, cg = RC.small_case("lstm", 1, 65), RC.small_case("gru", 1, 86)
    bl, bg = built(cl), built(cg)
    ml, mg = bl.load(na, loader), bg.load(na, loader)
    md, mw = loader.CreateFromFile(os.path.join(O.MODELS_DIR, DPP_LSTM)), loader.CreateFromFile(os.path.join(O.MODELS_DIR, NANO))
    order = [ml, mw, mg, md, mg, ml, md, mw]
    batch = na.Batch(0)
    for r, m in enumerate(order):
        assert batch.AddStreams(m, 1) == r
    sizes = [1, 2, 128, 129, 63, 77]
    x = np.stack([O.signal_noise(sum(sizes), 700 + r) for r in range(len(order))])
    y = run_batch(batch, x, sizes)
    batch.close()
    for r, m in enumerate(order):
        if m is ml or m is mg:
            want = (bl if m is ml else bg).oracle(True).process(x[r])
            bit_equal(y[r], _alone(na, m, x[r], sizes, True), r)
        else:
            want = O.oracle_from_file(DPP_LSTM if m is md else NANO).process(x[r])
        assert O.rms(y[r] - want) <= RC.bound(want), (r, O.rms(y[r] - want))


def test_batch_growing_past_its_first_capacity_keeps_live_state(na):
    """70 streams of LSTM 1x40: 60 run a block, ten more join -- more than the first capacity of 64 state columns, so the state of the
    live streams is re-strided -- and all of them go on to match their oracles."""
    c = RC.small_case("lstm", 1, 40)
    b = built(c)
    m = b.load(na)
    assert_regime(m, c)
    batch = na.Batch(0)
    assert batch.AddStreams(m, 60) == 0
    n1, later = 70, [1, 129, 50]
    x = np.stack([O.signal_noise(n1 + sum(later), 900 + r) for r in range(70)])
    y1 = batch.Process(np.ascontiguousarray(x[:60, :n1]))
    assert batch.AddStreams(m, 10) == 60
    y2 = run_batch(batch, x[:, n1:], later)
    batch.close()
    for r in range(70):
        got, xin = (np.concatenate([y1[r], y2[r]]), x[r]) if r < 60 else (y2[r], x[r, n1:])
        want = b.oracle(True).process(xin)
        assert O.rms(got - want) <= RC.bound(want), (r, O.rms(got - want))


# ---------------------------------------------------------------------------------------------------------------- (d) snapshot

def _snapshot_models(na):
    out = []
    for kind, layers, hidden in RC.SNAPSHOT_SHAPES:
        c = RC.small_case(kind, layers, hidden)
        out.append(("%s %dx%d" % (kind, layers, hidden), lambda c=c: (built(c).load(na), c)))
    spec = RC.TAIL_STACKS[1]
    out.append(("stack lstm130-dense64", lambda: (na.NeuralModelLoader().CreateFromString(json.dumps(R.synth_keras_stack(spec, seed=43)), ".json"), None)))
    return out


@pytest.mark.parametrize("which", range(len(RC.SNAPSHOT_SHAPES) + 1))
def test_snapshot_moves_a_stream_between_batches_bit_for_bit(na, which):
    """Half the signal in a batch of five, SaveStreams from slot 3, LoadStreams into slot 0 of a batch of two: the continuation there
    is the uninterrupted run's, bit for bit (LSTM 2x131, GRU 1x171, a multi-wave LSTM 130 with a dense tail)."""
    name, make = _snapshot_models(na)[which]
    m, c = make()
    assert m is not None
    if c is not None:
        assert_regime(m, c)
    half = [1, 129, 20]
    rest = [3, 64, 65, 18]
    x = np.stack([O.signal_noise(sum(half) + sum(rest), 40 + r) for r in range(5)])
    a = na.Batch(0)
    a.AddStreams(m, 5)
    run_batch(a, x[:, :sum(half)], half)
    blob = a.SaveStreams(3)
    want = run_batch(a, x[:, sum(half):], rest)[3]
    a.close()
    bb = na.Batch(0)
    bb.AddStreams(m, 2)
    bb.Process(np.ascontiguousarray(x[:2, :37]))  # (batch B has a past of its own)
    bb.LoadStreams(0, blob)
    x2 = np.stack([x[3, sum(half):], x[1, sum(half):]])
    got = run_batch(bb, x2, rest)[0]
    bb.close()
    assert np.any(want)
    bit_equal(got, want, name)


# ---------------------------------------------------------------------------------------------------------------- (e) pool

@pytest.mark.parametrize("kind,layers,hidden", RC.POOL_SHAPES, ids=lambda v: str(v))
def test_an_activated_stream_equals_a_freshly_added_prewarmed_one(na, kind, layers, hidden):
    """tests/test_gpu_pool.py's assertion at shapes whose stream state has hundreds of elements: reserve four, run with everybody
    parked, activate 2 and 1, run ragged calls -- the rows are those of a twin built with AddStreams, bit for bit, and match the oracle."""
    c = RC.small_case(kind, layers, hidden)
    b = built(c)
    m = b.load(na)
    sizes = [128, 1, 17, 129]
    x = np.stack([O.signal_noise(sum(sizes), 300 + r) for r in range(4)])
    pool = na.Batch(0)
    assert pool.ReserveStreams(m, 4, doPrewarm=True) == 0
    assert not np.any(pool.Process(np.stack([O.signal_noise(200, 90 + r) for r in range(4)])))
    pool.ActivateStream(2)
    pool.ActivateStream(1)
    y = run_batch(pool, x, sizes)
    pool.ParkStream(2)
    pool.ActivateStream(2)  # (a park -> activate cycle carries nothing over)
    y2 = run_batch(pool, x, sizes)
    twin = na.Batch(0)
    twin.AddStreams(m, 4, doPrewarm=True)
    yt = run_batch(twin, x, sizes)
    assert pool.StreamKernelName(2) == twin.StreamKernelName(2) == "RecurrentWaveRtKernel"
    pool.close()
    twin.close()
    for r in range(4):
        if r in (1, 2):
            bit_equal(y[r], yt[r], (kind, hidden, r))
            want = b.oracle(True).process(x[r])
            assert O.rms(y[r] - want) <= RC.bound(want), (r, O.rms(y[r] - want))
        else:
            assert not np.any(y[r]), r
    bit_equal(y2[2], yt[2], (kind, hidden, "after park -> activate"))


# ---------------------------------------------------------------------------------------------------------------- (f) tails

def _stack_parity(na, spec, seed, prewarm, must_load=True):
    mj = R.synth_keras_stack(spec, seed=seed)
    try:
        m = na.NeuralModelLoader().CreateFromString(json.dumps(mj), ".json", doPrewarm=prewarm)
    except na.NeuralAudioError as e:  # (a shape without a kernel is refused at load, by name)
        assert not must_load and "is not supported" in str(e), (spec, e)
        return None
    if m is None and not must_load:
        return None
    assert m is not None, spec
    x = O.signal_noise(300, 9)
    y = RC.run_in_calls(m.Process, x, RC.call_sizes(300, 3))
    want = R.keras_stack_forward(mj, x, prewarm=2048 if prewarm else 0)
    err = O.rms(y - want)
    print("%s: GPU-float64 rms %.3g, bound %.3g" % (spec, err, RC.bound(want)))
    assert np.all(np.isfinite(y)) and err <= RC.bound(want), (spec, err)
    return m


@pytest.mark.parametrize("spec", RC.TAIL_STACKS, ids=RC.stack_id)
def test_tail_behind_the_runtime_shaped_layers_matches_the_float64_stack(na, spec):
    """A dense or conv1d tail behind recurrent layers of several waves -- the first wave alone evaluates the tail while the workgroup has
    more than 64 threads -- and behind a one-wave stack whose conv1d scratch pushes the gate weights out of the LDS."""
    m = _stack_parity(na, spec, 40 + len(spec), True)
    if not RC.knob_set():
        p = m.RecurrentPlan()
        assert p["runs"] and not p["head_in_loop"], p
        assert {f: int(p[f]) for f in RC.FIELDS} == RC.stack_regime(spec), (p, RC.stack_regime(spec))


@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_widest_layer_with_a_dense_tail_and_the_next_one_up(na, kind):
    """The widest recurrent layer with a dense tail that the kernel's shape predicate admits (its [samples][H] buffer must fit the LDS)
    matches the reference; the next size up either fails to load or matches too -- never silently different."""
    h = RC.widest_with_dense_tail(kind)
    assert 128 < h < RC.MAX_HIDDEN
    tail = [("dense", RC.TAIL_DENSE, "tanh"), ("dense", 1)]
    assert _stack_parity(na, [(kind, h)] + tail, 77, False) is not None
    _stack_parity(na, [(kind, h + 1)] + tail, 78, False, must_load=False)


# ---------------------------------------------------------------------------------------------------------------- (g) level

@pytest.mark.parametrize("amp", RC.LEVELS)
@pytest.mark.parametrize("kind,layers,hidden", RC.LEVEL_SHAPES, ids=lambda v: str(v))
def test_level_stays_within_tolerance_of_the_float64_restatement(na, kind, layers, hidden, amp):
    """Amplitudes 1e-5, 30 and 1000 (the gates saturate; rms(y) reaches 1.8): finite, and within the bound of float64."""
    c = RC.small_case(kind, layers, hidden, prewarm=False)
    b = built(c)
    m = b.load(na)
    x = RC.signal(c, amp)
    y = RC.run_in_calls(m.Process, x, RC.call_sizes(c["samples"], 11))
    want = b.f64(x)
    err = O.rms(y - want)
    print("%s %dx%d amplitude %g: GPU-float64 rms %.3g, bound %.3g" % (kind, layers, hidden, amp, err, RC.bound(want)))
    assert np.all(np.isfinite(y))
    assert err <= RC.bound(want), (kind, hidden, amp, err, RC.bound(want))
    m.close()
