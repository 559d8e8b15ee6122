"""The keras-stack tails (recurrent_tail.h DenseTail / ConvTail) in batches and at their edges, through the C ABI.

A generic keras stack -- what the reference hands to RTNeural -- ends in a chain of dense and conv1d layers.  A chain of dense layers is
evaluated per sample (DenseTail: at the end of RecurrentWaveRtKernel, and inside LstmGenericKernel / GruGenericKernel under the knobs
that send models there); a chain with conv1d layers is evaluated layer by layer over the block by the first wave of
RecurrentWaveRtKernel (ConvTail), its input history living in the stream's state at state[(tailHistRow[t] + idx) * capacity + slot].

Checker: the float64 restatement tests/ref_np.keras_stack_forward -- RTNeural is an absent submodule, there is no C oracle -- with
prewarm = 2048 where the model is prewarmed and 0 where it is not.  Tolerance: the project's 5e-6 RMS as 5e-6 * max(1, rms(want)).
The cases (tests/tail_cases.py) carry a gain on their input kernels so that the signal path dominates the output;
tests/test_host_cpu.py proves without a GPU that every case's output depends on its input, that float32 arithmetic alone stays below a
quarter of the bound, and that a wrong tap, a wrong dilation or a missing softmax would be off by a hundred bounds.

Kernel-name and regime assertions hold for the default tuning and are skipped under a recurrent tuning knob (the forced runs of
tests/test_gpu_families.py); parity assertions never are.  A dense-tail case beyond the lane = stream kernels' LDS bound has no kernel
under the knobs that force those kernels and skips there.

Every test prints the distance it measured beside its bound before it asserts (`-s` / `-rP` shows them)."""
import os

import numpy as np
import pytest

import na_oracle as O
import recurrent_cases as RC
import tail_cases as TC

pytestmark = pytest.mark.gpu

NANO = "BossWN-nano.nam"
RT = "RecurrentWaveRtKernel"


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


_built = {}


def built(c):
    if c["name"] not in _built:
        _built[c["name"]] = TC.Built(c)
    return _built[c["name"]]


_wants = {}


def want64(c, x, key, prewarm):
    """The float64 walk of the case for signal x: computed once per key, shared between the tests, never changed."""
    key = (c["name"], bool(prewarm)) + tuple(key)
    if key not in _wants:
        w = built(c).f64(x, prewarm=prewarm)
        w.setflags(write=False)
        _wants[key] = (x.copy(), w)
    assert np.array_equal(_wants[key][0], x), key
    return _wants[key][1]


def runnable(na, c):
    """The kernel that runs the case under this process's tuning knobs; a forced run skips a case that no kernel takes there."""
    name = TC.kernel_under_knobs(na, c)
    if not name:
        assert RC.knob_set() and c["form"] == "dense", (c["name"], "no kernel by default")
        pytest.skip("beyond the lane = stream kernels' LDS bound")
    return name


def assert_listed(m, c):
    """Default tuning: the case runs on the kernel and in the regime it is listed for."""
    if RC.knob_set():
        return
    p, runs = m.RecurrentPlan(), c["runs"]
    assert p["runs"] == (runs["kernel"] == RT), (c["name"], p)
    if "waves" in runs:
        assert (p["waves"] == 1) == (runs["waves"] == "one"), (c["name"], p)
    if "l2w" in runs:
        assert int(p["l2w"]) == runs["l2w"], (c["name"], p)


def bit_equal(got, want, what):
    assert np.array_equal(got, want), (what, int(np.argmax(got != want)), int(np.count_nonzero(got != want)), O.rms(got - want))


def run_batch(batch, x, sizes):
    return RC.run_in_calls(lambda chunk: batch.Process(np.ascontiguousarray(chunk)), x, sizes)


def alone(na, m, x, sizes, prewarm):
    one = na.Batch(0)
    one.AddStreams(m, 1, doPrewarm=prewarm)
    y = run_batch(one, x[None, :], sizes)[0]
    one.close()
    return y


def within(c, got, want, what):
    err, bd = O.rms(got - want), TC.bound(want)
    print("%-28s %-22s GPU-float64 rms %.3g, bound %.3g (%.3f of it), rms(want) %.3g" % (c["name"], what, err, bd, err / bd, O.rms(want)))
    assert np.all(np.isfinite(got)), (c["name"], what)
    assert err <= bd, (c["name"], what, err, bd)
    return err


# ---------------------------------------------------------------------------------------------------------------- (a) one stream

@pytest.mark.parametrize("c", TC.cases(), ids=TC.case_id)
def test_case_matches_the_float64_stack(na, c):
    """One stream through the case's call partition: 1, 1, 2, 3, then 129 and 300 (launches chunk at 128), 63 .. 128 and hist - 1, hist,
    hist + 1 in a seeded order, over at least 3 hist + 300 samples so that every history row turns over."""
    runnable(na, c)
    b = built(c)
    m = b.load(na)
    assert_listed(m, c)
    x = TC.signal(c)
    y = RC.run_in_calls(m.Process, x, b.sizes())
    within(c, y, want64(c, x, ("stream", 0), c["prewarm"]), "one stream")
    m.close()


@pytest.mark.parametrize("c", TC.next_up_cases(), ids=TC.case_id)
def test_next_size_above_the_widest_conv_tail_input_is_refused_or_right(na, c):
    """One unit more than the widest recurrent layer the shape predicate admits in front of a conv1d layer: never silently different."""
    b = TC.Built(c)
    try:
        m = na.NeuralModelLoader().CreateFromString(b.doc, ".json", doPrewarm=False)
    except na.NeuralAudioError as e:
        assert "is not supported" in str(e), (c["name"], e)
        return
    assert m is not None, c["name"]
    x = TC.signal(c)
    within(c, RC.run_in_calls(m.Process, x, b.sizes()), b.f64(x, prewarm=False), "next size up")


def test_softmax_over_one_unit_is_constant_one(na):
    """softmax across a conv1d layer of ONE unit is 1 whatever the input: the dense layer behind it gives w + b for every sample, also
    for an input at amplitude 1000 (kept out of the case table: its output cannot depend on its input)."""
    c = dict(name="conv-softmax-1", spec=TC.SOFTMAX_ONE, seed=61, gain=TC.GAIN, bias_scale=TC.BIAS_SCALE, prewarm=False, hist=5, samples=916)
    b = TC.Built(c)
    m = b.load(na)
    last = b.mj["layers"][-1]["weights"]
    for amp in (1.0, 1000.0):
        x = TC.signal(c, amp)
        want = b.f64(x)
        assert np.allclose(want, last[0][0][0] + last[1][0], rtol=0, atol=1e-12)
        within(c, RC.run_in_calls(m.Process, x, TC.call_sizes(c["samples"], c["hist"], 3)), want, "amplitude %g" % amp)
    m.close()


# ---------------------------------------------------------------------------------------------------------------- (b) three streams

@pytest.mark.parametrize("c", TC.cases(), ids=TC.case_id)
def test_case_in_a_batch_of_three_matches_float64_and_the_stream_alone(na, c):
    """Three streams with different inputs in one batch: every row is within the bound of its own float64 walk and equals the same model
    run alone on the same inputs and call sizes bit for bit (slot and capacity indexing of the conv1d history rows)."""
    name = runnable(na, c)
    b = built(c)
    m = b.load(na)
    pw, sizes = c["prewarm"], b.sizes()
    x = np.stack([TC.signal(c, stream=r) for r in range(3)])
    batch = na.Batch(0)
    assert batch.AddStreams(m, 3, doPrewarm=pw) == 0
    assert batch.StreamKernelName(2) == name and (RC.knob_set() or name == c["runs"]["kernel"]), (c["name"], batch.StreamKernelName(2), name)
    y = run_batch(batch, x, sizes)
    batch.close()
    for r in range(3):
        within(c, y[r], want64(c, x[r], ("stream", r), pw), "row %d of 3" % r)
        bit_equal(y[r], alone(na, m, x[r], sizes, pw), (c["name"], r))
    m.close()


# ---------------------------------------------------------------------------------------------------------------- (c) growth

@pytest.mark.parametrize("name", TC.GROWTH_CASES)
def test_batch_growing_past_its_first_capacity_keeps_the_tail_history(na, name):
    """60 streams run a 70-sample call, ten more join -- more than the first capacity of 64 state columns, so the state of the live
    streams, conv1d history rows included, is re-strided -- and ragged calls follow.  Every one of the 70 rows matches its own float64
    walk; the joiners from the join onwards, against a fresh walk with zero history."""
    c = TC.by_name(name)
    kernel = runnable(na, c)
    assert c["hist"] <= 64
    m = built(c).load(na, prewarm=False)
    n1, later = 70, [1, 129, c["hist"] + 1, 50]
    x = np.stack([TC.signal(c, stream=200 + r, samples=n1 + sum(later)) for r in range(70)])
    batch = na.Batch(0)
    assert batch.AddStreams(m, 60, doPrewarm=False) == 0
    y1 = batch.Process(np.ascontiguousarray(x[:60, :n1]))
    assert batch.AddStreams(m, 10, doPrewarm=False) == 60
    assert batch.StreamKernelName(69) == kernel
    y2 = run_batch(batch, x[:, n1:], later)
    batch.close()
    worst = 0.0
    for r in range(70):
        got, xin = (np.concatenate([y1[r], y2[r]]), x[r]) if r < 60 else (y2[r], x[r, n1:])
        want = built(c).f64(xin, prewarm=False)
        err = O.rms(got - want)
        worst = max(worst, err / TC.bound(want))
        assert np.all(np.isfinite(got)) and err <= TC.bound(want), (name, r, err, TC.bound(want))
    print("%-28s 70 rows across the growth: worst GPU-float64 rms is %.3f of its bound" % (name, worst))
    m.close()


# ---------------------------------------------------------------------------------------------------------------- (d) leave and join

def test_recycled_slots_carry_nothing_of_the_leavers_conv_history(na):
    """Seven streams of a conv-tail case run 100 samples, streams 1 and 4 leave, three join one by one (ids 1, 4 and a new row 7).  The
    joiners equal a fresh stream's float64 walk -- nothing of a leaver's history survives in the recycled column -- and the stayers their
    uninterrupted walk; every row equals the same model alone on the same inputs and call sizes bit for bit."""
    c = TC.by_name(TC.LEAVE_JOIN_CASE)
    runnable(na, c)
    b = built(c)
    m = b.load(na)
    pw = c["prewarm"]
    first, later = [100], [1, 3, 129, c["hist"] - 1, 64, 65, 38]
    n1, n2 = sum(first), sum(later)
    x = np.stack([TC.signal(c, stream=300 + r, samples=n1 + n2) for r in range(8)])
    batch = na.Batch(0)
    assert batch.AddStreams(m, 7, doPrewarm=pw) == 0
    y1 = run_batch(batch, x[:7, :n1], first)
    batch.RemoveStreams(1)
    batch.RemoveStreams(4)
    assert [batch.AddStreams(m, 1, doPrewarm=pw) for _ in range(3)] == [1, 4, 7]
    assert batch.NumStreams() == 8 and batch.StreamKernelName(7) == RT
    y2 = run_batch(batch, x[:, n1:], later)
    batch.close()
    for r in range(8):
        if r in (1, 4, 7):
            got, xin, sizes, what = y2[r], x[r, n1:], later, "joiner %d" % r
        else:
            got, xin, sizes, what = np.concatenate([y1[r], y2[r]]), x[r], first + later, "stayer %d" % r
        within(c, got, b.f64(xin), what)
        bit_equal(got, alone(na, m, xin, sizes, pw), (c["name"], r))
    m.close()


# ---------------------------------------------------------------------------------------------------------------- (e) mixed launch list

def test_two_conv_tails_and_a_dense_tail_beside_an_lstm_and_a_wavenet(na):
    """Two different conv-tail models, a dense-tail model, a tail-less LSTM 1x65 and a Nano WaveNet in one batch, two streams each,
    interleaved rows, ragged calls with one above 128: every tail row equals its model alone bit for bit and is within the bound of
    float64; the others match their oracles."""
    loader = na.NeuralModelLoader()
    tails = [TC.by_name(n) for n in TC.MIXED_CASES]
    for c in tails:
        runnable(na, c)
    mt = [built(c).load(na, prewarm=False) for c in tails]  # (the tails from a reset state, the other two models prewarmed)
    cl = RC.small_case("lstm", 1, 65)
    bl = RC.Built(cl)
    ml, mw = bl.load(na, loader), loader.CreateFromFile(os.path.join(O.MODELS_DIR, NANO))
    order = [mt[0], mw, mt[1], ml, mt[2], mt[1], mw, mt[0], ml, mt[2]]
    batch = na.Batch(0)
    for r, m in enumerate(order):
        assert batch.AddStreams(m, 1, doPrewarm=m not in mt) == r
    sizes = [1, 2, 128, 129, 63, 77, 65]
    x = np.stack([O.signal_noise(sum(sizes), 700 + r) for r in range(len(order))])
    y = run_batch(batch, x, sizes)
    batch.close()
    for r, m in enumerate(order):
        if m in mt:
            c = tails[mt.index(m)]
            within(c, y[r], built(c).f64(x[r], prewarm=False), "mixed batch row %d" % r)
            bit_equal(y[r], alone(na, m, x[r], sizes, False), (c["name"], r))
        else:
            want = bl.oracle(True).process(x[r]) if m is ml else O.oracle_from_file(NANO).process(x[r])
            assert O.rms(y[r] - want) <= RC.bound(want), (r, O.rms(y[r] - want))


# ---------------------------------------------------------------------------------------------------------------- (f) in place

@pytest.mark.parametrize("name", TC.IN_PLACE_CASES)
def test_device_buffers_in_place_give_the_bits_of_the_out_of_place_run(na, name):
    """NA_BatchProcessDevice with the output rows equal to the input rows (torch tensors): the kernels have read a row's input before
    they write its output, so the bits are those of the run into a buffer of its own -- which is within the bound of float64."""
    import torch
    c = TC.by_name(name)
    runnable(na, c)
    dev = torch.device("cuda", 0)
    m = built(c).load(na)
    sizes = [1, 3, 129, 64, 128, 65]
    x = np.stack([TC.signal(c, stream=400 + r, samples=sum(sizes)) for r in range(3)])
    outs = []
    for in_place in (False, True):
        batch = na.Batch(0)
        batch.AddStreams(m, 3, doPrewarm=c["prewarm"])
        rows, pos = [], 0
        for n in sizes:
            din = torch.from_numpy(np.ascontiguousarray(x[:, pos:pos + n])).to(dev)
            dout = din if in_place else torch.zeros_like(din)
            torch.cuda.synchronize(dev)
            batch.ProcessDevice(din.data_ptr(), dout.data_ptr(), n, n, n)
            batch.Synchronize()
            rows.append(dout.cpu().numpy())
            pos += n
        batch.close()
        outs.append(np.concatenate(rows, axis=1))
    for r in range(3):
        bit_equal(outs[1][r], outs[0][r], (name, "in place", r))
        within(c, outs[0][r], built(c).f64(x[r]), "device buffers row %d" % r)
    m.close()


# ---------------------------------------------------------------------------------------------------------------- (g) levels

@pytest.mark.parametrize("amp", TC.LEVELS)
@pytest.mark.parametrize("name", TC.LEVEL_CASES)
def test_level_stays_within_tolerance_of_the_float64_stack(na, name, amp):
    """Amplitudes 1e-5, 30 and 1000 on cases whose tails hold elu, sigmoid, softmax and tanh layers: finite, and within the bound."""
    c = TC.by_name(name)
    runnable(na, c)
    b = built(c)
    m = b.load(na)
    x = TC.signal(c, amp)
    y = RC.run_in_calls(m.Process, x, b.sizes())
    within(c, y, want64(c, x, ("amplitude", amp), c["prewarm"]), "amplitude %g" % amp)
    m.close()


# ---------------------------------------------------------------------------------------------------------------- (h) lane = stream

LANE_CALLS = [1, 129, 70]


@pytest.mark.parametrize("streams", TC.LANE_STREAMS)
@pytest.mark.parametrize("name", TC.LANE_CASES)
def test_dense_tail_with_softmax_at_stream_counts_around_a_workgroup_of_lanes(na, name, streams):
    """1, 3, 64, 65 and 130 streams of an LSTM and a GRU with a dense tail that holds a softmax layer; the first, the 64th, the 65th and
    the last row against float64.  By default one workgroup of RecurrentWaveRtKernel per stream; under NA_LSTM_NO_WAVE_RT /
    NA_LSTM_LANE_KERNEL the lane = stream kernels (LstmGenericKernel / GruGenericKernel): 64 streams per workgroup, idle lanes in the
    last one."""
    c = TC.by_name(name)
    kernel = runnable(na, c)
    m = built(c).load(na)
    pw = c["prewarm"]
    x = np.stack([TC.signal(c, stream=500 + r, samples=sum(LANE_CALLS)) for r in range(streams)])
    batch = na.Batch(0)
    assert batch.AddStreams(m, streams, doPrewarm=pw) == 0
    assert batch.StreamKernelName(streams - 1) == kernel and (RC.knob_set() or kernel == RT), (batch.StreamKernelName(streams - 1), kernel)
    y = run_batch(batch, x, LANE_CALLS)
    batch.close()
    assert np.all(np.isfinite(y))
    for r in sorted({0, 63, 64, streams - 1}):
        if r < streams:
            within(c, y[r], want64(c, x[r], ("lane", r), pw), "row %d of %d" % (r, streams))
    m.close()
