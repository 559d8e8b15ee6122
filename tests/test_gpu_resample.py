"""GPU tests of batch resampling (NA_BatchSetResampling, csrc/resample.cpp, csrc/resample_kernels.hip).

The float64 reference is this file's own numpy restatement of the contract:
  up    u[j]   = te * sum_i x[i] * h[j * tm - i * te]           x[i] = 0 for i < 0
  down  out[k] = tm * sum_j v[j] * h[k * te - S - j * tm]       v[j] = 0 for j < 0, S = (q - 1) * tm + pad
with the SHIPPED f32 prototype h (NA_ResamplePrototype) widened to double, so only rounding is judged here (the design itself is judged
by tests/test_resample_cpu.py).  Each stage is held to the worst-case rounding bound of an f32 dot product of its length,
taps * 2^-24 * max over phases of sum |gain * h| * peak |input of the stage|, computed below, not typed in; the model between the stages
is pinned bit for bit against an ordinary batch fed the tapped model-rate input (NA_DebugResampleTap)."""
import ctypes as C
import math
import os
import time

import numpy as np
import pytest

import na_oracle as O
import wide_cases as WC

pytestmark = pytest.mark.gpu

FE, FM = 44100, 48000
T = 48
KNOBS = ("NA_WN_KERNEL", "NA_WN_SPEC", "NA_WN_PACK", "NA_WN_DENSE")


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


_loaders = []


def _model(na, name, quality=1.0, external_rate=None, opt_in=False, prewarm=False):
    loader = na.NeuralModelLoader()
    loader.SetDefaultQualityScaleFactor(quality)
    if external_rate is not None:
        loader.SetExternalSampleRate(external_rate)
    if opt_in:
        loader.SetResampleToExternalRate(True)
    if name == "wide-40/20":  # a synthetic model of the runtime-shaped kernels (layer arrays wider than 16 channels)
        arrays = WC.two_array(40, 20)
        m = loader.CreateFromString(O.nam_json_wavenet_generic(arrays, O.synth_wavenet_weights(arrays, seed=40)), ".nam", doPrewarm=prewarm)
    else:
        m = loader.CreateFromFile(os.path.join(O.MODELS_DIR, name), doPrewarm=prewarm)
    assert m is not None
    _loaders.append(loader)
    return m


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _calls(total, lengths):
    """(offset, length) pairs that cut `total` samples into calls of the given lengths (the last one shortened)"""
    out, pos, i = [], 0, 0
    while pos < total:
        n = min(int(lengths[i % len(lengths)]), total - pos)
        out.append((pos, n))
        pos += n
        i += 1
    return out


def _run(batch, x, lengths):
    x = np.atleast_2d(x)
    return np.concatenate([batch.Process(np.ascontiguousarray(x[:, a:a + n])) for a, n in _calls(x.shape[1], lengths)], axis=1)


# ---------------------------------------------------------------------------------------------------- the float64 stages

def _terms(fe, fm):
    g = math.gcd(fe, fm)
    return fm // g, fe // g


def _shift(te, tm, q):
    base = T * max(te, tm) + (q - 1) * tm
    pad = (-base) % te
    return (q - 1) * tm + pad


def _stage(sig, h, first_tick, step, period, gain, n_out):
    """out[o] = gain * sum_t h[phase + t * period] * sig[idx - t], (idx, phase) = divmod(first_tick + o * step, period); sig is 0 in front"""
    sig = np.asarray(sig, np.float64)
    K = h.size
    taps = (K - 1) // period + 1
    tick = first_tick + np.arange(n_out, dtype=np.int64) * step
    idx = tick // period
    phase = tick - idx * period
    t = np.arange(taps, dtype=np.int64)
    hidx = phase[:, None] + t[None, :] * period
    coef = np.where(hidx < K, h.astype(np.float64)[np.minimum(hidx, K - 1)], 0.0)
    sidx = idx[:, None] - t[None, :]
    assert n_out == 0 or sidx.max() < sig.shape[1], "the stage would read a sample that does not exist yet"
    vals = sig[:, np.maximum(sidx, 0)] * (sidx >= 0)
    return gain * np.einsum("rot,ot->ro", vals, coef)


def _up64(x, h, te, tm, frames):
    return _stage(np.nan_to_num(np.asarray(x, np.float64), nan=0.0), h, 0, tm, te, te, frames)


def _down64(v, h, te, tm, q, n_out):
    return _stage(v, h, -_shift(te, tm, q), te, tm, tm, n_out)


def _bound(h, period, gain, peak):
    taps = (h.size - 1) // period + 1
    worst = max(float(np.sum(np.abs(gain * h[p::period].astype(np.float64)))) for p in range(period))
    return taps * 2.0 ** -24 * worst * peak


def _tapped_run(batch, x, lengths):
    """the batch over x in calls; returns (y, u, v): outputs and the concatenated model-rate rows of every call"""
    ys, us, vs = [], [], []
    for a, n in _calls(x.shape[1], lengths):
        ys.append(batch.Process(np.ascontiguousarray(x[:, a:a + n])))
        u, v = batch.DebugResampleTap()
        us.append(u)
        vs.append(v)
    return np.concatenate(ys, axis=1), np.concatenate(us, axis=1), np.concatenate(vs, axis=1), [u.shape[1] for u in us]


# ---------------------------------------------------------------------------------------------------- 4

def test_equal_rates_change_nothing_bit_for_bit(na):
    m = _model(na, "BossWN-standard.nam")
    x = np.stack([O.signal_noise(128 * 6 + 37, 300 + s) for s in range(5)])
    plain, same = na.Batch(0), na.Batch(0)
    same.SetResampling(48000, 48000)
    assert same.ResampleInfo()["latency_samples"] == 0
    with pytest.raises(na.NeuralAudioError):
        plain.ResampleInfo()
    plain.AddStreams(m, 5)
    same.AddStreams(m, 5)
    for a, n in _calls(x.shape[1], [128]):
        blk = np.ascontiguousarray(x[:, a:a + n])
        assert np.array_equal(plain.Process(blk), same.Process(blk))
    plain.close()
    same.close()


# ---------------------------------------------------------------------------------------------------- 5

@pytest.mark.parametrize("q", [32, 1])
def test_each_stage_is_within_the_rounding_bound_of_its_dot_product_and_the_model_between_them_is_exact(na, q):
    """(i) tapped model input u against the float64 up stage of x; (ii) tapped model output v against an ordinary batch fed u in the same
    call lengths, bit for bit; (iii) the output against the float64 down stage of the GPU's own v.  The test prints the measured maxima
    beside their bounds (run with -s); a plain f32 numpy restatement of both stages sits 20-40 x under the bound, so a result within
    2 x of it is a defect to look into."""
    m = _model(na, "BossWN-standard.nam")
    S, n, calls = 8, 128, 40
    te, tm = _terms(FE, FM)
    h = na.resample_prototype(FE, FM)
    x = np.stack([O.signal_noise(n * calls, 500 + s) for s in range(S)])
    b = na.Batch(0)
    b.SetResampling(FE, FM, quantum=q, max_frames=n)
    info = b.ResampleInfo()
    assert (info["quantum"], info["te"], info["tm"]) == (q, te, tm)
    b.AddStreams(m, S)
    y, u, v, frames = _tapped_run(b, x, [n])
    assert frames == [na.resample_model_frames(FE, FM, q, n * (i + 1)) - na.resample_model_frames(FE, FM, q, n * i) for i in range(calls)]
    assert all(f % q == 0 for f in frames) and u.shape[1] == na.resample_model_frames(FE, FM, q, n * calls)
    if q == 32:
        assert set(frames) == {128, 160}
    # (i)
    err_up = float(np.max(np.abs(u - _up64(x, h, te, tm, u.shape[1]))))
    bound_up = _bound(h, te, te, float(np.max(np.abs(x))))
    # (iii)
    err_down = float(np.max(np.abs(y - _down64(v, h, te, tm, q, y.shape[1]))))
    bound_down = _bound(h, tm, tm, float(np.max(np.abs(v))))
    print("q=%d up: max err %.3g (bound %.3g, peak %.3g)  down: max err %.3g (bound %.3g, peak %.3g)"
          % (q, err_up, bound_up, np.max(np.abs(x)), err_down, bound_down, np.max(np.abs(v))))
    assert np.max(np.abs(v)) > 1e-3 and np.max(np.abs(y)) > 1e-3  # (the model really ran)
    assert err_up <= bound_up
    assert err_down <= bound_down
    # (ii)
    plain = na.Batch(0)
    plain.AddStreams(m, S)
    v_plain = np.concatenate([plain.Process(np.ascontiguousarray(u[:, a:a + f])) for a, f in
                              zip(np.cumsum([0] + frames[:-1]), frames) if f > 0], axis=1)
    assert np.array_equal(v_plain, v)
    plain.close()
    b.close()


# ---------------------------------------------------------------------------------------------------- 6

CHUNK_CASES = [("standard", [("BossWN-standard.nam", 1.0, 3)]), ("nano-packed", [("BossWN-nano.nam", 1.0, 8)]), ("a2-q0.3", [("BossWN-a2.nam", 0.3, 2)]),
               ("a2-q1.0", [("BossWN-a2.nam", 1.0, 2)]), ("lstm-1x16", [("BossLSTM-1x16.nam", 1.0, 3)]), ("wide-40/20", [("wide-40/20", 1.0, 2)]),
               ("mixed", [("BossWN-standard.nam", 1.0, 2), ("BossWN-nano.nam", 1.0, 4), ("BossWN-a2.nam", 0.3, 1), ("BossWN-a2.nam", 1.0, 1),
                          ("BossLSTM-1x16.nam", 1.0, 2)])]


@pytest.mark.parametrize("case,members", CHUNK_CASES, ids=[c[0] for c in CHUNK_CASES])
def test_the_output_does_not_depend_on_how_the_signal_is_cut_into_calls(na, case, members):
    models = [(_model(na, name, quality), quality, count) for name, quality, count in members]
    rows = sum(c for _, _, c in members)
    total = 6000
    x = np.stack([O.signal_noise(total, 700 + s) for s in range(rows)])
    rng = np.random.RandomState(6)

    def run(lengths):
        b = na.Batch(0)
        b.SetResampling(FE, FM, max_frames=300)
        for m, quality, count in models:
            b.AddStreams(m, count, quality=quality)
        if case == "nano-packed" and not any(os.environ.get(k) for k in KNOBS):
            assert b.StreamPackFactor(0) > 1
        y = _run(b, x, lengths)
        b.close()
        return y

    y128 = run([128])
    assert np.all(np.isfinite(y128)) and np.any(y128[:, 200:])
    assert np.array_equal(y128, run(list(rng.randint(1, 301, size=4000))))
    assert np.array_equal(y128, run([total]))


# ---------------------------------------------------------------------------------------------------- 7

def test_every_entry_point_gives_the_same_samples(na):
    import torch
    from neuralaudio_amd import capi
    lib = capi.load_library()
    m = _model(na, "BossWN-standard.nam")
    S, n, calls = 5, 128, 6
    x = np.stack([O.signal_noise(n * calls, 900 + s) for s in range(S)])

    def fresh():
        b = na.Batch(0)
        b.SetResampling(FE, FM, max_frames=n)
        b.AddStreams(m, S)
        return b

    b = fresh()
    want = _run(b, x, [n])
    assert not b.UsesHalfLaunches() and not b.UsesResidentLaunch()
    b.close()
    assert np.any(want)

    # a registered block: the stages read and write the caller's rows in place
    b = fresh()
    block = np.zeros((2, S, n), dtype=np.float32)
    assert lib.NA_RegisterHostBuffer(block.ctypes.data_as(C.c_void_p), block.nbytes) == 0
    got = []
    for k in range(calls):
        block[0] = x[:, k * n:(k + 1) * n]
        block[1] = 7.0
        assert lib.NA_BatchProcess(b._h, _fp(block[0]), _fp(block[1]), n) == 0
        got.append(block[1].copy())
    assert lib.NA_UnregisterHostBuffer(block.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(np.concatenate(got, axis=1), want)
    b.close()

    # device pointers with strides, n in external samples (the resident launch is accepted and has no effect)
    b = fresh()
    b.SetResidentLaunch(True)
    dev = torch.device("cuda", 0)
    din = torch.zeros(S, 200, device=dev)
    dout = torch.full((S, 160), 7.0, device=dev)
    got = []
    for k in range(calls):
        din[:, :n] = torch.from_numpy(x[:, k * n:(k + 1) * n]).to(dev)
        torch.cuda.synchronize(dev)
        b.ProcessDevice(din.data_ptr(), dout.data_ptr(), n, 200, 160)
        b.Synchronize()
        assert not b.UsesHalfLaunches() and not b.UsesResidentLaunch()
        got.append(dout[:, :n].cpu().numpy())
        assert torch.all(dout[:, n:] == 7.0)
    assert np.array_equal(np.concatenate(got, axis=1), want)
    b.close()

    # Submit / Collect with two tickets in flight
    b = fresh()
    got, pending = [], []
    for k in range(calls):
        pending.append(b.Submit(x[:, k * n:(k + 1) * n]))
        if len(pending) == 2:
            got.append(b.Collect(pending.pop(0)))
    while pending:
        got.append(b.Collect(pending.pop(0)))
    assert np.array_equal(np.concatenate(got, axis=1), want)
    b.close()

    # NextInput / OutputView
    b = fresh()
    got = []
    for k in range(calls):
        b.NextInput(n)[:] = x[:, k * n:(k + 1) * n]
        got.append(b.CollectView(b.SubmitInput(n)).copy())
    assert np.array_equal(np.concatenate(got, axis=1), want)
    b.close()


def test_the_loader_opt_in_is_a_resampling_batch_of_one_and_without_it_nothing_changes(na):
    n, calls = 128, 8
    x = O.signal_noise(n * calls, 41)
    m48 = _model(na, "BossWN-standard.nam", prewarm=True)
    assert m48.GetModelProcessRate() == 48000 and m48.GetProcessLatencySamples() == 0
    b = na.Batch(0)
    b.SetResampling(FE, FM, max_frames=n)
    b.AddStreams(m48, 1)
    want = _run(b, x[None, :], [n])[0]
    latency = b.ResampleInfo()["latency_samples"]
    b.close()
    opted = _model(na, "BossWN-standard.nam", external_rate=FE, opt_in=True, prewarm=True)
    assert opted.GetProcessLatencySamples() == latency == na.resample_plan(FE, FM)["latency_samples"]
    got = np.concatenate([opted.Process(x[k * n:(k + 1) * n]) for k in range(calls)])
    assert np.array_equal(got, want)
    # the same external rate WITHOUT the opt-in: today's behaviour, the model runs as loaded for 48 kHz
    plain = _model(na, "BossWN-standard.nam", external_rate=FE, prewarm=True)
    assert plain.GetProcessLatencySamples() == 0
    y_plain = np.concatenate([plain.Process(x[k * n:(k + 1) * n]) for k in range(calls)])
    y_48 = np.concatenate([m48.Process(x[k * n:(k + 1) * n]) for k in range(calls)])
    assert np.array_equal(y_plain, y_48)
    assert not np.array_equal(y_plain, got)
    # a whole multiple is still served by the dilations, opt-in or not; an LSTM is not oversampled and resamples with the opt-in
    wn96 = _model(na, "BossWN-standard.nam", external_rate=96000, opt_in=True)
    assert wn96.GetModelProcessRate() == 96000 and wn96.GetProcessLatencySamples() == 0
    lstm96 = _model(na, "BossLSTM-1x16.nam", external_rate=96000, opt_in=True)
    assert lstm96.GetModelProcessRate() == 48000
    assert lstm96.GetProcessLatencySamples() == na.resample_plan(96000, 48000)["latency_samples"] > 0
    assert np.all(np.isfinite(lstm96.Process(O.signal_noise(300, 5))))


# ---------------------------------------------------------------------------------------------------- 8

def test_streams_that_join_recycle_or_prewarm_start_from_zero_histories_at_the_batchs_phase(na):
    m = _model(na, "BossWN-standard.nam")
    n, first_calls = 128, 37
    xs = np.stack([O.signal_noise(n * 80, 1100 + s) for s in range(7)])
    z = O.signal_noise(n * 80, 1200)
    za, zb = O.signal_noise(n * 80, 1201), O.signal_noise(n * 80, 1202)

    def batch(count):
        b = na.Batch(0)
        b.SetResampling(FE, FM, max_frames=n)
        b.AddStreams(m, count)
        return b

    A, B, A0 = batch(7), batch(1), batch(7)
    pos = 0

    def step(calls, a_extra, b_extra):
        """`calls` calls of n on all three batches; a_extra / b_extra: the signal of the joined stream in A / B (None: not joined yet)"""
        nonlocal pos
        outs = ([], [], [])
        for _ in range(calls):
            sl = slice(pos, pos + n)
            outs[0].append(A.Process(xs[:, sl] if a_extra is None else np.vstack([xs[:, sl], a_extra[None, sl]])))
            outs[1].append(B.Process(xs[:1, sl] if b_extra is None else np.vstack([xs[:1, sl], b_extra[None, sl]])))
            outs[2].append(A0.Process(xs[:, sl]))
            pos += n
        return [np.concatenate(o, axis=1) for o in outs]

    yA, yB, yA0 = step(first_calls, None, None)
    assert np.array_equal(yA, yA0) and np.array_equal(yA[0], yB[0])
    # a stream joins each batch and gets the same signal: same rows from then on; the neighbours never notice
    assert A.AddStreams(m, 1) == 7 and B.AddStreams(m, 1) == 1
    yA, yB, yA0 = step(12, z, z)
    assert np.any(yA[7]) and np.array_equal(yA[7], yB[1])
    assert np.array_equal(yA[:7], yA0)
    # a joiner is not a stream that was there from the start (its histories are zero, the batch's phase is not)
    fresh = batch(1)
    y_fresh = _run(fresh, z[None, first_calls * n:(first_calls + 12) * n], [n])
    fresh.close()
    assert not np.array_equal(y_fresh[0], yA[7])
    # different signals, then remove + recycle: both start from zero histories again
    yA, yB, yA0 = step(5, za, zb)
    assert not np.array_equal(yA[7], yB[1]) and np.array_equal(yA[:7], yA0)
    A.RemoveStreams(7, 1)
    B.RemoveStreams(1, 1)
    assert A.AddStreams(m, 1) == 7 and B.AddStreams(m, 1) == 1
    yA, yB, yA0 = step(8, z, z)
    assert np.any(yA[7]) and np.array_equal(yA[7], yB[1]) and np.array_equal(yA[:7], yA0)
    # different signals again, then Prewarm(stream): zero histories, the neighbours carry on
    yA, yB, yA0 = step(5, za, zb)
    assert not np.array_equal(yA[7], yB[1])
    A.Prewarm(7)
    B.Prewarm(1)
    yA, yB, yA0 = step(8, z, z)
    assert np.array_equal(yA[7], yB[1]) and np.array_equal(yA[:7], yA0)
    for b in (A, B, A0):
        b.close()


def test_a_quality_switch_keeps_the_filter_histories(na):
    m = _model(na, "BossWN-a2.nam", quality=0.3)
    n = 128
    te, tm = _terms(FE, FM)
    h = na.resample_prototype(FE, FM)
    x = np.stack([O.signal_noise(n * 24, 1300 + s) for s in range(2)])
    b = na.Batch(0)
    b.SetResampling(FE, FM, max_frames=n)
    q = b.ResampleInfo()["quantum"]
    b.AddStreams(m, 2, quality=0.3)
    y1, _, v1, _ = _tapped_run(b, x[:, :n * 12], [n])
    first = b.GetActiveSubModel(0)
    b.SetQuality(0, 1.0)
    assert b.GetActiveSubModel(0) != first
    y2, _, v2, _ = _tapped_run(b, x[:, n * 12:], [n])
    y, v = np.concatenate([y1, y2], axis=1), np.concatenate([v1, v2], axis=1)
    err = float(np.max(np.abs(y - _down64(v, h, te, tm, q, y.shape[1]))))
    bound = _bound(h, tm, tm, float(np.max(np.abs(v))))
    print("across the switch: max err %.3g (bound %.3g)" % (err, bound))
    assert np.max(np.abs(v2)) > 1e-4 and err <= bound
    b.close()


# ---------------------------------------------------------------------------------------------------- 9

def test_refusals(na):
    m = _model(na, "BossWN-standard.nam")
    b = na.Batch(0)
    b.AddStreams(m, 1)
    with pytest.raises(na.NeuralAudioError, match="before the first AddStreams"):
        b.SetResampling(FE, FM)
    blob = b.SaveStreams([0])  # snapshots of an ordinary batch are untouched
    b.LoadStreams([0], blob)
    b.close()

    r = na.Batch(0)
    with pytest.raises(na.NeuralAudioError, match="quantum"):
        r.SetResampling(FE, FM, quantum=3)
    with pytest.raises(na.NeuralAudioError, match="640"):
        r.SetResampling(44101, FM)
    r.SetResampling(FE, FM)
    m96 = _model(na, "BossWN-standard.nam", external_rate=96000)
    assert m96.GetModelProcessRate() == 96000
    with pytest.raises(na.NeuralAudioError) as e:
        r.AddStreams(m96, 1)
    assert "96000" in str(e.value) and "48000" in str(e.value)
    assert r.NumStreams() == 0
    r.AddStreams(m, 2)
    with pytest.raises(na.NeuralAudioError, match="resampling batch"):
        r.SaveStreams([0])
    with pytest.raises(na.NeuralAudioError, match="resampling batch"):
        r.LoadStreams([0], blob)
    r.close()


def test_a_nan_sample_reads_as_silence_before_the_filter(na):
    m = _model(na, "BossWN-standard.nam")
    n = 128
    x0 = np.stack([O.signal_noise(n * 6, 1400 + s) for s in range(2)])
    x0[0, 300] = 0.0
    x0[1, 5] = 0.0
    xn = x0.copy()
    xn[0, 300] = np.nan
    xn[1, 5] = np.nan
    outs = []
    for x in (x0, xn):
        b = na.Batch(0)
        b.SetResampling(FE, FM, max_frames=n)
        b.AddStreams(m, 2)
        outs.append(_run(b, x, [n]))
        b.close()
    assert np.all(np.isfinite(outs[1])) and np.array_equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------- 10

def test_a_stalled_device_breaks_a_resampling_batch_like_any_other(na):
    """One case of tests/test_gpu_stall.py on a resampling batch: the blocking call gives up at the limit and returns silence."""
    import torch
    from neuralaudio_amd import capi
    lib = capi.load_library()
    limit_ms, stall_ms = 100.0, 1200.0
    m = _model(na, "BossWN-standard.nam")
    S, n = 16, 128
    b = na.Batch(0)
    b.SetResampling(FE, FM, max_frames=n)
    b.AddStreams(m, S)
    x = np.stack([O.signal_sine(n, start=977 * s) for s in range(S)]).astype(np.float32)
    for _ in range(3):
        y_ok = b.Process(x)
    assert np.any(y_ok)
    b.SetWaitLimitMs(limit_ms)
    b.DebugStallDevice(stall_ms)
    y = np.full_like(x, 7.0)
    t0 = time.monotonic()
    rc = lib.NA_BatchProcess(b._h, _fp(x), _fp(y), n)
    dt = time.monotonic() - t0
    assert rc != 0 and "did not answer within" in capi.last_error()
    assert limit_ms / 1000.0 * 0.8 <= dt < limit_ms / 1000.0 + 0.4, dt
    assert not np.any(y) and b.IsBroken()
    assert lib.NA_BatchProcess(b._h, _fp(x), _fp(y), n) != 0 and "broken" in capi.last_error()
    b.close()
    time.sleep(stall_ms / 1000.0)
    torch.cuda.synchronize()
