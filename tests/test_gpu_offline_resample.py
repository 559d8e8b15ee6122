"""GPU tests of offline rendering at an external rate (NA_RenderOfflineAtRate, csrc/offline_render.cpp,
csrc/offline_resample_kernels.hip).

The contract: with plan = NA_ResamplePlan(Fe, Fm, quantum 1), L its latency, N the job's samples and M = J(N + L) model frames,
out[k] = s[k + L], s what a fresh resampling batch of one prewarmed stream returns for x ++ zeros(L).  Three kinds of check:
  * each resampling stage against this file's float64 restatement (the helpers of tests/test_gpu_resample.py, copied: the SHIPPED f32
    prototype widened to double, so only rounding is judged), held to the worst-case rounding bound of an f32 dot product of its length,
    computed below, not typed in; the model between the stages bit for bit against NA_RenderOffline of the tapped model-rate input
  * the whole call bit for bit against the streaming batch where both run the stream on the same kernel
  * alignment: the latency compensation, by a shifted impulse (bit for bit) and by the envelope peak of a burst against the 48 kHz render."""
import json
import math
import os
import time

import numpy as np
import pytest

import na_oracle as O

pytestmark = pytest.mark.gpu

FE, FM = 44100, 48000
T = 48
TOL_RMS = 2e-6


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


def _model(na, name, quality=1.0, rate=None, opt_in=False, prewarm=False):
    loader = na.NeuralModelLoader()
    loader.SetDefaultQualityScaleFactor(quality)
    if rate:
        loader.SetExternalSampleRate(rate)
    if opt_in:
        loader.SetResampleToExternalRate(True)
    m = loader.CreateFromFile(os.path.join(O.MODELS_DIR, name), doPrewarm=prewarm)
    assert m is not None
    m._loader = loader  # (keeps the loader alive as long as the model)
    return m


def _a1_at(na, rate, seed=7):
    """a synthetic A1 Nano whose file says `rate`"""
    arrays = O.a1_arrays(4, 2)
    doc = json.loads(O.nam_json_wavenet_a1(4, 2, O.synth_wavenet_weights(arrays, seed=seed)))
    doc["sample_rate"] = rate
    loader = na.NeuralModelLoader()
    m = loader.CreateFromString(json.dumps(doc), ".nam", doPrewarm=False)
    assert m is not None and m.GetModelProcessRate() == rate
    m._loader = loader
    return m


def _calls(total, lengths):
    """(offset, length) pairs that cut `total` samples into calls of the given lengths (the last one shortened)"""
    out, pos, i = [], 0, 0
    while pos < total:
        n = min(int(lengths[i % len(lengths)]), total - pos)
        out.append((pos, n))
        pos += n
        i += 1
    return out


def _streaming(na, m, x, fe, quality=1.0, lengths=(128, 1, 300, 2048, 77, 3000, 129)):
    """the contract's reference: a one-stream batch with SetResampling(fe, Fm, quantum 1) and a prewarmed stream, fed x ++ zeros(L) in
    calls of mixed lengths, the first L outputs dropped; returns (out, kernel of the stream)"""
    fm = m.GetModelProcessRate()
    b = na.Batch(0)
    b.SetResampling(fe, fm, quantum=1, max_frames=2048)
    b.AddStreams(m, 1, quality=quality, doPrewarm=True)
    L = b.ResampleInfo()["latency_samples"]
    z = np.concatenate([x, np.zeros(L, np.float32)])[None, :]
    y = np.concatenate([b.Process(np.ascontiguousarray(z[:, a:a + n])) for a, n in _calls(z.shape[1], lengths)], axis=1)[0]
    kernel = b.StreamKernelName(0)
    b.close()
    return y[L:], kernel


# ---------------------------------------------------------------------------------------------------- the float64 stages
# (copied from tests/test_gpu_resample.py)

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


def _check_stages_and_model(na, m, x, fe, quality=1.0, ran=True, **options):
    """checks (1) and (2) of one render: the two stages within their rounding bounds, the model between them exact; returns (out, u, v)"""
    fm = m.GetModelProcessRate()
    te, tm = _terms(fe, fm)
    h = na.resample_prototype(fe, fm)
    L = na.resample_plan(fe, fm, 1)["latency_samples"]
    N = x.size
    M = na.resample_model_frames(fe, fm, 1, N + L)
    out, u, v = na.debug_render_tap(m, x, quality, external_rate=fe, **options)
    assert out.shape == x.shape and u.shape == (M,) and v.shape == (M,)
    z = np.concatenate([x, np.zeros(L, np.float32)])[None, :]
    err_up = float(np.max(np.abs(u - _up64(z, h, te, tm, M)[0])))
    bound_up = _bound(h, te, te, float(np.max(np.abs(x))))
    err_down = float(np.max(np.abs(out - _down64(v[None, :], h, te, tm, 1, N + L)[0, L:L + N])))
    bound_down = _bound(h, tm, tm, float(np.max(np.abs(v))))
    print("%d -> %d Hz, N=%d M=%d L=%d  up: max err %.3g (bound %.3g, peak %.3g)  down: max err %.3g (bound %.3g, peak %.3g)"
          % (fe, fm, N, M, L, err_up, bound_up, np.max(np.abs(x)), err_down, bound_down, np.max(np.abs(v))))
    if ran:
        assert np.max(np.abs(v)) > 1e-3 and np.max(np.abs(out)) > 1e-3  # (the model really ran)
    assert err_up <= bound_up
    assert err_down <= bound_down
    # (2) the un-resampled call on the tapped input
    assert np.array_equal(v, na.render_offline(m, u, quality=quality, **options))
    return out, u, v


# ---------------------------------------------------------------------------------------------------- 1, 2

@pytest.mark.parametrize("n", [44100, 1, 30, 5000])
def test_each_stage_is_within_its_rounding_bound_and_the_model_between_them_is_exact(na, n):
    m = _model(na, "BossWN-standard.nam")
    x = O.signal_noise(n, seed=100 + n)
    if n < 100:  # (N = 1 and N < L: all of the output is filter tail)
        x = np.full(n, 0.5, np.float32)
    _check_stages_and_model(na, m, x, FE, ran=n >= 100, segment_samples=512)


def test_nan_reads_as_silence_and_infinities_as_the_largest_finite_value(na):
    m = _model(na, "BossWN-standard.nam")
    x = O.signal_noise(6000, seed=3)
    dirty = x.copy()
    dirty[1000], dirty[2000] = np.nan, np.nan
    clean = x.copy()
    clean[1000], clean[2000] = 0.0, 0.0
    _, u_dirty, _ = na.debug_render_tap(m, dirty, external_rate=FE)
    _, u_clean, _ = na.debug_render_tap(m, clean, external_rate=FE)
    assert np.array_equal(u_dirty, u_clean)
    dirty[3000], clean[3000] = np.inf, 3.0e38
    dirty[4000], clean[4000] = -np.inf, -3.0e38
    _, u_dirty, _ = na.debug_render_tap(m, dirty, external_rate=FE)
    _, u_clean, _ = na.debug_render_tap(m, clean, external_rate=FE)
    assert np.array_equal(u_dirty, u_clean, equal_nan=True)


# ---------------------------------------------------------------------------------------------------- 3

CASES = [("BossWN-standard.nam", 1.0), ("BossWN-nano.nam", 1.0), ("BossWN-a2.nam", 0.0), ("BossWN-a2.nam", 1.0), ("BossLSTM-1x16.nam", 1.0),
         ("synthetic_gru_1x16.json", 1.0)]


@pytest.mark.parametrize("name,quality", CASES)
def test_the_render_equals_the_streaming_batch(na, name, quality):
    """Dozens of segment boundaries (segmentSamples = 512 over one second): bit-identical to the streaming batch where the segment batch
    and the batch of one run the stream on the same kernel, within the kernels' tolerance of it in every case."""
    m = _model(na, name, quality)
    x = O.signal_noise(FE, seed=21)
    y = na.render_offline(m, x, quality=quality, segment_samples=512, external_rate=FE)
    plan = na.render_plan(m, x.size, quality=quality, segment_samples=512, external_rate=FE)
    ys, kernel = _streaming(na, m, x, FE, quality)
    assert y.shape == x.shape == ys.shape and np.all(np.isfinite(y))
    if plan["lead"] > 0:
        assert plan["segments"] >= 80
    same = plan["kernel"] == kernel
    print("%s q=%g: %s" % (name, quality, "bit-identical" if same else "tolerance (segment kernel %s, stream kernel %s)" % (plan["kernel"], kernel)))
    if same:
        assert np.array_equal(y, ys), (name, quality, plan, int(np.argmax(y != ys)))
    assert O.rms(y - ys) < TOL_RMS, (name, quality, plan)


# ---------------------------------------------------------------------------------------------------- 4

@pytest.mark.parametrize("name", ["BossWN-standard.nam", "BossLSTM-1x16.nam"])
def test_equal_rates_give_the_plain_render_bit_for_bit(na, name):
    m = _model(na, name)
    x = O.signal_noise(30011, seed=4)
    assert na.render_plan(m, x.size, segment_samples=512, external_rate=48000)["resample"]["latency_samples"] == 0
    assert np.array_equal(na.render_offline(m, x, segment_samples=512, external_rate=48000), na.render_offline(m, x, segment_samples=512))
    out, u, v = na.debug_render_tap(m, x, external_rate=48000, segment_samples=512)
    assert np.array_equal(u, x) and np.array_equal(v, out)


# ---------------------------------------------------------------------------------------------------- 5

def test_a_model_loaded_at_96_khz_renders_at_88200_hz(na):
    m = _model(na, "BossWN-standard.nam", rate=96000)
    assert m.GetModelProcessRate() == 96000
    assert _terms(88200, 96000) == (160, 147)
    x = O.signal_noise(2 * 44100, seed=6)
    _check_stages_and_model(na, m, x, 88200, segment_samples=1024)


# ---------------------------------------------------------------------------------------------------- 6

def test_an_impulse_moved_by_one_phase_period_moves_the_output_by_exactly_that(na):
    """The phase period at 44.1 -> 48 kHz, quantum 1, is 147 external samples (160 model frames): the same impulse 147 samples later is the
    same arithmetic 147 samples later."""
    m = _model(na, "BossWN-standard.nam")
    N, i0 = 40000, 20000
    a, b = np.zeros(N, np.float32), np.zeros(N, np.float32)
    a[i0], b[i0 + 147] = 0.5, 0.5
    ya = na.render_offline(m, a, segment_samples=512, external_rate=FE)
    yb = na.render_offline(m, b, segment_samples=512, external_rate=FE)
    assert np.max(np.abs(ya - ya[0])) > 1e-3  # (the impulse came through)
    # The comparison starts behind the first `lead` model frames: until the rings have turned over once they hold the idle state as the
    # prewarm kernel rounded it, a few 1e-7 beside what the stream kernel itself settles on -- the start of every fresh prewarmed
    # stream, not a property of the position.  Everything after it, the whole response to the impulse included, is compared.
    p = na.render_plan(m, N, segment_samples=512, external_rate=FE)
    w = -(-(p["lead"] + p["resample"]["taps_down"]) * 147 // 160) + p["resample"]["latency_samples"]
    assert w < i0 - 4096
    assert np.array_equal(yb[147 + w:], ya[w:N - 147]), w + int(np.argmax(yb[147 + w:] != ya[w:N - 147]))
    # ... and not by anything else
    assert not np.array_equal(yb[146 + w:], ya[w:N - 146])


def _envelope_peak(y, rate):
    """position of the maximum of the analytic envelope of y minus its idle level (FFT Hilbert transform; parabola through the top three)"""
    y = np.asarray(y, np.float64)
    y = y - np.median(y)
    n = y.size
    spec = np.fft.fft(y)
    w = np.zeros(n)
    w[0] = 1.0
    w[1:(n + 1) // 2] = 2.0
    if n % 2 == 0:
        w[n // 2] = 1.0
    env = np.abs(np.fft.ifft(spec * w))
    # the envelope of a distorted burst carries ripple at the carrier's harmonics: smooth over one carrier period (1 ms at either rate)
    k = np.hanning(2 * (rate // 2000) + 1)
    env = np.convolve(env, k / k.sum(), mode="same")
    p = int(np.argmax(env))
    a, b, c = env[p - 1], env[p], env[p + 1]
    return p + 0.5 * (a - c) / (a - 2 * b + c)


def test_the_envelope_peak_of_a_burst_sits_where_the_48_khz_render_puts_it(na):
    """The same band-limited burst (a 1 kHz tone under a Gaussian of 1 ms) sampled at 44.1 and at 48 kHz: the rendered envelope peaks at
    the same TIME, i.e. within +-1 sample of the 48 kHz peak position scaled by 44.1 / 48.  An output that was not latency-compensated
    would sit L = 48 samples late."""
    m = _model(na, "BossWN-standard.nam")
    t0, sigma, f = 1.0 / 3.0, 1.0e-3, 1000.0

    def burst(rate, n):
        t = np.arange(n, dtype=np.float64) / rate - t0
        return (0.25 * np.exp(-0.5 * (t / sigma) ** 2) * np.cos(2 * np.pi * f * t)).astype(np.float32)
    y441 = na.render_offline(m, burst(44100, 29400), external_rate=44100)
    y48 = na.render_offline(m, burst(48000, 32000))
    p441, p48 = _envelope_peak(y441, 44100), _envelope_peak(y48, 48000)
    L = na.resample_plan(44100, 48000, 1)["latency_samples"]
    print("envelope peak: %.2f at 44.1 kHz, %.2f at 48 kHz = %.2f at 44.1 kHz (input peak at %d; L = %d)" % (p441, p48, p48 * 44.1 / 48.0, 14700, L))
    assert abs(p441 - p48 * 44.1 / 48.0) <= 1.0


# ---------------------------------------------------------------------------------------------------- 7

def test_three_jobs_of_two_model_rates_in_one_call_match_each_alone(na):
    """A1 Standard (48 kHz) and an LSTM resample, a 44.1 kHz model is an identity job of the same call."""
    std, m441, lstm = _model(na, "BossWN-standard.nam"), _a1_at(na, 44100), _model(na, "BossLSTM-1x16.nam")
    xs = [O.signal_noise(50000, seed=1), O.signal_noise(30011, seed=2), O.signal_noise(20000, seed=3)]
    together = na.render_offline([(std, xs[0]), (m441, xs[1]), (lstm, xs[2])], segment_samples=1024, external_rate=FE)
    alone = [na.render_offline(std, xs[0], segment_samples=1024, external_rate=FE), na.render_offline(m441, xs[1], segment_samples=1024, external_rate=FE),
             na.render_offline(lstm, xs[2], external_rate=FE)]
    for j in range(3):
        assert together[j].shape == xs[j].shape
        assert np.array_equal(together[j], alone[j]), j
    assert np.array_equal(alone[1], na.render_offline(m441, xs[1], segment_samples=1024))
    ys, _ = _streaming(na, lstm, xs[2], FE)
    assert np.array_equal(alone[2], ys)  # (a recurrent job is the sequential stream on either path)
    # the other order: job 0 is the identity job
    swapped = na.render_offline([(m441, xs[1]), (std, xs[0])], segment_samples=1024, external_rate=FE)
    assert np.array_equal(swapped[0], alone[1]) and np.array_equal(swapped[1], alone[0])


def test_several_passes_match_one_pass(na):
    m = _model(na, "BossWN-standard.nam")
    x = O.signal_noise(60000, seed=9)
    one = na.render_offline(m, x, segment_samples=1024, external_rate=FE)
    p1 = na.render_plan(m, x.size, segment_samples=1024, external_rate=FE)
    cap = 8 * p1["row_samples"]
    p3 = na.render_plan(m, x.size, segment_samples=1024, max_samples_per_pass=cap, external_rate=FE)
    assert p1["passes"] == 1 and p3["passes"] >= 3, (p1, p3)
    many = na.render_offline(m, x, segment_samples=1024, max_samples_per_pass=cap, external_rate=FE)
    assert np.array_equal(one, many)


def test_the_models_own_state_is_untouched(na):
    for name in ("BossWN-standard.nam", "BossLSTM-1x16.nam"):
        m, twin = _model(na, name, prewarm=True), _model(na, name, prewarm=True)
        x = O.signal_noise(4096, seed=11)
        a, b = m.Process(x[:2048]), twin.Process(x[:2048])
        assert np.array_equal(a, b)
        na.render_offline(m, O.signal_noise(30000, seed=12), segment_samples=1024, external_rate=FE)
        assert np.array_equal(m.Process(x[2048:]), twin.Process(x[2048:])), name


def test_the_loader_opt_in_of_the_model_is_ignored(na):
    """A model created with NA_SetResampleToExternalRate at 44.1 kHz resamples in its own Process; the render builds its batch from the
    loaded model and gives what the plain model gives."""
    plain = _model(na, "BossWN-standard.nam")
    opted = _model(na, "BossWN-standard.nam", rate=FE, opt_in=True)
    assert opted.GetProcessLatencySamples() > 0 and opted.GetModelProcessRate() == FM
    x = O.signal_noise(20000, seed=14)
    assert np.array_equal(na.render_offline(opted, x, segment_samples=512, external_rate=FE), na.render_offline(plain, x, segment_samples=512, external_rate=FE))


# ---------------------------------------------------------------------------------------------------- 8

@pytest.mark.watchdog(300)
def test_sixty_seconds_at_44100_hz_render_much_faster_than_the_streaming_path(na):
    """A relative speed check with a wide margin, same process: 60 s of A1 Standard at 44.1 kHz at least 5x faster than the one-stream
    streaming path -- the loader opt-in model at 44.1 kHz, Process in pieces of one second."""
    m = _model(na, "BossWN-standard.nam")
    x = O.signal_sine(FE * 60)
    na.render_offline(m, x[:FE], external_rate=FE)  # (first call: code objects, allocations)
    t0 = time.perf_counter()
    y = na.render_offline(m, x, external_rate=FE)
    t_render = time.perf_counter() - t0
    seq = _model(na, "BossWN-standard.nam", rate=FE, opt_in=True, prewarm=True)
    L = seq.GetProcessLatencySamples()
    seq.Process(x[:147 * 64])  # (whole phase periods: the batch of one is back at phase 0)
    seq.Prewarm()
    t0 = time.perf_counter()
    ys = np.concatenate([seq.Process(x[i:i + FE]) for i in range(0, x.size, FE)])
    t_seq = time.perf_counter() - t0
    print("60 s A1 Standard at 44.1 kHz: render %.1f ms, streaming %.1f ms, speed-up %.0fx" % (1e3 * t_render, 1e3 * t_seq, t_seq / t_render))
    assert t_seq >= 5.0 * t_render, (t_render, t_seq)
    # the streaming path is L samples late and runs the default quantum, which moves no tap: the same sums around a model that each
    # path may run on another kernel, each within the suite's WaveNet tolerance of the exact result
    err = O.rms(y[:x.size - L] - ys[L:])
    print("render against streaming: rms %.3g" % err)
    assert err < 2 * TOL_RMS
