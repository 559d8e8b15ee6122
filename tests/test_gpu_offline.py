"""GPU tests of the offline renderer (NA_RenderOffline, csrc/offline_render.cpp): time-parallel segments of one long signal.

The reference of every comparison is the sequential path on a FRESH prewarmed instance of the model (Process over the whole signal,
in chunks -- the kernels are chunk-invariant bit for bit, test_gpu_batch.py).  Where the segment batch runs the model on the same
kernel as a one-stream batch, the render must be bit-identical to it; in every case it must be within the suite's WaveNet tolerance
of the live oracle."""
import os
import time

import numpy as np
import pytest

import na_oracle as O
import wide_cases as WC

pytestmark = pytest.mark.gpu

TOL_RMS = 2e-6
CHUNK = 8192


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


def _model(na, name, quality=1.0, rate=None, prewarm=True):
    loader = na.NeuralModelLoader()
    loader.SetDefaultQualityScaleFactor(quality)
    if rate:
        loader.SetExternalSampleRate(rate)
    m = loader.CreateFromFile(os.path.join(O.MODELS_DIR, name), doPrewarm=prewarm)
    assert m is not None
    m._loader = loader  # (keeps the loader alive as long as the model)
    return m


def _sequential(na, name, x, quality=1.0, rate=None):
    """a fresh instance, prewarmed, Process over the whole signal"""
    m = _model(na, name, quality, rate)
    y = np.concatenate([m.Process(x[i:i + CHUNK]) for i in range(0, x.size, CHUNK)]) if x.size else np.zeros(0, np.float32)
    m.close()
    return y


def _kernel(na, name, quality, streams, rate=None):
    """NA_BatchStreamKernelName of the first stream of a batch of `streams` streams of the model"""
    m = _model(na, name, quality, rate, prewarm=False)
    b = na.Batch(0)
    b.AddStreams(m, streams, quality=quality, doPrewarm=False)
    k = b.StreamKernelName(0)
    b.close()
    return k


WIDE = {"wide-40/20": (40, 20), "wide-72/36": (72, 36)}  # synthetic models of the runtime-shaped kernels (> 16 channels)
CASES = [("BossWN-standard.nam", 1.0), ("BossWN-lite.nam", 1.0), ("wide-40/20", 1.0), ("wide-72/36", 1.0), ("BossWN-feather.nam", 1.0), ("BossWN-nano.nam", 1.0),
         ("BossWN-a2.nam", 0.0), ("BossWN-a2.nam", 1.0), ("BossLSTM-1x16.nam", 1.0), ("BossLSTM-2x8.nam", 1.0),
         ("synthetic_gru_1x16.json", 1.0)]


@pytest.mark.parametrize("name,quality", CASES)
def test_every_sample_model_matches_the_sequential_run(na, name, quality):
    """~90 segment boundaries (segmentSamples = 512 over 48 000 samples of clipped noise): bit-identical to the sequential run where both
    batches run the stream on the same kernel; within the WaveNet tolerance of the oracle in every case."""
    if name == "BossWN-lite.nam" or name in WIDE:
        if name in WIDE:
            arrays = WC.two_array(*WIDE[name])
            w = O.synth_wavenet_weights(arrays, seed=WIDE[name][0])
            text = O.nam_json_wavenet_generic(arrays, w)
        else:
            # (no A1 Lite capture among the sample models: a synthetic A1 Lite stands in for it)
            arrays = O.a1_arrays(12, 6)
            w = O.synth_wavenet_weights(arrays, seed=41)
            text = O.nam_json_wavenet_a1(12, 6, w)
        loader = na.NeuralModelLoader()
        m = loader.CreateFromString(text, ".nam", doPrewarm=False)
        seq_m = loader.CreateFromString(text, ".nam", doPrewarm=True)
        ora = O.OracleWaveNet(arrays, w)
        x = O.signal_noise(48000, seed=5)
        y = na.render_offline(m, x, quality=quality, segment_samples=512)
        ys = np.concatenate([seq_m.Process(x[i:i + CHUNK]) for i in range(0, x.size, CHUNK)])
        plan = na.render_plan(m, x.size, quality=quality, segment_samples=512)
        b = na.Batch(0)
        b.AddStreams(m, 1, doPrewarm=False)
        same = plan["kernel"] == b.StreamKernelName(0)
        b.close()
    else:
        m = _model(na, name, quality, prewarm=False)
        x = O.signal_noise(48000, seed=5)
        y = na.render_offline(m, x, quality=quality, segment_samples=512)
        ys = _sequential(na, name, x, quality)
        plan = na.render_plan(m, x.size, quality=quality, segment_samples=512)
        same = plan["kernel"] == _kernel(na, name, quality, 1)
        ora = O.oracle_from_file(name, quality)
    assert y.shape == x.shape and np.all(np.isfinite(y))
    if plan["lead"] > 0:
        assert plan["segments"] >= 80
    print("%s q=%g: %s" % (name, quality, "bit-identical" if same else "tolerance (segment kernel %s)" % plan["kernel"]))
    if same:
        assert np.array_equal(y, ys), (name, quality, plan, int(np.argmax(y != ys)))
    yo = ora.process(x)
    assert O.rms(y - yo) < TOL_RMS, (name, quality, plan)
    assert O.rms(ys - yo) < TOL_RMS


def test_impulse_before_a_segment_boundary_is_seen(na):
    """A unit impulse 1, lead - 1 and lead samples before a boundary: a lead that is too short would lose it in the next segment."""
    m = _model(na, "BossWN-standard.nam", prewarm=False)
    L = 512
    plan = na.render_plan(m, 40000, segment_samples=L)
    lead = plan["lead"]
    boundary = lead + 20 * L  # where segment 20 starts keeping
    for back in (1, lead - 1, lead):
        x = np.zeros(40000, np.float32)
        x[boundary - back] = 1.0
        y = na.render_offline(m, x, segment_samples=L)
        ys = _sequential(na, "BossWN-standard.nam", x)
        assert np.array_equal(y, ys), (back, int(np.argmax(y != ys)))


@pytest.mark.parametrize("length_of", ["1", "127", "128", "129", "lead-1", "lead", "lead+1", "3lead+77"])
def test_lengths(na, length_of):
    m = _model(na, "BossWN-standard.nam", prewarm=False)
    lead = na.render_plan(m, 100000)["lead"]
    n = {"1": 1, "127": 127, "128": 128, "129": 129, "lead-1": lead - 1, "lead": lead, "lead+1": lead + 1, "3lead+77": 3 * lead + 77}[length_of]
    x = O.signal_noise(n, seed=n)
    ys = _sequential(na, "BossWN-standard.nam", x)
    for seg in (0, 128):
        y = na.render_offline(m, x, segment_samples=seg)
        assert y.shape == x.shape and np.array_equal(y, ys), (n, seg)


def test_several_passes_match_one_pass(na):
    m = _model(na, "BossWN-standard.nam", prewarm=False)
    x = O.signal_noise(60000, seed=9)
    one = na.render_offline(m, x, segment_samples=1024)
    p1 = na.render_plan(m, x.size, segment_samples=1024)
    cap = 8 * p1["row_samples"]
    p3 = na.render_plan(m, x.size, segment_samples=1024, max_samples_per_pass=cap)
    assert p1["passes"] == 1 and p3["passes"] >= 3, (p1, p3)
    many = na.render_offline(m, x, segment_samples=1024, max_samples_per_pass=cap)
    assert np.array_equal(one, many)
    if p3["kernel"] == _kernel(na, "BossWN-standard.nam", 1.0, 1):
        assert np.array_equal(many, _sequential(na, "BossWN-standard.nam", x))


def test_three_jobs_in_one_call_match_each_alone(na):
    """Two WaveNet models of different leads (A1 Standard, A2) plus an LSTM, different lengths and qualities, in one call."""
    std = _model(na, "BossWN-standard.nam", prewarm=False)
    a2 = _model(na, "BossWN-a2.nam", 0.0, prewarm=False)
    lstm = _model(na, "BossLSTM-1x16.nam", prewarm=False)
    xs = [O.signal_noise(50000, seed=1), O.signal_noise(30011, seed=2), O.signal_noise(20000, seed=3)]
    together = na.render_offline([(std, xs[0], 1.0), (a2, xs[1], 0.0), (lstm, xs[2], 1.0)], segment_samples=1024)
    alone = [na.render_offline(std, xs[0], segment_samples=1024), na.render_offline(a2, xs[1], quality=0.0, segment_samples=1024),
             na.render_offline(lstm, xs[2])]
    for j in range(3):
        assert together[j].shape == xs[j].shape
        assert np.array_equal(together[j], alone[j]), j
    assert np.array_equal(alone[2], _sequential(na, "BossLSTM-1x16.nam", xs[2]))
    assert O.rms(together[1] - O.oracle_from_file("BossWN-a2.nam", 0.0).process(xs[1])) < TOL_RMS


def test_the_models_own_state_is_untouched(na):
    for name in ("BossWN-standard.nam", "BossLSTM-1x16.nam"):
        m, twin = _model(na, name), _model(na, name)
        x = O.signal_noise(4096, seed=11)
        a, b = m.Process(x[:2048]), twin.Process(x[:2048])
        assert np.array_equal(a, b)
        na.render_offline(m, O.signal_noise(30000, seed=12), segment_samples=1024)
        assert np.array_equal(m.Process(x[2048:]), twin.Process(x[2048:])), name


def test_oversampled_model_matches_its_sequential_run(na):
    m = _model(na, "BossWN-standard.nam", rate=96000, prewarm=False)
    x = O.signal_noise(96000, seed=13)
    plan = na.render_plan(m, x.size, segment_samples=1024)
    assert plan["lead"] >= 2 * 4092 and plan["segments"] > 10
    y = na.render_offline(m, x, segment_samples=1024)
    ys = _sequential(na, "BossWN-standard.nam", x, rate=96000)
    if plan["kernel"] == _kernel(na, "BossWN-standard.nam", 1.0, 1, rate=96000):
        assert np.array_equal(y, ys)
    assert O.rms(y - ys) < TOL_RMS


@pytest.mark.watchdog(300)
def test_sixty_seconds_render_much_faster_than_the_sequential_path(na):
    """A relative speed check with a wide margin: 60 s of A1 Standard at least 5x faster than the sequential path, same process."""
    m = _model(na, "BossWN-standard.nam", prewarm=False)
    x = O.signal_sine(48000 * 60)
    na.render_offline(m, x[:48000])  # (first call: code objects, allocations)
    t0 = time.perf_counter()
    y = na.render_offline(m, x)
    t_render = time.perf_counter() - t0
    seq = _model(na, "BossWN-standard.nam")
    seq.Process(x[:CHUNK])
    seq.Prewarm()
    t0 = time.perf_counter()
    ys = np.concatenate([seq.Process(x[i:i + 48000]) for i in range(0, x.size, 48000)])
    t_seq = time.perf_counter() - t0
    print("60 s A1 Standard: render %.1f ms, sequential %.1f ms, speed-up %.0fx" % (1e3 * t_render, 1e3 * t_seq, t_seq / t_render))
    assert t_seq >= 5.0 * t_render, (t_render, t_seq)
    assert O.rms(y - ys) < TOL_RMS
