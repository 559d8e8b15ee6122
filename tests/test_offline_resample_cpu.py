"""CPU-side tests of offline rendering at an external rate (NA_RenderPlanAtRate / NA_RenderOfflineAtRate, csrc/offline_render.cpp):
the plan and every refusal need no device.

  * the plan at a rate is the plan of NA_RenderPlan for jobs of M = J(N + L) model-rate frames, J from NA_ResampleModelFrames
    (quantum 1) and L from NA_ResamplePlan -- up to two hours of samples, where the ticks need 64 bits
  * a refused pair, a rate <= 0, a job without a model and overlapping buffers fail the call, with the reason, before any device work
  * without external_rate the Python calls are today's
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import na_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWO_HOURS = 2 * 3600


@pytest.fixture(scope="module")
def na():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "neuralaudio_amd", "libNeuralAudioCAPI.so")):
        g.build()
    import neuralaudio_amd
    return neuralaudio_amd


def _load(na, name, rate=None):
    loader = na.NeuralModelLoader()
    if rate:
        loader.SetExternalSampleRate(rate)
    m = loader.CreateFromFile(os.path.join(O.MODELS_DIR, name), doPrewarm=False)
    assert m is not None
    return m


def _a1_at(na, rate):
    """a synthetic A1 Nano whose file says `rate`"""
    arrays = O.a1_arrays(4, 2)
    doc = json.loads(O.nam_json_wavenet_a1(4, 2, O.synth_wavenet_weights(arrays, seed=7)))
    doc["sample_rate"] = rate
    loader = na.NeuralModelLoader()
    m = loader.CreateFromString(json.dumps(doc), ".nam", doPrewarm=False)
    assert m is not None and m.GetModelProcessRate() == rate
    m._loader = loader  # (keeps the loader alive as long as the model)
    return m


def _plan(na, m, n, external_rate=None, segment_samples=0, max_samples_per_pass=0):
    """NA_RenderPlan / NA_RenderPlanAtRate of one job of n samples through the C ABI (a plan reads no buffer: none is made, so n may be
    hours of samples); returns (plan numbers, resample info or None)"""
    from neuralaudio_amd import capi
    jobs = (capi.NA_RenderJob * 1)()
    jobs[0].model, jobs[0].quality, jobs[0].numSamples = m._h, 1.0, n
    o = capi.NA_RenderOptions(segment_samples, max_samples_per_pass, 0.0)
    info, rs = capi.NA_RenderPlanInfo(), capi.NA_ResampleInfo()
    lib = capi.load_library()
    rc = (lib.NA_RenderPlan(jobs, 1, C.byref(o), C.byref(info)) if external_rate is None
          else lib.NA_RenderPlanAtRate(jobs, 1, C.byref(o), external_rate, C.byref(info), C.byref(rs)))
    assert rc == 0, capi.last_error()
    numbers = (info.segments, info.lead, info.segmentSamples, info.rowSamples, info.passes, info.streams, info.estimatedMs, info.kernel)
    return numbers, (None if external_rate is None else na._resample_info(rs))


# (external rate, model): 44.1 -> 48 kHz; 48 -> 44.1 kHz for a 44.1 kHz model; 32 -> 48 kHz; 96 -> 48 kHz with the model loaded at the
# default rate; the identity
PAIRS = ["44100->48000", "48000->44100", "32000->48000", "96000->48000", "48000->48000"]


def _pair(na, pair):
    fe, fm = (int(v) for v in pair.split("->"))
    return fe, fm, (_a1_at(na, 44100) if fm == 44100 else _load(na, "BossWN-standard.nam"))


@pytest.mark.parametrize("pair", PAIRS)
def test_the_plan_at_a_rate_is_the_plan_of_the_model_rate_frames(na, pair):
    fe, fm, m = _pair(na, pair)
    assert m.GetModelProcessRate() == fm
    rp = na.resample_plan(fe, fm, 1)
    L = rp["latency_samples"]
    assert (L == 0) == (fe == fm)
    lengths = [0, 1, fe * 10, fe * TWO_HOURS] + ([L - 1] if L > 1 else [])
    for N in lengths:
        M = na.resample_model_frames(fe, fm, 1, N + L)
        for opts in ({}, {"segment_samples": 512}, {"segment_samples": 4096, "max_samples_per_pass": 1 << 20}):
            at, info = _plan(na, m, N, external_rate=fe, **opts)
            assert info == rp
            assert at == _plan(na, m, M, **opts)[0], (pair, N, M, opts)
            if N <= fe * 10:  # (the Python call makes the signal)
                py = na.render_plan(m, N, external_rate=fe, **opts)
                assert py.pop("resample") == rp and py == na.render_plan(m, M, **opts)
    # two hours: the tick of the last model frame does not fit 32 bits, and the frame count is the exact rational one
    N = fe * TWO_HOURS
    M = na.resample_model_frames(fe, fm, 1, N + L)
    assert M == ((N + L - 1) * rp["te"]) // rp["tm"] + 1 if fe != fm else M == N
    if 44100 in (fe, fm):
        assert (M - 1) * rp["tm"] > 2 ** 32
    (segments, lead, kept, _, _, _, _, _), _ = _plan(na, m, N, external_rate=fe, segment_samples=1 << 16)
    assert lead + segments * kept >= M > lead + (segments - 1) * kept


def test_jobs_of_one_call_may_have_different_model_rates(na):
    std, m441, lstm = _load(na, "BossWN-standard.nam"), _a1_at(na, 44100), _load(na, "BossLSTM-1x16.nam")
    fe = 44100
    L = na.resample_plan(fe, 48000, 1)["latency_samples"]
    assert lstm.GetModelProcessRate() == 48000
    M = na.resample_model_frames(fe, 48000, 1, 50000 + L)
    at = na.render_plan([(std, 50000), (m441, 30000), (lstm, 20000)], segment_samples=1024, external_rate=fe)
    # job 0's pair; the 44.1 kHz model is an identity job of its own 30000 samples; the LSTM runs J(20000 + L) frames
    assert at.pop("resample") == na.resample_plan(fe, 48000, 1)
    assert at == na.render_plan([(std, M), (m441, 30000), (lstm, na.resample_model_frames(fe, 48000, 1, 20000 + L))], segment_samples=1024)


def test_refusals_come_with_their_reason_and_before_any_device_work(na):
    from neuralaudio_amd import capi
    lib = capi.load_library()
    m = _load(na, "BossWN-nano.nam")
    x, y = np.zeros(4096, np.float32), np.full(4096, 123.0, np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    jobs = (capi.NA_RenderJob * 1)()
    jobs[0].model, jobs[0].quality, jobs[0].numSamples, jobs[0].input, jobs[0].output = m._h, 1.0, x.size, fp(x), fp(y)
    info, rs = capi.NA_RenderPlanInfo(), capi.NA_ResampleInfo()
    # 44101 : 48000 does not reduce below 640
    assert lib.NA_RenderPlanAtRate(jobs, 1, None, 44101, C.byref(info), C.byref(rs)) != 0
    assert "640" in capi.last_error()
    assert lib.NA_RenderOfflineAtRate(jobs, 1, None, 44101) != 0
    assert "640" in capi.last_error()
    with pytest.raises(na.NeuralAudioError, match="640"):
        na.render_offline(m, x, external_rate=44101)
    with pytest.raises(na.NeuralAudioError, match="640"):
        na.render_plan(m, x.size, external_rate=44101)
    # a refused pair anywhere among the jobs refuses the whole call: 128000 : 48000 is 8 : 3, 128000 : 44100 is 1280 : 441
    assert na.render_plan(m, x.size, external_rate=128000)["resample"]["te"] == 3
    with pytest.raises(na.NeuralAudioError, match="640"):
        na.render_offline([(m, x), (_a1_at(na, 44100), x)], external_rate=128000)
    for rate in (0, -44100):
        assert lib.NA_RenderPlanAtRate(jobs, 1, None, rate, C.byref(info), None) != 0
        assert "positive" in capi.last_error()
        assert lib.NA_RenderOfflineAtRate(jobs, 1, None, rate) != 0
        assert "positive" in capi.last_error()
    # overlapping buffers
    jobs[0].output = fp(x[1:])
    jobs[0].numSamples = 1000
    assert lib.NA_RenderOfflineAtRate(jobs, 1, None, 44100) != 0
    assert "overlap" in capi.last_error()
    # a job without a model
    jobs[0].model = None
    assert lib.NA_RenderOfflineAtRate(jobs, 1, None, 44100) != 0
    assert "NULL model" in capi.last_error()
    assert lib.NA_RenderPlanAtRate(jobs, 1, None, 44100, C.byref(info), None) != 0
    assert "NULL model" in capi.last_error()
    assert lib.NA_RenderPlanAtRate(None, 1, None, 44100, C.byref(info), None) != 0
    assert lib.NA_RenderPlanAtRate(jobs, 1, None, 44100, None, None) != 0
    assert np.all(y == 123.0)  # (no call wrote a sample)


def test_the_tap_refuses_a_call_it_cannot_hold(na):
    """NA_DebugSetRenderTap: M > capacity fails the next call before any device work, and the tap is then off again."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    m = _load(na, "BossWN-nano.nam")
    x = np.zeros(4096, np.float32)
    u = np.zeros(16, np.float32)
    lib.NA_DebugSetRenderTap(u.ctypes.data_as(C.POINTER(C.c_float)), None, 16)
    with pytest.raises(na.NeuralAudioError, match="tap"):
        na.render_offline(m, x, external_rate=44100)
    if na.device_count() < 1:
        with pytest.raises(na.NeuralAudioError, match="no HIP device"):  # (not the tap's refusal any more)
            na.render_offline(m, x, external_rate=44100)


def test_without_an_external_rate_the_python_calls_are_unchanged(na):
    from neuralaudio_amd import capi
    m = _load(na, "BossWN-standard.nam")
    for n, opts in ((48000 * 60, {}), (48000, {"segment_samples": 512}), (1000, {})):
        p = na.render_plan(m, n, **opts)
        assert p == na.render_plan(m, n, external_rate=None, **opts)
        assert sorted(p) == ["estimated_ms", "kernel", "lead", "passes", "row_samples", "segment_samples", "segments", "streams"]
        # ... and they are NA_RenderPlan's own numbers
        jobs = (capi.NA_RenderJob * 1)()
        jobs[0].model, jobs[0].quality, jobs[0].numSamples = m._h, 1.0, n
        o = capi.NA_RenderOptions(int(opts.get("segment_samples", 0)), 0, 0.0)
        info = capi.NA_RenderPlanInfo()
        assert capi.load_library().NA_RenderPlan(jobs, 1, C.byref(o), C.byref(info)) == 0
        assert (p["segments"], p["lead"], p["segment_samples"], p["row_samples"], p["passes"], p["streams"]) == \
            (info.segments, info.lead, info.segmentSamples, info.rowSamples, info.passes, info.streams)
    if na.device_count() < 1:
        with pytest.raises(na.NeuralAudioError, match="no HIP device"):
            na.render_offline(m, np.ones(64, np.float32), external_rate=44100)
