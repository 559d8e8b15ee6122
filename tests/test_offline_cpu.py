"""CPU-side tests of the offline renderer (NA_RenderPlan / NA_RenderOffline, csrc/offline_render.cpp): the planner needs no device.

  * the lead covers the summed history of the stream's rings, rounded up to a block, for A1 / A2 / oversampled models
  * recurrent models are never cut: one segment per job
  * segment length and pass count follow the options; bad arguments fail with a reason
  * without a device NA_RenderOffline fails loudly (no CPU fallback)
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import na_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


@pytest.mark.parametrize("name", ["BossWN-standard.nam", "BossWN-nano.nam", "BossWN-feather.nam"])
def test_a1_lead_covers_the_receptive_field_rounded_to_a_block(na, name):
    m = _load(na, name)
    p = na.render_plan(m, 48000 * 60)
    assert p["lead"] >= 4091 and p["lead"] % 128 == 0 and p["lead"] - 128 < m.GetReceptiveFieldSize()
    assert p["segments"] > 1 and p["passes"] >= 1 and p["streams"] >= 1
    assert p["row_samples"] == p["lead"] + p["segment_samples"]
    # the kept parts tile the signal: segment 0 keeps lead + L, every later one L
    assert p["lead"] + p["segments"] * p["segment_samples"] >= 48000 * 60 > p["lead"] + (p["segments"] - 1) * p["segment_samples"]


def test_a2_lead_includes_the_conv_head(na):
    a2 = _load(na, "BossWN-a2.nam")
    for q in (0.0, 1.0):
        a2.SetQualityScaleFactor(q)
        rf = a2.GetReceptiveFieldSize()
        p = na.render_plan(a2, 48000 * 10, quality=q)
        # the A2 head is a 16-tap conv: 15 more frames of history on top of the layers
        assert p["lead"] >= rf and p["lead"] % 128 == 0, (q, rf, p)
        assert p["lead"] > na.render_plan(_load(na, "BossWN-standard.nam"), 48000 * 10)["lead"]


def test_oversampled_model_has_about_twice_the_lead(na):
    base = na.render_plan(_load(na, "BossWN-standard.nam"), 96000)["lead"]
    over = na.render_plan(_load(na, "BossWN-standard.nam", rate=96000), 96000)["lead"]
    assert 2 * base - 256 <= over <= 2 * base + 128, (base, over)


@pytest.mark.parametrize("name", ["BossLSTM-1x16.nam", "BossLSTM-2x8.nam", "synthetic_gru_1x16.json"])
def test_recurrent_model_is_one_segment_per_job(na, name):
    m = _load(na, name)
    p = na.render_plan(m, 48000 * 30)
    assert p["segments"] == 1 and p["streams"] == 1 and p["lead"] == 0
    p = na.render_plan([(m, 48000 * 30), (m, 1000), (m, 77)])
    assert p["segments"] == 3 and p["streams"] == 3 and p["lead"] == 0


def test_segment_length_and_passes_follow_the_options(na):
    m = _load(na, "BossWN-standard.nam")
    p = na.render_plan(m, 48000, segment_samples=512)
    assert p["segment_samples"] == 512 and p["row_samples"] == p["lead"] + 512
    assert p["segments"] == -(-(48000 - p["lead"]) // 512) and p["passes"] == 1 and p["streams"] == p["segments"]
    # a pass holds at most maxSamplesPerPass samples of segment rows: here four rows, so the 86 segments take 22 passes
    q = na.render_plan(m, 48000, segment_samples=512, max_samples_per_pass=4 * p["row_samples"])
    assert q["streams"] * q["row_samples"] <= 4 * p["row_samples"]
    assert q["segments"] == p["segments"] and q["passes"] == -(-p["segments"] // q["streams"]) and q["passes"] >= 3
    # a signal that fits one row is one segment without a lead-in
    s = na.render_plan(m, 1000)
    assert s["segments"] == 1 and s["passes"] == 1 and s["streams"] == 1 and s["row_samples"] >= 1000


def test_several_jobs_share_one_lead_and_one_batch(na):
    std, a2, lstm = _load(na, "BossWN-standard.nam"), _load(na, "BossWN-a2.nam"), _load(na, "BossLSTM-1x16.nam")
    p = na.render_plan([(std, 48000), (a2, 30000, 0.0), (lstm, 20000)], segment_samples=1024)
    assert p["lead"] == na.render_plan(a2, 30000, quality=0.0)["lead"]
    g = [-(-(48000 - p["lead"]) // 1024), -(-(30000 - p["lead"]) // 1024)]
    assert p["segments"] == sum(g) + 1
    # the LSTM walks its 20000 samples one row length per pass; the WaveNet segments are dealt over those passes
    assert p["passes"] == -(-20000 // p["row_samples"]) > 1
    assert p["streams"] == sum(-(-x // p["passes"]) for x in g) + 1


def test_bad_arguments_fail_with_a_reason(na):
    from neuralaudio_amd import capi
    lib = capi.load_library()
    info = capi.NA_RenderPlanInfo()
    assert lib.NA_RenderPlan(None, 1, None, C.byref(info)) != 0
    assert "NULL" in capi.last_error()
    jobs = (capi.NA_RenderJob * 1)()
    jobs[0].numSamples = 16
    assert lib.NA_RenderPlan(jobs, 1, None, C.byref(info)) != 0
    assert "NULL model" in capi.last_error()
    assert lib.NA_RenderOffline(jobs, 1, None) != 0
    assert "NULL model" in capi.last_error()
    m = _load(na, "BossWN-nano.nam")
    jobs[0].model = m._h
    for n in (0, -1):
        assert lib.NA_RenderPlan(jobs, n, None, C.byref(info)) != 0
        assert "numJobs" in capi.last_error()
        assert lib.NA_RenderOffline(jobs, n, None) != 0
        assert "numJobs" in capi.last_error()
    assert lib.NA_RenderPlan(jobs, 1, None, None) != 0
    # a job with samples but no buffers
    assert lib.NA_RenderOffline(jobs, 1, None) != 0
    assert "buffer" in capi.last_error()


def test_render_without_gpu_fails_loudly(na):
    """No CPU fallback: without a HIP device NA_RenderOffline reports an error and writes no numbers."""
    if na.device_count() > 0:
        pytest.skip("a GPU is present")
    m = _load(na, "BossWN-nano.nam")
    x = np.ones(4096, np.float32)
    with pytest.raises(na.NeuralAudioError) as e:
        na.render_offline(m, x)
    assert "no HIP device" in str(e.value)
    from neuralaudio_amd import capi
    y = np.full(16, 123.0, np.float32)
    jobs = (capi.NA_RenderJob * 1)()
    jobs[0].model, jobs[0].quality, jobs[0].numSamples = m._h, 1.0, 16
    jobs[0].input = x.ctypes.data_as(C.POINTER(C.c_float))
    jobs[0].output = y.ctypes.data_as(C.POINTER(C.c_float))
    assert capi.load_library().NA_RenderOffline(jobs, 1, None) != 0
    assert "no HIP device" in capi.last_error()
    assert np.all(y == 123.0)
