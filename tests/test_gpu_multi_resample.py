"""The multi-GPU host at an external sample rate (NA_MultiSetResampling, csrc/multi_gpu.cpp): every shard's batch is a resampling batch
of one plan, every n counts external samples, all shards share one phase.  On a one-GPU box the shards share the device
(devices = [0, 0, ...]); the reference is ONE resampling batch holding the same global list, bit for bit -- whatever the call lengths,
through the blocking and the pipelined interface and under both fan-in modes (RCCL through the in-library loopback table)."""
import os

import numpy as np
import pytest

import na_oracle as O

pytestmark = pytest.mark.gpu

FE, FM = 44100, 48000


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


def _path(name):
    return os.path.join(O.MODELS_DIR, name)


def _entries(loader):
    std = loader.CreateFromFile(_path("BossWN-standard.nam"), doPrewarm=False)
    nano = loader.CreateFromFile(_path("BossWN-nano.nam"), doPrewarm=False)
    lstm = loader.CreateFromFile(_path("BossLSTM-1x16.nam"), doPrewarm=False)
    return [(std, 5), (nano, 9), (lstm, 7)]  # architecture-sorted global list


def _single(na, entries):
    one = na.Batch(0)
    one.SetResampling(FE, FM, max_frames=512)
    for m, c in entries:
        one.AddStreams(m, c)
    return one


def _multi(na, entries, shards, fan_in="host"):
    multi = na.MultiBatch([0] * shards)
    multi.SetResampling(FE, FM, max_frames=512)
    if fan_in != "host":
        multi.SetFanIn(fan_in)
    first = 0
    for m, c in entries:
        assert multi.AddStreams(m, c) == first
        first += c
    multi.Commit()
    return multi


@pytest.mark.parametrize("shards", [2, 3])
def test_sharded_resampling_host_matches_one_resampling_batch(na, shards):
    """Calls of 128 samples, of every length from 1 to 300 and one call of 3000 (beyond the 2048-sample piece of the stages): the blocking
    and the pipelined multi batch both return the single batch's rows bit for bit."""
    loader = na.NeuralModelLoader()
    entries = _entries(loader)
    one, blocking, pipelined = _single(na, entries), _multi(na, entries, shards), _multi(na, entries, shards)
    assert blocking.ResampleInfo() == pipelined.ResampleInfo() == one.ResampleInfo() == na.resample_plan(FE, FM)
    ranges = blocking.ShardRanges()
    S = one.NumStreams()
    assert len(ranges) == shards and ranges[0][0] == 0 and ranges[-1][1] == S and all(ranges[i][1] > ranges[i][0] for i in range(shards))
    rng = np.random.default_rng(2)
    for n in [128] * 6 + list(range(1, 301)) + [3000, 128]:
        x = (0.3 * rng.standard_normal((S, n))).clip(-1, 1).astype(np.float32)
        ref = one.Process(x)
        assert ref.shape == (S, n)
        assert np.array_equal(blocking.Process(x), ref), n
        assert np.array_equal(pipelined.Collect(pipelined.Submit(x)), ref), n
    assert np.all(np.isfinite(ref)) and O.rms(ref[0]) > 1e-3 and O.rms(ref[S - 1]) > 1e-4  # (the streams ran: not silence)
    # several buffers in flight
    xs = [(0.3 * rng.standard_normal((S, 128))).clip(-1, 1).astype(np.float32) for _ in range(2)]
    tickets = [pipelined.Submit(x) for x in xs]
    for x, t in zip(xs, tickets):
        assert np.array_equal(pipelined.Collect(t), one.Process(x))
    for b in (one, blocking, pipelined):
        b.close()


def test_refusals(na):
    loader = na.NeuralModelLoader()
    std = loader.CreateFromFile(_path("BossWN-standard.nam"), doPrewarm=False)
    over = na.NeuralModelLoader()
    over.SetExternalSampleRate(96000)
    std96 = over.CreateFromFile(_path("BossWN-standard.nam"), doPrewarm=False)
    assert std96.GetModelProcessRate() == 96000
    multi = na.MultiBatch([0, 0])
    with pytest.raises(na.NeuralAudioError, match="NA_MultiSetResampling was not called"):
        multi.ResampleInfo()
    with pytest.raises(na.NeuralAudioError, match="quantum"):
        multi.SetResampling(FE, FM, quantum=3)
    with pytest.raises(na.NeuralAudioError, match="640"):
        multi.SetResampling(44101, FM)
    with pytest.raises(na.NeuralAudioError, match="positive"):
        multi.SetResampling(0, FM)
    with pytest.raises(na.NeuralAudioError, match="maxFrames"):
        multi.SetResampling(FE, FM, max_frames=0)
    with pytest.raises(na.NeuralAudioError):  # (none of them left a plan behind)
        multi.ResampleInfo()
    multi.SetResampling(FE, FM, quantum=64)
    assert multi.ResampleInfo() == na.resample_plan(FE, FM, 64)
    # a model of the wrong process rate: the message NA_BatchAddStreams gives
    one = na.Batch(0)
    one.SetResampling(FE, FM, quantum=64)
    with pytest.raises(na.NeuralAudioError, match="resamples to a model rate of 48000") as single:
        one.AddStreams(std96, 2)
    with pytest.raises(na.NeuralAudioError, match="resamples to a model rate of 48000") as sharded:
        multi.AddStreams(std96, 2)
    assert str(single.value) == str(sharded.value)
    assert multi.NumStreams() == 0
    multi.AddStreams(std, 6)
    multi.Commit()
    with pytest.raises(na.NeuralAudioError, match="after Commit"):
        multi.SetResampling(FE, FM)
    assert multi.ResampleInfo() == na.resample_plan(FE, FM, 64)
    # ... and a wrong-rate model that is already on the list refuses the set-up call itself
    late = na.MultiBatch([0])
    late.AddStreams(std96, 1)
    with pytest.raises(na.NeuralAudioError, match="resamples to a model rate of 48000"):
        late.SetResampling(FE, FM)
    for b in (one, multi, late):
        b.close()


@pytest.fixture
def loopback(na):
    """The multi-GPU host bound to the in-library loopback table instead of librccl.so: ranks may share the one GPU of this box."""
    na.debug_set_rccl_api(1)
    yield na
    na.debug_set_rccl_api(0)


@pytest.mark.parametrize("shards", [2, 3])
def test_rccl_fan_in_gathers_rows_of_external_samples(loopback, shards):
    """RCCL fan-in works with resampling: the gathered buffer is [streams][n] in external samples on every rank, bit-identical to one
    resampling batch (weights fanned out, rows gathered, one download from shard 0 -- through the loopback table on one GPU)."""
    na = loopback
    loader = na.NeuralModelLoader()
    entries = _entries(loader)
    one, multi = _single(na, entries), _multi(na, entries, shards, fan_in="rccl")
    assert multi.ResampleInfo() == one.ResampleInfo()
    S = one.NumStreams()
    rng = np.random.default_rng(11)
    for n in (128, 64, 1, 300, 128, 2500):
        x = (0.3 * rng.standard_normal((S, n))).clip(-1, 1).astype(np.float32)
        ym, yo = multi.Process(x), one.Process(x)
        assert np.array_equal(ym, yo), n
        for s in range(shards):  # every rank holds the whole gathered array
            assert np.array_equal(multi.GatheredOutput(s, n), yo), (n, s)
    assert O.rms(yo[0]) > 1e-3 and O.rms(yo[S - 1]) > 1e-4
    multi.close()
    one.close()
