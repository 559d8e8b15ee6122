"""GPU tests of the drive stage (NA_BatchEnableDriveStage / NA_BatchSetStreamDrive, csrc/drive_stage.h): the launch that
fills the model-input block -- oversampling FIR, shaper, decimating FIR, dry mix -- against the float64 restatement of the contract
(tests/drive_cases.py), read directly through a unit-gain pass-through model, and through an LSTM and a packed nano WaveNet.

Measured on an MI355X, worst 32-frame window as a fraction of the 2e-6 bound: 0.065 .. 0.17 (ten parity cases, growing with L), 0.092 (the ramp)."""
import os
import re

import numpy as np
import pytest

import drive_cases as D
import na_oracle as O

pytestmark = pytest.mark.gpu
NANO, LSTM = "BossWN-nano.nam", "BossLSTM-2x8.nam"


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


@pytest.fixture(scope="module")
def models(na):
    loader = na.NeuralModelLoader()
    m = {name: loader.CreateFromFile(os.path.join(O.MODELS_DIR, name), doPrewarm=False) for name in (NANO, LSTM)}
    m["pass"] = loader.CreateFromString(D.passthrough_json(), ".json", doPrewarm=False)
    assert all(v is not None for v in m.values())
    m["loader"] = loader
    return m


def make(na, models, names, drives=None, R=0):
    """a batch of one stream per name; drives: {row: params} set before the first call (None: the stage is never enabled)"""
    b = na.Batch(0)
    for name in names:
        b.AddStreams(models[name], 1, 1.0, False)
    if drives is not None:
        b.EnableDriveStage()
        for s, p in drives.items():
            b.SetStreamDrive(s, p, R)
        assert b.GetDriveInfo()["numDrives"] == len(drives)
    return b


def run(b, x, calls, close=True):
    pos, out = 0, []
    for n in calls:
        out.append(b.Process(x[:, pos:pos + n]))
        pos += n
    if close:
        b.close()
    return np.concatenate(out, axis=1)


def rows_of(count, n=D.N):
    return np.stack([D.signal(n, 5 + r) for r in range(count)])


@pytest.mark.parametrize("case", D.CASES)
def test_parity(na, models, case):
    """Row 0 (pass-through) is the stage's row itself: within the bound of the float64 restatement.  Row 1, an LSTM, and rows 2 .. 5, four
    nano WaveNets packed into one kernel-level stream, read the same block: they agree with a batch without the stage that is fed the restatement rounded to f32 -- to 1e-4,
    the bound on the row times a model gain of 50 at the most (both models' outputs are below 1)."""
    p, names = D.params(case), ("pass", LSTM) + (NANO,) * 4
    x = rows_of(len(names))
    ref = np.stack([D.restate(row, p) for row in x])
    assert np.sqrt(np.mean(ref[0] ** 2)) > 1e-3
    y = run(make(na, models, names, {s: p for s in range(len(names))}), x, [128, 128, 128, 24])
    yt = run(make(na, models, names), ref.astype(np.float32), [128, 128, 128, 24])
    frac = D.worst_window(y[0], ref[0], p["level"])
    print(case, "worst window / bound =", frac, "models:", np.abs(y[1:] - yt[1:]).max())
    assert frac < 1.0
    assert np.abs(y[1:] - yt[1:]).max() < 1e-4


def test_chunking(na, models):
    """The bits do not depend on the cut: L = 2, 4, 8 side by side; and a call longer than 4096 samples at L = 8."""
    drives = {i: D.params((D.TANH, L, 8.0, 0.1, 0.8, 1.0)) for i, L in enumerate((2, 4, 8))}
    x = rows_of(3, 512)
    whole = run(make(na, models, ["pass"] * 3, drives), x, [408])
    assert np.array_equal(run(make(na, models, ["pass"] * 3, drives), x, [128] * 4)[:, :408], whole)
    assert np.array_equal(run(make(na, models, ["pass"] * 3, drives), x, [1] + [37] * 11), whole)
    x = rows_of(1, 4096 + 37)
    long = run(make(na, models, ["pass"], {0: drives[2]}), x, [4096 + 37])
    assert np.array_equal(run(make(na, models, ["pass"], {0: drives[2]}), x, [2000, 2096, 37]), long)
    assert D.worst_window(long[0], D.restate(x[0], drives[2])) < 1.0


@pytest.mark.parametrize("L", [2, 4, 8])
def test_latency_and_dry_path(na, models, L):
    """mix 0, level 1: the input delayed by exactly 32 samples, bit for bit; drive 0: the wet part is exactly 0."""
    x = rows_of(2)
    dry, dead = D.params((D.TANH, L, 8.0, 0.2, 0.0, 1.0)), D.params((D.CUBIC, L, 0.0, 0.2, 1.0, 2.0))
    y = run(make(na, models, ["pass"] * 2, {0: dry, 1: dead}), x, [128, 37, 243])
    assert np.array_equal(y[0, D.T:], x[0, :-D.T]) and not np.any(y[0, :D.T])
    assert not np.any(y[1])


def test_ramp(na, models):
    """rampSamples = 300 on a new entry: the cut does not matter, the restatement's ramp is met, the count runs down, a set call meanwhile is refused."""
    p, x, calls = D.params((D.TANH, 4, 8.0, 0.3, 0.7, 1.5)), rows_of(1), [128, 37, 128, 115]
    whole = run(make(na, models, ["pass"], {0: p}, R=300), x, [408])
    b = make(na, models, ["pass"], {0: p}, R=300)
    assert b.StreamDriveRampRemaining(0) == 300
    first = run(b, x, calls[:1], close=False)
    assert b.StreamDriveRampRemaining(0) == 172
    with pytest.raises(na.NeuralAudioError, match="ramp running"):
        b.SetStreamDrive(0, p, 0)
    rest = run(b, x[:, 128:], calls[1:], close=False)
    assert b.StreamDriveRampRemaining(0) == 0
    b.SetStreamDrive(0, p, 0)
    b.close()
    assert np.array_equal(np.concatenate([first, rest], axis=1), whole)
    frac = D.worst_window(whole[0], D.restate(x[0], p, R=300), p["level"])
    print("ramp: worst window / bound =", frac)
    assert frac < 1.0


def test_neighbours(na, models):
    """Streams 1 and 3 of five driven: rows 0, 2, 4 are those of a batch that never enabled the stage; gate, tuner and meter IN tap of a
    driven stream read the caller's row; in place on device rows (dIn == dOut) the call gives what it gives on host rows."""
    import torch
    x, p = rows_of(5), D.params((D.HARD, 2, 8.0, 0.0, 1.0, 1.0))
    read = []
    for drives in ({1: p, 3: p}, None):
        b = make(na, models, [NANO] * 5, drives)
        b.EnableGateStage(), b.EnableTunerStage(), b.EnableMeterStage()
        b.SetStreamGate(1, na.gate_params_from_db(48000, -20.0, -30.0, -40.0), False)
        b.SetStreamTuner(1, na.tuner_params_from_range(48000, 200.0, 1000.0, 200.0))
        b.SetStreamMeter(1, {"windowSamples": 128, "clipLevelIn": 0.9, "clipLevelOut": 0.9})
        y = run(b, x, [128, 128, 128, 24], close=False)
        b.Synchronize()
        read.append((y, b.StreamGateGain(1), b.ReadStreamTuner(1), b.ReadStreamMeter(1)["in"]))
        b.close()
    assert np.array_equal(read[0][0][[0, 2, 4]], read[1][0][[0, 2, 4]]) and not np.array_equal(read[0][0][1], read[1][0][1])
    assert read[0][1:] == read[1][1:] and read[0][2] is not None
    b = make(na, models, [NANO] * 5, {1: p, 3: p})
    d = torch.from_numpy(x).to("cuda:0")
    torch.cuda.synchronize()
    b.ProcessDevice(d.data_ptr(), d.data_ptr(), D.N)
    b.Synchronize()
    b.close()
    assert np.array_equal(d.cpu().numpy(), run(make(na, models, [NANO] * 5, {1: p, 3: p}), x, [D.N]))


def test_lifecycle_and_refusals(na, models):
    p = D.params(D.CASES[0])
    b = na.Batch(0)
    with pytest.raises(na.NeuralAudioError, match=re.escape("drive stage not enabled (NA_BatchEnableDriveStage)")):
        b.SetStreamDrive(0, p)
    first = b.ReserveStreams(models["pass"], 3, False)
    b.EnableDriveStage(), b.EnableOutputStage()
    with pytest.raises(na.NeuralAudioError, match="is parked"):
        b.SetStreamDrive(first, p)
    b.ActivateStream(0), b.ActivateStream(1)
    b.SetStreamDrive(0, p), b.SetStreamDrive(1, p)
    assert b.GetStreamDrive(0) == p and b.GetStreamDrive(2) is None
    for field, bad in (("shape", 3), ("oversample", 3), ("drive", 1001.0), ("drive", float("nan")), ("bias", -4.5), ("mix", 1.5), ("level", 17.0)):
        with pytest.raises(na.NeuralAudioError, match=field):
            b.SetStreamDrive(1, dict(p, **{field: bad}))
    with pytest.raises(na.NeuralAudioError, match="rampSamples"):
        b.SetStreamDrive(1, p, (1 << 20) + 1)
    for field, other in (("shape", D.HARD), ("oversample", 8)):  # they belong to the entry for its life
        with pytest.raises(na.NeuralAudioError, match=field):
            b.SetStreamDrive(1, dict(p, **{field: other}))
    b.AddStreams(models["pass"], 20, 1.0, False)  # growth past the 16 rows the stage was sized for: the entries stay
    x = rows_of(b.NumStreams(), 128)
    y = b.Process(x)
    assert b.GetDriveInfo()["numDrives"] == 2 and D.worst_window(y[0], D.restate(x[0], p)) < 1.0 and np.array_equal(y[5], x[5])
    b.Handover(0, 2, 1.0, 64)  # the park that ends the hand-over drops the drive of stream 0
    b.Process(x), b.Process(x)
    assert b.GetDriveInfo()["numDrives"] == 1 and b.GetStreamDrive(1) == p
    b.ParkStream(1)
    b.SetStreamDrive(3, p), b.SetStreamDrive(4, p)
    b.SetStreamDrive(4, None)
    b.RemoveStreams(3)
    assert b.GetDriveInfo()["numDrives"] == 0
    assert np.array_equal(b.Process(x)[5], x[5])
    b.close()
    b = na.Batch(0)
    b.SetResampling(44100)
    with pytest.raises(na.NeuralAudioError, match="EnableDriveStage.*resampling"):
        b.EnableDriveStage()
    b.close()
    b = na.Batch(0)
    b.EnableDriveStage()
    with pytest.raises(na.NeuralAudioError, match="SetResampling.*drive stage"):
        b.SetResampling(44100)
    b.close()
