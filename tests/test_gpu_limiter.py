"""GPU tests of the limiter stage (NA_BatchEnableLimiterStage / NA_BatchSetStreamLimiter, csrc/limiter_stage.h): the
launch behind the mix stage against the numpy float32 restatement of the contract (tests/limiter_cases.py), bit for bit, read through
a unit-gain pass-through model."""
import re

import numpy as np
import pytest

import drive_cases as D
import limiter_cases as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


@pytest.fixture(scope="module")
def model(na):
    loader = na.NeuralModelLoader()
    m = loader.CreateFromString(D.passthrough_json(), ".json", doPrewarm=False)
    assert m is not None
    return loader, m


def make(na, model, rows, limiters=None):
    """a batch of `rows` pass-through streams; limiters: {row: params} set before the first call (None: the stage is never enabled)"""
    b = na.Batch(0)
    b.AddStreams(model[1], rows, 1.0, False)
    if limiters is not None:
        b.EnableLimiterStage()
        for s, p in limiters.items():
            b.SetStreamLimiter(s, p)
        assert b.GetLimiterInfo()["numLimiters"] == len(limiters)
    return b


def run(b, x, calls, close=True):
    pos, out = 0, []
    for n in calls:
        out.append(b.Process(x[:, pos:pos + n]))
        pos += n
    if close:
        b.close()
    return np.concatenate(out, axis=1)


@pytest.mark.parametrize("L,H", M.CASES)
def test_parity_at_every_cut(na, model, L, H):
    """Row 0 is limited, row 1 never reaches c: every cut into calls gives the restatement's bits, |y| <= c, and the quiet row comes out
    bit for bit, L samples late."""
    p = M.params(L, H)
    x = np.stack([M.signal(L, H), M.F(0.2) * M.signal(L, H, seed=8)])
    ref, g = M.restate(x[0], [(0, p, 0)])
    assert (g < 1).mean() >= 0.1 and (g == 1).mean() >= 0.1 and np.abs(x[1]).max() < M.C
    for name, calls in M.cuts(x.shape[1]).items():
        y = run(make(na, model, 2, {0: p, 1: p}), x, calls)
        assert np.array_equal(y[0], ref), (name, int((y[0] != ref).sum()), int(np.argmax(y[0] != ref)))
        assert np.abs(y).max() <= M.F(M.C)
        assert np.array_equal(y[1, L:], x[1, :-L]) and not np.any(y[1, :L]), name


def test_neighbours_and_no_entry(na, model):
    """Limiters on every third of 70 rows: those rows are the restatement's, the others those of a batch that never enabled the stage;
    an enabled stage without an entry launches nothing."""
    from neuralaudio_amd import capi
    L, H, rows = 64, 300, 70
    x = np.stack([M.signal(L, H, seed=20 + r) for r in range(rows)])
    calls = M.cuts(x.shape[1])["128"]
    plain = run(make(na, model, rows), x, calls)
    launches = capi.load_library().NA_DebugLimiterLaunches()
    assert np.array_equal(run(make(na, model, rows, {}), x, calls), plain)
    assert capi.load_library().NA_DebugLimiterLaunches() == launches
    y = run(make(na, model, rows, {r: M.params(L, H) for r in range(0, rows, 3)}), x, calls)
    assert capi.load_library().NA_DebugLimiterLaunches() == launches + len(calls)
    for r in range(rows):
        if r % 3:
            assert np.array_equal(y[r], plain[r]), r
        else:
            ref, g = M.restate(x[r], [(0, M.params(L, H), 0)])
            assert (g < 1).any() and np.array_equal(y[r], ref), r


def test_set_call_in_mid_signal(na, model):
    """A set call at sample 1024 lowers the ceiling over a ramp of 300 samples and shortens the hold; one at 2048 raises both at once."""
    L, x = 64, np.tile(M.signal(64, 100), 3)[None, :4096]
    sets = [(0, M.params(L, 100), 0), (1024, M.params(L, 10, 0.25), 300), (2048, M.params(L, 500, 0.375), 0)]
    ref, g = M.restate(x[0], sets)
    assert all((g[a:b] < 1).any() for a, b in ((0, 1024), (1024, 2048), (2048, 4096)))
    b = make(na, model, 1, {0: sets[0][1]})
    out = [run(b, x, [128] * 8, close=False)]
    b.SetStreamLimiter(0, sets[1][1], 300)
    out.append(run(b, x[:, 1024:], [100, 1, 923], close=False))
    b.SetStreamLimiter(0, sets[2][1])
    assert b.GetStreamLimiter(0) == sets[2][1]
    out.append(run(b, x[:, 2048:], [2048]))
    y = np.concatenate(out, axis=1)[0]
    assert np.array_equal(y, ref), int(np.argmax(y != ref))
    c = np.concatenate([M.ceiling(0.5, 0.5, 0, np.arange(1024)), M.ceiling(0.5, 0.25, 300, np.arange(1024)), np.full(2048, M.F(0.375))])
    assert np.all(np.abs(y) <= c)


def test_refusals_removal_and_reuse(na, model):
    L, H = 8, 1
    p, x = M.params(L, H), M.signal(L, H)[None, :]
    b = na.Batch(0)
    with pytest.raises(na.NeuralAudioError, match=re.escape("limiter stage not enabled (NA_BatchEnableLimiterStage)")):
        b.SetStreamLimiter(0, p)
    b.close()
    b = make(na, model, 1, {0: p})
    for field, bad in (("lookahead", 48), ("lookahead", 1024), ("hold", 4097), ("ceiling", 0.0), ("ceiling", float("inf"))):
        with pytest.raises(na.NeuralAudioError, match=field):
            b.SetStreamLimiter(0, dict(p, **{field: bad}))
    with pytest.raises(na.NeuralAudioError, match="lookahead belongs to the limiter"):
        b.SetStreamLimiter(0, dict(p, lookahead=16))
    ref = M.restate(x[0], [(0, p, 0)])[0]
    assert np.array_equal(run(b, x, [300], close=False)[0], ref[:300])
    b.SetStreamLimiter(0, None)  # at once: the row comes out undelayed
    assert b.GetStreamLimiter(0) is None and np.array_equal(run(b, x[:, 300:], [200], close=False), x[:, 300:500])
    b.SetStreamLimiter(0, dict(p, lookahead=16))  # a new entry: position 0, silence behind it, whatever the ring holds
    assert np.array_equal(run(b, x, [x.shape[1]])[0], M.restate(x[0], [(0, M.params(16, H), 0)])[0])
    b = na.Batch(0)
    b.EnableLimiterStage()
    with pytest.raises(na.NeuralAudioError, match="SetResampling.*limiter stage"):
        b.SetResampling(44100)
    b.close()


def test_behind_a_mix_group(na, model):
    """Two members summed into row 0 exceed c: the delivered row is the restatement of the sum, and the meter's OUT peak is <= c."""
    L, H = 64, 0
    x = np.stack([M.signal(L, H, seed=3), M.signal(L, H, seed=4)])[:, :1280]
    b = make(na, model, 2, {0: M.params(L, H)})
    b.EnableMixStage(), b.EnableMeterStage()
    b.SetMixGroup([0, 1], [[1.0, 1.0]])
    b.SetStreamMeter(0, {"windowSamples": 1280, "clipLevelIn": 8.0, "clipLevelOut": 8.0})
    y = run(b, x, [128] * 10, close=False)
    b.Synchronize()
    peak = b.ReadStreamMeter(0)["out"]["peak"]
    b.close()
    ref, g = M.restate(x[0] + x[1], [(0, M.params(L, H), 0)])
    assert (g < 1).any() and np.array_equal(y[0], ref) and np.array_equal(y[1], x[1])
    assert peak == np.abs(ref).max() <= M.C
