"""The limiter stage without a GPU (tests/limiter_cases.py): NA_LimiterParamsFromDb, and the conditions that give the GPU tests their
meaning."""
import numpy as np
import pytest

import limiter_cases as M


def test_params_from_db():
    import neuralaudio_amd as na
    assert na.limiter_params_from_db(48000, -6.0, 1.5, 10.0) == {"lookahead": 64, "hold": 480, "ceiling": float(np.float32(10 ** -0.3))}
    assert na.limiter_params_from_db(48000, 0.0, 2.0, 0.0)["lookahead"] == 64  # 96 samples = 1.5 x 64: the smaller one
    assert na.limiter_params_from_db(48000, 0.0, 2.01, 0.0)["lookahead"] == 128
    assert [na.limiter_params_from_db(48000, 0.0, ms)["lookahead"] for ms in (0.0, 100.0)] == [8, 512]
    for bad, field in (((48000, 0.0, 1.5, 90.0), "hold"), ((48000, float("nan"), 1.5, 0.0), "ceiling"), ((0, 0.0, 1.5, 0.0), "sampleRate")):
        with pytest.raises(na.NeuralAudioError, match=field):
            na.limiter_params_from_db(*bad)


@pytest.mark.parametrize("L,H", M.CASES)
def test_cases_limit_and_pass(L, H):
    """At least a tenth of every case's samples pass at g = 1 and a tenth are reduced; nothing exceeds c; the gain alone does the
    limiting (g <= need[t - L]); a quiet sample comes out bit for bit, L samples late."""
    x = M.signal(L, H)
    y, g = M.restate(x, [(0, M.params(L, H), 0)])
    assert len(x) > 1024 and (g == 1).mean() >= 0.1 and (g < 1).mean() >= 0.1 and g.max() <= 1
    assert np.abs(y).max() <= M.F(M.C) and np.abs(x).max() > 3 * M.C
    xd = np.concatenate([np.zeros(L, M.F), x[:-L]])
    assert np.abs(xd * g).max() <= M.F(M.C)
    assert np.array_equal(y[g == 1], xd[g == 1])
