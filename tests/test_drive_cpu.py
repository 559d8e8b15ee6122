"""The drive stage without a GPU (tests/drive_cases.py): the prototype's response, and the float32 restatement against float64."""
import numpy as np
import pytest

import drive_cases as D


@pytest.mark.parametrize("L", [2, 4, 8])
def test_prototype_response(L):
    h, j = D.prototype(L), np.arange(L * D.T + 1)
    db = lambda f: 20 * np.log10(np.maximum(np.abs(np.exp(-2j * np.pi * np.outer(np.atleast_1d(f), j) / L) @ h), 1e-30))
    f = np.linspace(0, L / 2, 8001)
    assert abs(h.sum() - 1) < 1e-15
    assert np.abs(db(f[f <= 0.4])).max() <= 0.00025
    assert abs(db(20 / 48)[0] + 3.9e-3) < 1e-4
    assert db(f[f >= 0.6]).max() <= -90.9


@pytest.mark.parametrize("case", D.CASES)
def test_float32_restatement_within_half_the_gpu_bound(case):
    p, x = D.params(case), D.signal()
    ref = D.restate(x, p)
    assert np.sqrt(np.mean(ref ** 2)) > 1e-3
    frac = D.worst_window(D.restate(x, p, dtype=np.float32), ref, p["level"])
    print(case, "float32 / bound =", frac)
    assert frac < 0.5
