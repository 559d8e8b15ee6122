"""The limiter stage's contract (include/neuralaudio_amd.h, csrc/limiter_stage.h) restated in numpy float32 in its plain form -- a
windowed minimum and an explicit pairwise tree, not the kernel's doubling passes -- and the cases the CPU and GPU tests share.  Helper
code only."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

F = np.float32
C = 0.5  # the cases' ceiling
# (lookahead, hold): the smallest L, W = L + H + 1 a power of two and not, W longer than a piece
CASES = [(8, 0), (8, 1), (64, 300), (64, 4031), (512, 4096)]


def params(L, H, c=C):
    return {"lookahead": L, "hold": H, "ceiling": c}


def signal(L, H, seed=7, c=C):
    """quiet noise below c with two bursts of up to 4 c in it; every quiet stretch is longer than W + L (= 2 L + H + 1)"""
    K = 2 * L + H
    rng = np.random.default_rng(seed)
    quiet = lambda: rng.uniform(-0.9 * c, 0.9 * c, K + max(200, K // 8))
    burst = lambda: rng.uniform(-4 * c, 4 * c, 300)
    return np.concatenate([quiet(), burst(), quiet(), burst(), quiet()]).astype(F)


def cuts(n):
    """the same n samples as 128-sample calls, as one-sample calls followed by 37-sample calls, and as one call (longer than a piece)"""
    even = lambda first, size: first + [size] * ((n - sum(first)) // size) + [(n - sum(first)) % size] * ((n - sum(first)) % size > 0)
    return {"128": even([], 128), "1+37": even([1, 1, 1], 37), "one": [n]}


def ceiling(frm, to, R, k):
    w = (k + 1).astype(F) / F(max(R, 1))
    return np.where(k < 0, F(frm), np.where(k >= R - 1, F(to), F(frm) + (F(to) - F(frm)) * w)).astype(F)


def restate(x, sets):
    """(y, g) of the row x: sets = [(position of the set call, params, rampSamples), ...], the first at 0 (it creates the entry)"""
    x, n, L = np.asarray(x, F), len(x), sets[0][1]["lookahead"]
    y, g, frm = np.zeros(n, F), np.ones(n, F), F(sets[0][1]["ceiling"])
    for i, (t0, p, R) in enumerate(sets):
        t1, H, to = (sets[i + 1][0] if i + 1 < len(sets) else n), p["hold"], F(p["ceiling"])
        R = R if i else 0
        t = np.arange(t0 - (2 * L + H) + 1, t1)  # everything the outputs t0 .. t1 - 1 read
        c = ceiling(frm, to, R, t - t0)
        a = np.where(t >= 0, np.abs(x[np.maximum(t, 0)]), F(0))
        need = np.where(a > c, c / np.where(a > c, a, F(1)), F(1)).astype(F)
        m = sliding_window_view(need, L + H + 1).min(axis=1)
        s = sliding_window_view(m, L).copy()  # row r: m[t - L + 1 .. t] of output t0 + r
        while s.shape[1] > 1:
            s = s[:, 0::2] + s[:, 1::2]
        out = np.arange(t0, t1)
        g[t0:t1] = s[:, 0] * F(1.0 / L)
        v = np.where(out >= L, x[np.maximum(out - L, 0)], F(0)) * g[t0:t1]
        y[t0:t1] = np.minimum(np.maximum(v, -c[-len(out):]), c[-len(out):])
        frm = ceiling(frm, to, R, np.array([t1 - t0 - 1]))[0]
    return y, g
