"""Shared pieces of tests/test_tuner_cpu.py and tests/test_gpu_tuner.py: the tuner stage's contract (include/neuralaudio_amd.h) restated
in numpy -- one float32 product per sample, then int64 --, the two host helpers restated in Python floats, the case lists, and the
runner that drives a batch with tuners.

Everything behind the one product is an integer, so everything that is compared is compared for equality: a reading is a dict of
integers, and the expected one is the restatement's reading for the evaluation index the batch reports.

A scenario is a list of call lengths and, per call index, the operations issued in front of that call:
  ("tuner", stream, params)  ("untuner", stream)  ("park", stream)  ("activate", stream)"""
import itertools
import math

import numpy as np

import handover_cases as H

F = np.float32
FIELDS = ("decimation", "windowSamples", "minLag", "maxLag", "hopSamples", "phase", "thresholdQ10", "minEnergy")
READING = ("evaluations", "position", "r", "e0", "e", "lag", "decimation")
CONTRACT = ["c    = (x is NaN) ? 0 : min(max(x, -1.0f), 1.0f)",
            "q[p] = (int) trunc(c * 32767.0f)                      (one f32 product, then integers only)",
            "d[m] = q[mD] + q[mD+1] + ... + q[mD+D-1]   for m >= 0;   d[m] = 0 for m < 0        (|d| < 2^18)",
            "evaluation k = 0, 1, ... ends at m_k = phase + (k+1)*H - 1 and belongs to the call that holds position (m_k+1)*D - 1",
            "for t = 0 .. maxLag+1, signed / unsigned 64-bit:",
            "r[t] = sum over j = 0 .. W-1 of d[m_k - j] * d[m_k - j - t]                      (|r| < 2^47)",
            "e[t] = sum over j = 0 .. W-1 of d[m_k - j - t] * d[m_k - j - t]                  (e[0] = r[0])",
            "lag = 0 if e[0] < minEnergy",
            "z   = the smallest t in [1, maxLag+1] with r[t] <= 0;          none: lag = 0",
            "candidates: t in [max(minLag, z+1), maxLag] with r[t] > 0 and r[t] > r[t-1] and r[t] >= r[t+1];   none: lag = 0",
            "rmax = max of r[t] over the candidates",
            "lag  = the smallest candidate t with 1024 * r[t] >= thresholdQ10 * rmax              (< 2^57)"]
STRUCTS = ["typedef struct NA_TunerParams  { int decimation, windowSamples, minLag, maxLag, hopSamples, phase, thresholdQ10, reserved;\n"
           "                                 unsigned long long minEnergy; } NA_TunerParams;",
           "typedef struct NA_TunerReading { unsigned long long evaluations; long long position; long long r[3];\n"
           "                                 unsigned long long e0, e[3]; int lag, decimation; } NA_TunerReading;",
           "typedef struct NA_TunerInfo    { int numTuners; long long deviceBytes; } NA_TunerInfo;"]
LIMITS = [(dict(decimation=0), "decimation must lie in [1, 8]"), (dict(decimation=9), "decimation must lie in [1, 8]"),
          (dict(windowSamples=31), "windowSamples must lie in [32, 2048]"), (dict(windowSamples=2049), "windowSamples must lie in [32, 2048]"),
          (dict(maxLag=3, minLag=2), "maxLag must lie in [4, 1024]"), (dict(maxLag=1025), "maxLag must lie in [4, 1024]"),
          (dict(minLag=1), "minLag must lie in [2, maxLag]"), (dict(minLag=65, maxLag=64), "minLag must lie in [2, maxLag]"),
          (dict(hopSamples=15), "hopSamples must lie in [16, 65536]"), (dict(hopSamples=65537), "hopSamples must lie in [16, 65536]"),
          (dict(phase=-1), "phase must lie in [0, hopSamples)"), (dict(hopSamples=64, phase=64), "phase must lie in [0, hopSamples)"),
          (dict(thresholdQ10=511), "thresholdQ10 must lie in [512, 1024]"), (dict(thresholdQ10=1025), "thresholdQ10 must lie in [512, 1024]")]
NOT_ENABLED = "tuner stage not enabled (NA_BatchEnableTunerStage)"


def params(decimation=1, windowSamples=100, minLag=2, maxLag=64, hopSamples=37, phase=0, thresholdQ10=922, minEnergy=None):
    if minEnergy is None:
        minEnergy = windowSamples * (33 * decimation) ** 2
    return dict(decimation=int(decimation), windowSamples=int(windowSamples), minLag=int(minLag), maxLag=int(maxLag), hopSamples=int(hopSamples),
                phase=int(phase), thresholdQ10=int(thresholdQ10), minEnergy=int(minEnergy))


def quantise(x):
    """c and q of the contract: float32 in, int64 out"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        c = np.where(np.isnan(x), F(0), np.minimum(np.maximum(x, F(-1.0)), F(1.0))).astype(np.float32)
        p = c * F(32767.0)
    assert p.dtype == np.float32
    return np.trunc(p).astype(np.int64)


class TunerRef:
    """One stream's tuner.  feed(x) takes a call's input row; reading(k) is evaluation k's; latest() the reading a synchronised batch
    shows: the last evaluation whose end has gone by (the last of a call is always computed)."""

    def __init__(self, p):
        self.p = dict(p)
        self.q = np.zeros(0, np.int64)
        self.ends = []  # per call: evaluation ends that have gone by after it
        self._cache = {}

    @property
    def position(self):
        return len(self.q)

    def feed(self, x):
        self.q = np.concatenate([self.q, quantise(x)])
        self.ends.append(self.evaluations)

    @property
    def evaluations(self):
        have = self.position // self.p["decimation"]
        return max(0, (have - self.p["phase"]) // self.p["hopSamples"]) if have >= self.p["phase"] else 0

    def computed(self):
        """the evaluation indices the stage computes for the cut fed so far: the last of every call that holds one"""
        out, before = [], 0
        for after in self.ends:
            if after > before:
                out.append(after - 1)
            before = after
        return out

    def reading(self, k):
        if k in self._cache:
            return self._cache[k]
        p = self.p
        D, W, top = p["decimation"], p["windowSamples"], p["maxLag"] + 1
        m = p["phase"] + (k + 1) * p["hopSamples"] - 1
        assert (m + 1) * D <= self.position, "evaluation %d has not ended" % k
        d = self.q[:(m + 1) * D].reshape(m + 1, D).sum(axis=1)
        assert np.all(np.abs(d) < 1 << 18)
        span = np.concatenate([np.zeros(W + top, np.int64), d])[-(W + top):]  # d[m - W - top + 1 .. m], zeros below index 0
        a = span[top:]
        windows = np.lib.stride_tricks.sliding_window_view(span, W)  # windows[i] = d[m - W - top + 1 + i ...]: lag t is row top - t
        r = (windows @ a)[::-1]
        e = np.einsum("ij,ij->i", windows, windows)[::-1]
        assert r.dtype == np.int64 and len(r) == top + 1 and e[0] == r[0] and np.all(np.abs(r) < 1 << 47)
        r, e = [int(v) for v in r], [int(v) for v in e]
        lag = 0
        zeros = [t for t in range(1, top + 1) if r[t] <= 0]
        if e[0] >= p["minEnergy"] and zeros:
            z = zeros[0]
            cand = [t for t in range(max(p["minLag"], z + 1), p["maxLag"] + 1) if r[t] > 0 and r[t] > r[t - 1] and r[t] >= r[t + 1]]
            if cand:
                rmax = max(r[t] for t in cand)
                lag = min(t for t in cand if 1024 * r[t] >= p["thresholdQ10"] * rmax)
        out = {"evaluations": k + 1, "position": (m + 1) * D, "r": [r[lag + i] for i in (-1, 0, 1)] if lag else [0, 0, 0], "e0": e[0],
               "e": [e[lag + i] for i in (-1, 0, 1)] if lag else [0, 0, 0], "lag": lag, "decimation": D}
        self._cache[k] = out
        return out

    def latest(self):
        return self.reading(self.evaluations - 1) if self.evaluations > 0 else None


def pitch(reading, sample_rate):
    """NA_TunerPitch restated: (hz, clarity), None when lag == 0"""
    if reading["lag"] == 0:
        return None
    n = []
    for i in range(3):
        den = float(reading["e0"]) + float(reading["e"][i])
        n.append(2.0 * float(reading["r"][i]) / den if den != 0.0 else 0.0)
    den = n[0] - 2.0 * n[1] + n[2]
    off = min(1.0, max(-1.0, 0.5 * (n[0] - n[2]) / den)) if den < 0.0 else 0.0
    return sample_rate / (reading["decimation"] * (reading["lag"] + off)), n[1] - 0.25 * (n[0] - n[2]) * off


def params_from_range(sample_rate, lowest, highest, per_second):
    """NA_TunerParamsFromRange restated; None where it fails (maxLag above 1024)"""
    D = max([d for d in range(1, 9) if sample_rate / (d * highest) >= 16.0] or [1])
    max_lag = math.ceil(sample_rate / (D * lowest)) + 2
    if max_lag > 1024:
        return None
    W = min(2048, max(32, 3 * max_lag))
    return params(D, W, max(2, math.floor(sample_rate / (D * highest)) - 1), max_lag, max(16, math.floor(sample_rate / (D * per_second) + 0.5)), 0, 922,
                  W * (33 * D) ** 2)


def cents(hz, f0):
    return 1200.0 * math.log2(hz / f0)


# ---- the cases ----

TOTAL = 1200
CUTS = {"1": [1] * TOTAL, "7": [7] * (TOTAL // 7) + [TOTAL % 7], "63": [63] * 19 + [3], "64": [64] * 18 + [48], "65": [65] * 18 + [30], "100": [100] * 12,
        "128": [128] * 9 + [48], "333": [333] * 3 + [201], "ragged": H.ragged(TOTAL)}
SHAPES = [(32, 4), (100, 63), (100, 64), (257, 65), (257, 130)]  # (W, maxLag): around one and two waves of lags


def cut_cases():
    """24 tuners: every D in {1, 2, 3, 8} with every (W, maxLag) of SHAPES, H in {16, 37, W} and phase in {0, H - 1} in turn (a hop that
    1200 samples do not reach at that D becomes 37), and four more that put H = 16 and H = W beside D = 8 and D = 1"""
    out = []
    combos = list(itertools.product((1, 2, 3, 8), SHAPES)) + [(8, (32, 4)), (8, (100, 64)), (1, (257, 130)), (1, (100, 63))]
    for i, (D, (W, max_lag)) in enumerate(combos):
        hop = [16, 37, W][i % 3] if i < 20 else [16, W, W, 16][i - 20]
        phase = [0, hop - 1][(i // 3) % 2] if i < 20 else [hop - 1, 0, hop - 1, 0][i - 20]
        if (phase + hop) * D > TOTAL:
            hop, phase = 37, min(phase, 36)
        out.append(params(D, W, 2, max_lag, hop, phase))
    return out


def pitched(total, period, seed, level=0.5, noise=0.02):
    """a tone of `period` samples with a weak fundamental and a strong second harmonic, and a little noise"""
    t = np.arange(total) * (2.0 * np.pi / period)
    rng = np.random.default_rng(seed)
    x = 0.5 * np.sin(t) + 1.0 * np.sin(2 * t + 0.3) + 0.4 * np.sin(3 * t + 1.1)
    return (level * x / np.max(np.abs(x)) + noise * rng.standard_normal(total)).astype(np.float32)


SPECIAL = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 1.0, -1.0, 1.0000001, -1.5, 0.99999994, -0.0, 1e-45, 3.0518044e-05, 3.05e-05, -6.2e-05], np.float32)


def cut_signal(seed=0):
    """[ROWS, 1200]: every row its own period (23.7 .. 61 samples); rows 4 and 8 also carry the special inputs"""
    x = np.stack([pitched(TOTAL, 23.7 + 3.4 * r, 700 + 10 * seed + r) for r in range(H.ROWS)])
    for row, first in ((4, 2), (8, 9)):
        x[row, first + 11 * np.arange(len(SPECIAL))] = SPECIAL
    return x


def sawtooth(total, period, amplitude=20000):
    """integers on the quantiser's grid: q == the ramp exactly"""
    ramp = (np.arange(total) % period) * (2 * amplitude // period) - amplitude
    x = (ramp.astype(np.float64) + 0.5 * np.sign(ramp)) / 32767.0
    x = x.astype(np.float32)
    assert np.array_equal(quantise(x), ramp)
    return x


def harmonic_tone(f0, sample_rate, total, peak):
    t = np.arange(total) / sample_rate
    x = sum(a * np.sin(2 * np.pi * f0 * (h + 1) * t) for h, a in enumerate((0.6, 1.0, 0.7, 0.4, 0.3)))
    return (peak * x / np.max(np.abs(x))).astype(np.float32)


NOTES = (41.20, 55.0, 61.74, 82.41, 98.0, 110.0, 146.83, 196.0, 246.94, 329.63, 440.0, 523.25)


# ---- the batch under test (the twelve rows of handover_cases) ----

def make_batch(na, models, tuner=True, resample=None):
    b = H.make_batch(na, models, stage=False, resample=resample)
    if tuner:
        b.EnableTunerStage()
    return b


def drive(batch, op, tuner):
    if op[0] == "tuner":
        if tuner:
            batch.SetStreamTuner(op[1], op[2])
    elif op[0] == "untuner":
        if tuner:
            batch.SetStreamTuner(op[1], None)
    elif op[0] == "park":
        batch.ParkStream(op[1])
    elif op[0] == "activate":
        batch.ActivateStream(op[1], 1.0)
    else:
        raise ValueError(op)


def run_tuners(batch, runner, x, calls, ops, refs=None, every_call=True):
    """Drives `batch` through `runner` over x in `calls`, the operations of ops[i] in front of call i; behind a synchronise after every
    call (every_call) or after the last one, every tuned row's reading must be the restatement's newest.  Returns (rows, refs, the
    readings after the last call)."""
    refs = {} if refs is None else refs
    got, pos, last = [], 0, {}
    for i, n in enumerate(calls):
        for op in ops.get(i, ()):
            drive(batch, op, True)
            if op[0] == "tuner":
                refs[op[1]] = TunerRef(op[2])
            elif op[0] in ("untuner", "park"):
                refs.pop(op[1], None)
        xs = x[:, pos:pos + n]
        got.append(runner.call(xs))
        for s, ref in refs.items():
            ref.feed(xs[s])
        if every_call or i == len(calls) - 1:
            batch.Synchronize()
            for s, ref in refs.items():
                last[s] = batch.ReadStreamTuner(s)
                assert last[s] == ref.latest(), ("call", i, "n", n, "row", s, ref.p, last[s], ref.latest())
        pos += n
    return np.concatenate(got, axis=1), refs, last
