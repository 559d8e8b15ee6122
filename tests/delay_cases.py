"""Shared pieces of tests/test_delay_cpu.py and tests/test_gpu_delay.py: the delay stage's contract (include/neuralaudio_amd.h) restated
in numpy float32, operation for operation, the case tables and the hook batch.

DelayRef holds one stream's state -- the line w since T0, l, q, the two settings of a fade and k -- and process(x) returns what the
stage makes of the next samples of the row, so any cut into calls can be replayed.  Every operation is one numpy float32 operation
(scalars in the sample loop).  Where no fade runs and both filters are out (aL == 1, aH == 0) a sample depends on nothing younger than
t - D, so runs of up to D samples are computed as arrays: the same operations on the same operands, element by element -- that is what
makes the 2^18-sample line affordable."""
import numpy as np

F = np.float32
FIELDS = ("delaySamples", "feedback", "lowpassCoeff", "highpassCoeff", "wet", "dry")
NOT_ENABLED = "delay stage not enabled \\(NA_BatchEnableDelayStage\\)"
STEP = ["x' = isnan(x) ? 0 : clamp(x, +-1e18f)",
        "d  = w[t - D]                                       (+0 where t - D < 0)",
        "l  = (aL == 1) ? d : fl(l + fl(aL * fl(d - l)))     (aL == 1: l takes d, bit for bit)",
        "if aH == 0: h = l, q left alone;  else: q = fl(q + fl(aH * fl(l - q))), h = fl(l - q)",
        "w[t] = clamp(fl(x' + fl(fb * h)), +-1e30f)",
        "y  = (wet == 0) ? fl(dry * x') : fl(fl(dry * x') + fl(wet * h))"]
BOUNDARY_DELAYS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 299, 300]
BOUNDARY_CALLS = [1, 7, 64, 128, 129, 2048, 2049, 3000]
LONG_DELAYS = [2047, 2048, 2049, 262144]
CPU_DELAYS = [1, 2, 64, 300]
CPU_CUTS = [1, 7, 128, 2049]


def params(delaySamples=100, feedback=0.5, lowpassCoeff=1.0, highpassCoeff=0.0, wet=1.0, dry=1.0):
    return dict(delaySamples=int(delaySamples), feedback=float(F(feedback)), lowpassCoeff=float(F(lowpassCoeff)), highpassCoeff=float(F(highpassCoeff)),
                wet=float(F(wet)), dry=float(F(dry)))


def filtered(delaySamples, feedback=0.6, wet=0.7, dry=0.9):
    """both filters in the loop"""
    return params(delaySamples, feedback, 0.35, 0.02, wet, dry)


def weight(N, k):
    """OutStageWeightAt: 1 for k >= N - 1, else (float)(k + 1) / (float)N"""
    return F(1.0) if k >= N - 1 else F(k + 1) / F(N)


def sanitise(x):
    x = np.asarray(x, F)
    return np.where(np.isnan(x), F(0.0), np.minimum(np.maximum(x, F(-1e18)), F(1e18))).astype(F)


def _ramp(gA, gB, wk):
    if wk == F(1.0):
        return gB
    return gA + (gB - gA) * wk


def _silent(p):
    q = dict(p)
    q["wet"], q["dry"] = 0.0, 1.0
    return q


class DelayRef:
    """one stream of the stage"""

    def __init__(self):
        self.on = False

    # ---- the set calls, as DelayBook makes them ----
    def set(self, p, N=0):
        assert not self.fading(), "a set call while a fade runs is refused"
        if not self.on:
            if p is None:
                return
            self.on, self.to_none = True, False
            self.w, self.t = np.zeros(1 << 12, F), 0  # the line since T0
            self.l = self.q = F(0.0)
            self.B, self.A = dict(p), _silent(p)
        else:
            self.A = self.B
            self.B = dict(p) if p is not None else _silent(self.A)
            self.to_none = p is None
        self.N, self.k = (N, 0) if N > 0 else (0, 0)
        if N == 0:
            self.A = self.B
            if self.to_none:
                self.on = False

    def leave(self):
        self.on = False

    def fading(self):
        return self.on and self.N > 0

    def remaining(self):
        return self.N - self.k if self.fading() else 0

    def target(self):
        return dict(self.B) if self.on and not self.to_none else None

    # ---- the samples ----
    def _tap(self, D):
        return self.w[self.t - D] if self.t - D >= 0 else F(0.0)

    def _room(self, n):
        while self.t + n > len(self.w):
            self.w = np.concatenate([self.w, np.zeros(len(self.w), F)])

    def process(self, x):
        x = np.asarray(x, F)
        y = x.copy()
        if not self.on:
            return y
        n = len(x)
        self._room(n)
        xs = sanitise(x)
        i = 0
        with np.errstate(all="ignore"):
            while i < n and self.on:
                A, B = self.A, self.B
                if self.N == 0 and B["lowpassCoeff"] == 1.0 and B["highpassCoeff"] == 0.0:
                    i += self._run(xs, y, i, min(n - i, B["delaySamples"]))
                    continue
                wk = weight(self.N, self.k) if self.N > 0 else F(1.0)
                DA, DB = A["delaySamples"], B["delaySamples"]
                d = self._tap(DB)
                if wk != F(1.0) and DA != DB:
                    d = (F(1.0) - wk) * self._tap(DA) + wk * d
                fb, wet, dry = (_ramp(F(A[g]), F(B[g]), wk) for g in ("feedback", "wet", "dry"))
                aL, aH = F(B["lowpassCoeff"]), F(B["highpassCoeff"])
                self.l = d if aL == F(1.0) else self.l + aL * (d - self.l)
                if aH == F(0.0):
                    h = self.l
                else:
                    self.q = self.q + aH * (self.l - self.q)
                    h = self.l - self.q
                self.w[self.t] = np.minimum(np.maximum(xs[i] + fb * h, F(-1e30)), F(1e30))
                y[i] = dry * xs[i] if wet == F(0.0) else dry * xs[i] + wet * h
                self.t += 1
                i += 1
                if self.N > 0:
                    self.k += 1
                    if self.k >= self.N:  # the fade has produced its last sample
                        self.N = self.k = 0
                        self.A = self.B
                        if self.to_none:
                            self.on = False  # retired with this sample: the rest of the row is not touched
        return y

    def _run(self, xs, y, i, c):
        """c <= D samples with no fade and no filter: arrays"""
        B = self.B
        D, fb, wet, dry = B["delaySamples"], F(B["feedback"]), F(B["wet"]), F(B["dry"])
        lo = self.t - D
        d = np.zeros(c, F)
        if lo + c > 0:
            d[max(0, -lo):] = self.w[max(lo, 0):lo + c]
        x = xs[i:i + c]
        self.w[self.t:self.t + c] = np.minimum(np.maximum(x + fb * d, F(-1e30)), F(1e30))
        y[i:i + c] = dry * x if wet == F(0.0) else dry * x + wet * d
        self.l = d[-1]
        self.t += c
        return c


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))


def first_difference(a, b):
    d = np.flatnonzero(np.ascontiguousarray(a, F).view(np.uint32) != np.ascontiguousarray(b, F).view(np.uint32))
    return (int(d[0]), len(d)) if len(d) else None


def noise(n, seed, gain=0.25):
    return (gain * np.random.default_rng(seed).standard_normal(n)).astype(F)


def cuts(total, lengths):
    """call lengths from `lengths`, in turn, that add up to `total`"""
    calls, left, i = [], total, 0
    while left > 0:
        n = min(lengths[i % len(lengths)], left)
        calls.append(n)
        left -= n
        i += 1
    return calls


class HookBatch:
    """`rows` rows (BossWN-nano streams that never run) with the stage enabled: the hook runs the stage on host rows."""

    def __init__(self, na, nano, rows, max_delay):
        self.b = na.Batch(0)
        assert self.b.AddStreams(nano, rows, doPrewarm=False) == 0
        self.b.EnableDelayStage(max_delay)
        self.rows = rows

    def run(self, x, calls=None, stride=lambda n: n):
        """the stage over x[rows, total], cut into `calls`; every call's block has rows stride(n) floats apart"""
        calls = [x.shape[1]] if calls is None else calls
        assert sum(calls) == x.shape[1]
        out, pos = [], 0
        for n in calls:
            block = np.full((self.rows, stride(n)), F(7.0))
            block[:, :n] = x[:, pos:pos + n]
            self.b.DebugRunDelayStage(block, n)
            assert np.all(block[:, n:] == F(7.0)), "the stage wrote past the end of a row"
            out.append(block[:, :n].copy())
            pos += n
        return np.concatenate(out, axis=1)

    def close(self):
        self.b.close()
