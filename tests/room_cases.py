"""The room stage's contract (include/neuralaudio_amd.h, csrc/room_stage.h) restated in numpy float32, operation for operation, and the
parameter table tests/test_room_cpu.py (no device) and tests/test_gpu_room.py (the C ABI on the device) share.  Every floating-point
operation below is one numpy float32 operation, so each is rounded separately; nothing is contracted; subnormals are kept.

No line is shorter than 128 samples, so the restatement evaluates runs of up to 128 samples as arrays; a run reads nothing it writes."""
import math

import numpy as np

from mod_cases import ramp, weight, x_prime

F = np.float32
LINES, MIN_LINE, MAX_LINE, RUN = 8, 128, 16384, 128
PAD = MAX_LINE + 2                       # zeros in front of the lines: L_i[t] = +0 for t < 0
MAX_FEEDBACK = float(F(1.0 / math.sqrt(8.0)))


def params(lines, feedback, damp=0.0, wet=1.0, dry=1.0):
    """a dict of the NA_RoomParams fields; floats already float32; a scalar feedback goes to every line"""
    feedback = [feedback] * LINES if np.isscalar(feedback) else feedback
    return dict(lineSamples=[int(v) for v in lines], feedback=[float(F(v)) for v in feedback], damp=float(F(damp)), wet=float(F(wet)), dry=float(F(dry)))


def prime_from(v):
    while v < 2 or any(v % f == 0 for f in range(2, math.isqrt(v) + 1)):
        v += 1
    return v


def from_seconds(rate, size_ms, decay_seconds, damp, wet_db, dry_db):
    """NA_RoomParamsFromSeconds in Python floats (double), each value rounded once"""
    gain = lambda db: 0.0 if db == float("-inf") else float(F(math.pow(10.0, db / 20.0)))
    lines = []
    for i in range(LINES):
        want = rate * size_ms / 1000.0 * math.pow(2.0, -i / 8.0)
        lines.append(max(MIN_LINE, MAX_LINE if want > MAX_LINE else min(MAX_LINE, prime_from(max(2, math.ceil(want))))))
    return dict(lineSamples=lines, feedback=[float(F(math.pow(10.0, -3.0 * n / (decay_seconds * rate)) / math.sqrt(8.0))) for n in lines],
                damp=float(F(damp)), wet=gain(wet_db), dry=gain(dry_db))


class RoomRef:
    """one stream's room: set calls, fades and the eight lines, by the contract"""

    def __init__(self):
        self.has = False

    def set(self, p, N):
        """p: a dict of the fields, or None: no room; the caller has seen to it that no fade is running"""
        assert not (self.has and self.fading)
        if not self.has:
            if p is None:
                return
            self.has, self.to_none = True, False
            self.A, self.B = dict(p, wet=0.0, dry=1.0), dict(p)
            self.L = np.zeros((LINES, PAD), F)
        else:
            self.A = self.B
            self.B = dict(p) if p is not None else dict(self.A, wet=0.0, dry=1.0)
            self.to_none = p is None
        self.N, self.k, self.fading = N, 0, N > 0
        if not self.fading:
            self.A = self.B
            self.has = not self.to_none

    def energy(self):
        """V = sum_i (sum of L_i^2 over the len_i samples r_i has yet to read + damp * the square of the one only q_i has yet to read), in
        float64.  Without input V(t + 1) - V(t) = sum L_i[t]^2 - sum (keep r_i^2 + damp q_i^2) <= 0 in exact arithmetic: sum L_i^2 <=
        sum h_i^2 / 8 = sum d_i^2 (fb_i <= 1 / sqrt 8, H8 / sqrt 8 orthogonal) and d_i^2 <= keep r_i^2 + damp q_i^2 (convexity)."""
        sq = self.L.astype(np.float64) ** 2
        return sum(float(np.sum(sq[i, -n:]) + self.B["damp"] * sq[i, -n - 1]) for i, n in enumerate(self.B["lineSamples"]))

    def run(self, x):
        """a processing call: returns what replaces the row's samples (a retired entry leaves the rest of the row as it was)"""
        x = np.asarray(x, F)
        y = x.copy()
        if not self.has or len(x) == 0:
            return y
        n = len(x)
        live = n if not self.to_none else max(0, min(n, self.N - self.k))
        t0 = self.L.shape[1]
        L = np.concatenate([self.L, np.zeros((LINES, live), F)], axis=1)
        A, B = self.A, self.B
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            for j0 in range(0, live, RUN):
                j = np.arange(j0, min(live, j0 + RUN), dtype=np.int64)
                wk = weight(self.N, self.k + j) if self.fading else np.ones(len(j), F)
                xs = x_prime(x[j])
                damp = ramp(A["damp"], B["damp"], wk)
                keep = (F(1.0) - damp).astype(F)
                d = []
                for i in range(LINES):
                    taps = []
                    for back in (0, 1):
                        tap = L[i, t0 + j - B["lineSamples"][i] - back]
                        if A["lineSamples"][i] != B["lineSamples"][i]:
                            old = L[i, t0 + j - A["lineSamples"][i] - back]
                            blend = (((F(1.0) - wk).astype(F) * old).astype(F) + (wk * tap).astype(F)).astype(F)
                            tap = np.where(wk == F(1.0), tap, blend).astype(F)
                        taps.append(tap)
                    d.append(((taps[0] * keep).astype(F) + (taps[1] * damp).astype(F)).astype(F))
                h = list(d)
                for span in (1, 2, 4):
                    for i in range(LINES):
                        if not i & span:
                            h[i], h[i + span] = (h[i] + h[i + span]).astype(F), (h[i] - h[i + span]).astype(F)
                for i in range(LINES):
                    L[i, t0 + j] = (xs + (ramp(A["feedback"][i], B["feedback"][i], wk) * h[i]).astype(F)).astype(F)
                s = (((d[0] - d[1]).astype(F) + (d[2] - d[3]).astype(F)).astype(F) + ((d[4] - d[5]).astype(F) + (d[6] - d[7]).astype(F)).astype(F)).astype(F)
                y[j] = ((ramp(A["dry"], B["dry"], wk) * xs).astype(F) + (ramp(A["wet"], B["wet"], wk) * s).astype(F)).astype(F)
        self.L = L[:, -PAD:].copy()
        if self.fading:
            self.k = min(self.N, self.k + n)
            if self.k >= self.N:
                self.fading, self.A = False, self.B
                self.has = not self.to_none
        return y


def run_cuts(ops, x, cuts):
    """fresh references over x[rows, total] cut into calls of `cuts` samples; ops: {call index: [(row, params or None, fade)]}"""
    refs = [RoomRef() for _ in range(x.shape[0])]
    out, pos = [], 0
    for c, n in enumerate(cuts):
        for row, p, fade in ops.get(c, ()):
            refs[row].set(p, fade)
        out.append(np.stack([ref.run(x[row, pos:pos + n]) for row, ref in enumerate(refs)]))
        pos += n
    return np.concatenate(out, axis=1), refs


def cuts_of(total, sizes):
    """calls of `sizes` samples, taken in turn, that add up to `total`"""
    calls = []
    while sum(calls) < total:
        calls.append(min(sizes[len(calls) % len(sizes)], total - sum(calls)))
    return calls


# the parameter table: (maxLineSamples, lines) -- every line 128 (the taps at t - 128 and t - 129 cross the piece's edge); mixed primes up
# to the maximum; one line AT the maximum of the smallest stage, whose rings of 512 wrap inside the windows
EDGES = {"all-128": (256, [128] * 8), "primes": (1024, [1021, 769, 521, 383, 257, 131, 129, 128]), "at-max": (256, [256, 255, 193, 128, 251, 130, 211, 149])}
CUTS = [1, 127, 128, 129, 333]
