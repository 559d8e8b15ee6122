"""The EQ stage's contract (include/neuralaudio_amd.h, "the EQ stage") restated in Python float64 / numpy float32, and the case lists of
tests/test_eq_cpu.py and tests/test_gpu_eq.py.

Every Python float operation is one IEEE double operation and every numpy float32 operation one IEEE single operation, each rounded to
nearest even, and neither language contracts a multiply and an add: `eq_sample` below IS the contract, scalar and obvious.  The tests
compare with it bit for bit."""
import math

import numpy as np

F = np.float32
MAX_SECTIONS = 8
FIELDS = ("b0", "b1", "b2", "a1", "a2")
KINDS = {"lowpass": 0, "highpass": 1, "lowshelf": 2, "highshelf": 3, "peaking": 4}
SECTION_COUNTS = (1, 3, 8)
CALL_SIZES = (1, 2, 7, 8, 9, 127, 128, 129, 300)  # the tile edge (128) and calls shorter than the pipeline is deep (8)
FADES = (0, 1, 5, 128, 200)
LIMIT = F(1e18)


def sanitize(x):
    """x' = isnan(x) ? 0 : clamp(x, +-1e18f), in f32"""
    x = F(x)
    if np.isnan(x):
        return F(0.0)
    return min(max(x, -LIMIT), LIMIT)


def eq_sample(sections, state, x):
    """One sample through one cascade: sections a list of (b0, b1, b2, a1, a2) Python floats, state a list of [x1, x2, y1, y2] per
    section (updated in place), x the f32 input sample.  Returns o = (float)v."""
    v = float(sanitize(x))
    for (b0, b1, b2, a1, a2), s in zip(sections, state):
        acc = b0 * v
        acc = acc + b1 * s[0]
        acc = acc + b2 * s[1]
        acc = acc - a1 * s[2]
        acc = acc - a2 * s[3]
        s[1] = s[0]
        s[0] = v
        s[3] = s[2]
        s[2] = acc
        v = acc
    with np.errstate(over="ignore"):
        return F(v)


def weight32(N, k):
    """OutStageWeightAt: w = (min(k, N-1) + 1) / N in f32"""
    if k >= N - 1:
        return F(1.0)
    return F(k + 1) / F(N)


def mix(N, k, oA, oB):
    """the k-th sample after a set call of length N: fl32(fl32(fl32(1 - w) * o_A) + fl32(w * o_B)); o_B itself where w == 1"""
    w = weight32(N, k)
    if w == F(1.0):
        return oB
    with np.errstate(over="ignore", invalid="ignore"):
        return F(F(F(1.0) - w) * oA) + F(w * oB)


def tuples(sections):
    return [tuple(float(s[name]) for name in FIELDS) for s in sections]


class EqRef:
    """One stream: the cascade it has (fades to), the one it fades from, the fade's position."""

    def __init__(self):
        self.sec, self.state = [], []      # B: the target
        self.from_sec, self.from_state = None, None
        self.N = self.k = 0
        self.fading = False

    def set(self, sections, N=0):
        """a set call: B starts from A's state, sections [0, min(S_A, S_B)); the others at zero"""
        assert not self.fading
        sections = tuples(sections or [])
        if not self.sec and not sections:
            return  # flat to flat: nothing
        keep = min(len(self.sec), len(sections))
        state = [list(self.state[i]) if i < keep else [0.0] * 4 for i in range(len(sections))]
        if N > 0:
            self.from_sec, self.from_state = self.sec, self.state
            self.fading, self.N, self.k = True, N, 0
        self.sec, self.state = sections, state

    def leave(self):
        self.__init__()

    @property
    def remaining(self):
        return self.N - self.k if self.fading else 0

    @property
    def is_entry(self):
        """as the book sees it BETWEEN calls"""
        return bool(self.sec) or self.fading

    def run(self, x):
        out = np.empty(len(x), np.float32)
        for t, xs in enumerate(np.asarray(x, np.float32)):
            o = eq_sample(self.sec, self.state, xs)
            if self.fading:
                oA = eq_sample(self.from_sec, self.from_state, xs)
                o = mix(self.N, self.k, oA, o)
                self.k += 1
                if self.k >= self.N:
                    self.fading, self.from_sec, self.from_state = False, None, None
            out[t] = o
        return out


# ---- the cookbook, restated ----

def design(kind, fs, f, q, db=0.0):
    """RBJ cookbook, Q form, divided through by a0; a dict of the NA_EqSection fields"""
    kind = KINDS.get(kind, kind)
    w0 = 2.0 * math.pi * f / fs
    cw, sw = math.cos(w0), math.sin(w0)
    alpha = sw / (2.0 * q)
    A = 10.0 ** (db / 40.0)
    if kind == 0:
        b = ((1 - cw) / 2, 1 - cw, (1 - cw) / 2)
        a = (1 + alpha, -2 * cw, 1 - alpha)
    elif kind == 1:
        b = ((1 + cw) / 2, -(1 + cw), (1 + cw) / 2)
        a = (1 + alpha, -2 * cw, 1 - alpha)
    elif kind == 4:
        b = (1 + alpha * A, -2 * cw, 1 - alpha * A)
        a = (1 + alpha / A, -2 * cw, 1 - alpha / A)
    elif kind == 2:
        sq = 2 * math.sqrt(A) * alpha
        b = (A * ((A + 1) - (A - 1) * cw + sq), 2 * A * ((A - 1) - (A + 1) * cw), A * ((A + 1) - (A - 1) * cw - sq))
        a = ((A + 1) + (A - 1) * cw + sq, -2 * ((A - 1) + (A + 1) * cw), (A + 1) + (A - 1) * cw - sq)
    elif kind == 3:
        sq = 2 * math.sqrt(A) * alpha
        b = (A * ((A + 1) + (A - 1) * cw + sq), -2 * A * ((A - 1) + (A + 1) * cw), A * ((A + 1) + (A - 1) * cw - sq))
        a = ((A + 1) - (A - 1) * cw + sq, 2 * ((A - 1) - (A + 1) * cw), (A + 1) - (A - 1) * cw - sq)
    else:
        raise ValueError(kind)
    return dict(b0=b[0] / a[0], b1=b[1] / a[0], b2=b[2] / a[0], a1=a[1] / a[0], a2=a[2] / a[0])


DESIGNS = [(0, 48000.0, 8000.0, 0.707, 0.0), (1, 48000.0, 80.0, 0.707, 0.0), (2, 48000.0, 120.0, 0.8, 6.0), (3, 44100.0, 6000.0, 0.6, -9.0),
           (4, 48000.0, 750.0, 1.4, 4.5), (4, 96000.0, 3000.0, 4.0, -12.0), (2, 44100.0, 300.0, 0.5, -15.0), (3, 48000.0, 10000.0, 1.0, 12.0),
           (0, 44100.0, 22000.0, 0.3, 0.0), (1, 48000.0, 1.0, 10.0, 0.0)]


def cascade(S, seed=0, fs=48000.0):
    """S sections of a tone stack: high-pass, low shelf, peaks, high shelf, low-pass ..., the parameters varied with `seed`"""
    rng = np.random.default_rng(1000 + 31 * seed + S)
    plan = [(1, 60.0, 0.707), (2, 150.0, 0.8), (4, 500.0, 1.2), (3, 5000.0, 0.7), (0, 9000.0, 0.707), (4, 1800.0, 2.5), (4, 3200.0, 0.9), (4, 250.0, 3.0)]
    out = []
    for i in range(S):
        kind, f, q = plan[(i + seed) % len(plan)]
        out.append(design(kind, fs, f * float(rng.uniform(0.7, 1.4)), q * float(rng.uniform(0.8, 1.25)), float(rng.uniform(-9.0, 9.0))))
    return out


def noise(n, seed, gain=0.25):
    rng = np.random.default_rng(seed)
    return np.clip(gain * rng.standard_normal(n), -1.0, 1.0).astype(np.float32)


def ragged(total, sizes=CALL_SIZES):
    """call lengths from `sizes`, in turn, that add up to `total`"""
    calls, left, i = [], total, 0
    while left > 0:
        n = min(sizes[i % len(sizes)], left)
        calls.append(n)
        left -= n
        i += 1
    return calls


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
