"""Shared pieces of tests/test_compressor_cpu.py and tests/test_gpu_compressor.py: the compressor stage's contract
(include/neuralaudio_amd.h) restated in numpy float32, the closed form of NA_CompressorParamsFromDb in float64, the test curves, and the
runner that drives a batch with compressors beside its twin.

The contract is bit-exact, so everything that is compared is compared with np.array_equal: the expected row of a compressed stream is
fl(twin_row * g_ref) with g_ref computed from the twin's row -- the stage listens to the row it scales --, of any other stream the
twin's row.

A scenario is a list of call lengths and, per call index, the operations issued in front of that call:
  ("comp", stream, params or None, fadeSamples)  and the operations of tests/handover_cases.py ("park", "activate", ...)."""
import math

import numpy as np

import handover_cases as H

F = np.float32
POINTS = 513
FIRST_Q = 1648
STEP = ["x' = (x is NaN) ? 0 : min(|x|, 255.0f)",
        "c  = (x' > e) ? aA : aR",
        "d  = fl(x' - e);  e = fl(e + fl(c * d))",
        "b  = bits(e);  q = b >> 19",
        "curve(t): q < 1648 ? t[0]",
        ": i = min(q - 1648, 511);  f = fl((float)(b & 0x7FFFF) * 2^-19);",
        "fl(t[i] + fl(f * fl(t[i+1] - t[i])))",
        "g  = curve(tB)                                              where w == 1",
        "g  = fl(fl(fl(1 - w) * curve(tA)) + fl(w * curve(tB)))      else, w = OutStageWeightAt(N, k)",
        "y  = fl(x * g)"]


def knot_level(i):
    """the level of knot i, exact in float64 (and in float32)"""
    i = np.asarray(i)
    return np.ldexp(1.0 + (i & 15) / 16.0, -24 + (i >> 4))


LEVELS = knot_level(np.arange(POINTS))


def static_gain_db(level_db, threshold_db, ratio, knee_db):
    """G of the header, float64, on an array of levels in dB"""
    o = np.asarray(level_db, np.float64) - threshold_db
    s = (0.0 if math.isinf(ratio) else 1.0 / ratio) - 1.0
    W = float(knee_db)
    knee = s * (o + W / 2.0) ** 2 / (2.0 * W) if W > 0 else np.zeros_like(o)
    return np.where(2.0 * o < -W, 0.0, np.where((W > 0) & (2.0 * np.abs(o) <= W), knee, s * o))


def closed_form(level, threshold_db, ratio, knee_db, makeup_db):
    """the gain the header's formulas give at `level` (float64, not rounded)"""
    with np.errstate(divide="ignore"):
        L = 20.0 * np.log10(np.asarray(level, np.float64))
    return 10.0 ** ((static_gain_db(L, threshold_db, ratio, knee_db) + makeup_db) / 20.0)


def coeff(ms, rate):
    return F(1.0) if ms == 0 else F(1.0 - math.exp(-1.0 / (float(F(ms)) * rate / 1000.0)))


def params(attack=0.3, release=0.02, curve=None, **design):
    """a params dict: `curve` as given, or designed in float64 from threshold_db / ratio / knee_db / makeup_db (rounded once)"""
    if curve is None:
        d = dict(threshold_db=-60.0, ratio=4.0, knee_db=6.0, makeup_db=0.0)
        d.update(design)
        curve = closed_form(LEVELS, d["threshold_db"], d["ratio"], d["knee_db"], d["makeup_db"])
    return {"attackCoeff": float(F(attack)), "releaseCoeff": float(F(release)), "curve": np.asarray(curve, np.float64).astype(np.float32)}


def unity_curve():
    return np.ones(POINTS, np.float32)


def known_answer_curve():
    """1 below knot 384 (level 1.0), 0.25 from it on"""
    return np.where(np.arange(POINTS) < 384, 1.0, 0.25).astype(np.float32)


def weight(N, k):
    """OutStageWeightAt on an int64 array k, float32"""
    k = np.asarray(k, np.int64)
    w = ((k + 1).astype(np.float32) / F(N)).astype(np.float32) if N > 0 else np.ones(k.shape, np.float32)
    return np.where(k >= N - 1, F(1), w).astype(np.float32)


def level_of(x):
    """x' of the contract, float32 array"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), F(0), np.minimum(np.abs(x), F(255))).astype(np.float32)


def follow(aA, aR, e, xa):
    """the follower over the float32 array xa from state e: one float32 scalar operation per line of the contract; returns (levels, e)"""
    aA, aR, e = F(aA), F(aR), F(e)
    out = np.empty(len(xa), np.float32)
    for t, v in enumerate(xa):
        c = aA if v > e else aR
        d = F(v - e)
        e = F(e + F(c * d))
        out[t] = e
    return out, e


def curve_at(t, e):
    """curve(t) at the float32 array e: float32 array operations, one rounding each"""
    t = np.asarray(t, np.float32)
    b = np.asarray(e, np.float32).view(np.uint32)
    q = b >> 19
    i = np.minimum(np.maximum(q.astype(np.int64) - FIRST_Q, 0), 511)
    f = ((b & 0x7FFFF).astype(np.float32) * F(2.0 ** -19)).astype(np.float32)
    rise = (t[i + 1] - t[i]).astype(np.float32)
    part = (f * rise).astype(np.float32)
    return np.where(q < FIRST_Q, t[0], (t[i] + part).astype(np.float32)).astype(np.float32)


def mix(w, gA, gB):
    u = (F(1) - w).astype(np.float32)
    a = (u * gA).astype(np.float32)
    b = (w * gB).astype(np.float32)
    return np.where(w == F(1), gB, (a + b).astype(np.float32)).astype(np.float32)


class CompRef:
    """One stream's compressor: the header's step and the set call's rules.  run(x) returns the gains of len(x) more samples and keeps
    the follower's levels (self.levels) for the conditions on the inputs."""

    def __init__(self):
        self.e = F(0)
        self.aA = self.aR = F(1)
        self.tB, self.tA = None, None  # None: the unity curve
        self.N = self.k = 0
        self.fading = False
        self.has = False
        self.last_g = F(1)
        self.levels, self.took = [], set()

    def set(self, p, N):
        """the rules of NA_BatchSetStreamCompressor; returns False where the call is refused (a fade is running)"""
        if self.fading:
            return False
        if not self.has:
            if p is None:
                return True
            self.has, self.e, self.tB, self.tA = True, F(0), None, None
        if p is not None:
            self.aA, self.aR = F(p["attackCoeff"]), F(p["releaseCoeff"])
        new = None if p is None else np.asarray(p["curve"], np.float32).copy()
        if N == 0:
            self.tB = new
            if new is None:
                self._retire()
            return True
        self.tA, self.tB = self.tB, new
        self.fading, self.N, self.k = True, N, 0
        return True

    def _retire(self):
        self.has, self.fading, self.tA, self.tB, self.last_g = False, False, None, None, F(1)

    def remaining(self):
        return self.N - self.k if self.fading else 0

    def run(self, x):
        assert self.has
        x = np.asarray(x, np.float32)
        n = len(x)
        xa = level_of(x)
        e0 = self.e
        lev, self.e = follow(self.aA, self.aR, self.e, xa)
        prev = np.concatenate([[e0], lev[:-1]]).astype(np.float32)[:n]
        self.took |= set(np.unique(xa > prev).tolist())
        gB = curve_at(self.tB, lev) if self.tB is not None else np.ones(n, np.float32)
        g = gB
        if self.fading:
            w = weight(self.N, self.k + np.arange(n))
            gA = curve_at(self.tA, lev) if self.tA is not None else np.ones(n, np.float32)
            g = mix(w, gA, gB)
            self.k = min(self.N, self.k + n)
            if self.k >= self.N and n:
                self.fading, self.tA = False, None
        self.levels.append(lev)
        if n:
            self.last_g = g[-1]
            if not self.fading and self.tB is None:
                self._retire()
        return g.astype(np.float32)


def octaves_crossed(levels):
    q = np.concatenate(levels).view(np.uint32) >> 19
    q = q[q >= FIRST_Q]
    return 0 if len(q) == 0 else (int(q.max()) - int(q.min())) // 16


def assert_inputs_reach_every_case(ref, gains, what):
    """The conditions on a compressed row, on the restatement alone: both branches of c, samples with q < 1648 -- zero and subnormal
    levels among them --, at least three octaves of knots, g < 1 on at least a quarter of the samples."""
    lev, g = np.concatenate(ref.levels), np.concatenate(gains)
    assert ref.took == {True, False}, (what, "the follower took one branch of c only")
    q = lev.view(np.uint32) >> 19
    assert np.any(q < FIRST_Q) and np.any(lev == 0) and np.any((lev > 0) & (lev < F(2.0 ** -126))), (what, "no level below knot 0 / zero / subnormal")
    assert octaves_crossed(ref.levels) >= 3, (what, "octaves of knots", octaves_crossed(ref.levels))
    assert np.count_nonzero(g < 1) * 4 >= len(g), (what, "g < 1 on", int(np.count_nonzero(g < 1)), "of", len(g))


# ---- the batch under test and its twin (the twelve rows of handover_cases) ----

def drive(batch, op, stage):
    if op[0] == "comp":
        if stage:
            batch.SetStreamCompressor(op[1], op[2], op[3])
    else:
        H.drive(batch, op, False)  # (park / activate: the same on both batches)


class Contract:
    """per row: a CompRef; who is parked"""

    def __init__(self, rows=H.ROWS, live=H.LIVE):
        self.rows = rows
        self.comp = {s: CompRef() for s in range(rows)}
        self.parked = set(range(rows)) - set(live)
        self.gains = {s: [] for s in range(rows)}

    def apply(self, op):
        if op[0] == "comp":
            assert self.comp[op[1]].set(op[2], op[3]), ("the scenario sets during a fade", op[1])
        elif op[0] == "park":
            self.comp[op[1]] = CompRef()
            self.parked.add(op[1])
        elif op[0] == "activate":
            self.parked.discard(op[1])
        else:
            raise KeyError(op)

    def entries(self):
        return sum(1 for r in self.comp.values() if r.has)

    def step(self, yt):
        """yt: the twin's rows of this call.  Returns the expected rows."""
        e = yt.copy()
        for s in range(self.rows):
            ref = self.comp[s]
            if s in self.parked:
                e[s] = 0.0
            elif ref.has:
                g = ref.run(yt[s])
                self.gains[s].append(g)
                e[s] = (yt[s] * g).astype(np.float32)  # one f32 multiplication per sample
        return e


def make_batch(na, models, stage, resample=None, before=None):
    """the twelve rows; `before(batch)` sets up what twin and batch under test share (other stages); stage: the compressor stage"""
    b = H.make_batch(na, models, stage=False, resample=resample)
    if before:
        before(b)
    if stage:
        b.EnableCompressorStage()
    return b


def run_scenario(na, models, x, calls, ops, path="process", resample=None, hook=None, before=None, check=None):
    """The batch under test through `path` against its twin and the contract: every row of every call, bit for bit.  check(contract)
    runs on the restatement alone, before the batch under test exists; hook(batch, contract, i) runs after call i.  Returns (rows
    [ROWS, total], the twin's rows, the contract)."""
    twin = make_batch(na, models, stage=False, resample=resample, before=before)
    yts, pos = [], 0
    for i, n in enumerate(calls):
        for op in ops.get(i, ()):
            drive(twin, op, False)
        yts.append(twin.Process(np.ascontiguousarray(x[:, pos:pos + n])))
        pos += n
    twin.close()
    contract, expected = Contract(), []
    for i, n in enumerate(calls):
        for op in ops.get(i, ()):
            contract.apply(op)
        expected.append((contract.step(yts[i]), contract.entries(), {s: (r.last_g, r.remaining(), r.has and r.tB is not None) for s, r in contract.comp.items()}))
    if check:
        check(contract)
    b = make_batch(na, models, stage=True, resample=resample, before=before)
    runner = H.Runner(na, b, path)
    got, pos = [], 0
    try:
        for i, n in enumerate(calls):
            for op in ops.get(i, ()):
                drive(b, op, True)
            y = runner.call(x[:, pos:pos + n])
            e = expected[i][0]
            for s in range(y.shape[0]):
                assert np.array_equal(y[s], e[s]), (path, "call", i, "n", n, "row", s, int(np.count_nonzero(y[s] != e[s])), "samples differ, first at",
                                                    int(np.flatnonzero(y[s] != e[s])[0]))
            got.append(y)
            pos += n
            if hook:
                hook(b, expected[i], i)
    finally:
        runner.close()
        b.close()
    return np.concatenate(got, axis=1), np.concatenate(yts, axis=1), contract
