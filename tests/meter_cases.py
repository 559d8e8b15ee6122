"""Shared pieces of tests/test_meter_cpu.py and tests/test_gpu_meter.py: the meter stage's contract (include/neuralaudio_amd.h) restated
in numpy -- uint64 sums, float32 values, maxima and minima on the bit patterns --, the special inputs, and the runner that drives a
batch with meters beside its twin.

Every quantity of the contract is a max, a min or an integer sum, so everything that is compared is compared for equality: a reading is
a dict of integers and float32 bit patterns (`norm`), and the expected one is the reference's reading for the window index the batch
reports.

A scenario is a list of call lengths and, per call index, the operations issued in front of that call:
  ("meter", stream, params)  ("unmeter", stream)  and the operations of tests/gate_cases.py ("gate", "ungate", "park", "activate")."""
import numpy as np

import gate_cases as G
import handover_cases as H

F = np.float32
FIELDS = ("windowSamples", "clipLevelIn", "clipLevelOut")
TAP = ("energy", "oversTotal", "peak", "peakHold", "overs")
CONTRACT = ["x' = (x is NaN) ? 0 : min(|x|, 1e18f)",
            "q  = (unsigned) trunc(min(x', 8.0f) * 2^21)     (the product is exact; q <= 2^24)",
            "peak   = max(peak, x')        over the window      (exact; subnormals kept)",
            "energy = energy + q * q       over the window, unsigned 64-bit    (<= 2^63 for W <= 32768)",
            "overs  = overs + (x' >= clipLevel ? 1 : 0)   over the window",
            "peakHold   = max over every sample since the meter was set",
            "oversTotal = overs summed over every sample since the meter was set (64-bit)",
            "gateGainMin  = min(g) over the window",
            "gateGainLast = g of the window's last sample"]
STRUCTS = ["typedef struct NA_MeterParams  { int windowSamples; float clipLevelIn, clipLevelOut; } NA_MeterParams;",
           "typedef struct NA_MeterTap     { unsigned long long energy, oversTotal; float peak, peakHold; unsigned int overs, reserved; } NA_MeterTap;",
           "typedef struct NA_MeterReading { unsigned long long windows; NA_MeterTap in, out; float gateGainMin, gateGainLast; int windowSamples, reserved; } NA_MeterReading;",
           "typedef struct NA_MeterInfo    { int numMeters; long long deviceBytes; } NA_MeterInfo;"]


def params(window=48, clip_in=0.5, clip_out=0.5):
    return dict(windowSamples=int(window), clipLevelIn=float(F(clip_in)), clipLevelOut=float(F(clip_out)))


def bits(v):
    return int(np.asarray(v, np.float32).reshape(1).view(np.uint32)[0])


def special_inputs(clip):
    """NaN, +-inf, 1e30, -0.0, subnormals, k * 2^-21 and its two f32 neighbours, a sample exactly at `clip` and its two neighbours"""
    c = F(clip)
    out = [np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0, 0.0, 1e-45, -3e-42, 1.1754942e-38]
    for k in (1, 3, 77777, 1 << 20, (1 << 23) + 5):
        v = F(k * 2.0 ** -21)
        out += [np.nextafter(v, F(0)), v, -np.nextafter(v, F(9))]
    out += [np.nextafter(c, F(0)), -c, np.nextafter(c, F(9)), 7.9999995, 8.0, -8.000001, 100.0]
    return np.array(out, np.float32)


class TapRef:
    """One tap of one meter.  feed(x) takes more samples; self.readings[k] is the reading of window k."""

    def __init__(self, window, clip):
        self.W, self.clip = int(window), F(clip)
        self.pending = np.zeros(0, np.float32)
        self.hold, self.total = np.uint32(0), 0
        self.readings = []

    def feed(self, x):
        self.pending = np.concatenate([self.pending, np.asarray(x, np.float32)])
        while len(self.pending) >= self.W:
            w, self.pending = self.pending[:self.W], self.pending[self.W:]
            b = w.view(np.uint32) & np.uint32(0x7FFFFFFF)
            xa = b.view(np.float32).copy()
            xa[np.isnan(xa)] = 0.0                               # x' = (x is NaN) ? 0 : min(|x|, 1e18f)
            xa = np.minimum(xa, F(1e18))
            q = np.trunc(np.minimum(xa, F(8.0)) * F(2.0 ** 21))  # float32 product: exact
            assert q.dtype == np.float32 and np.all(q <= 2.0 ** 24)
            q = q.astype(np.uint64)
            energy = int(np.sum(q * q, dtype=np.uint64))
            peak = np.max(xa.view(np.uint32))                    # for non-negative floats the max of the bit patterns is the max
            overs = int(np.count_nonzero(xa >= self.clip))
            self.hold = max(self.hold, peak)
            self.total += overs
            self.readings.append(dict(energy=energy, oversTotal=self.total, peak=int(peak), peakHold=int(self.hold), overs=overs))


class MeterRef:
    """One stream's meter: feed(x, y, g) takes a call's input row, the row the caller receives and the gate's gains (None: not gated
    in this call).  reading(k): the reading of window k in the normal form of `norm`."""

    def __init__(self, p):
        self.p = dict(p)
        self.W = int(p["windowSamples"])
        self.tin, self.tout = TapRef(self.W, p["clipLevelIn"]), TapRef(self.W, p["clipLevelOut"])
        self.g = np.zeros(0, np.float32)
        self.position = 0

    def feed(self, x, y, g=None):
        self.tin.feed(x)
        self.tout.feed(y)
        self.g = np.concatenate([self.g, np.ones(len(x), np.float32) if g is None else np.asarray(g, np.float32)])
        self.position += len(x)

    @property
    def windows(self):
        return self.position // self.W

    def reading(self, k):
        g = self.g[k * self.W:(k + 1) * self.W]
        return {"windows": k + 1, "in": self.tin.readings[k], "out": self.tout.readings[k], "gateGainMin": bits(np.min(g)), "gateGainLast": bits(g[-1]),
                "windowSamples": self.W}

    def latest(self):
        return self.reading(self.windows - 1) if self.windows > 0 else None


def norm(r):
    """a ReadStreamMeter dict with its floats as bit patterns (None stays None)"""
    if r is None:
        return None
    tap = lambda t: dict(energy=t["energy"], oversTotal=t["oversTotal"], peak=bits(t["peak"]), peakHold=bits(t["peakHold"]), overs=t["overs"])
    return {"windows": r["windows"], "in": tap(r["in"]), "out": tap(r["out"]), "gateGainMin": bits(r["gateGainMin"]), "gateGainLast": bits(r["gateGainLast"]),
            "windowSamples": r["windowSamples"]}


def rms(tap, window):
    """the header's recipe: sqrt(energy / W) / 2^21"""
    return float(np.sqrt(tap["energy"] / window) / 2.0 ** 21)


# ---- the batch under test and its twin (the twelve rows of handover_cases) ----

def make_batch(na, models, meter, gate=False, resample=None):
    b = H.make_batch(na, models, stage=False, resample=resample)
    if gate:
        b.EnableGateStage()
    if meter:
        b.EnableMeterStage()
    return b


def drive(batch, op, meter):
    if op[0] == "meter":
        if meter:
            batch.SetStreamMeter(op[1], op[2])
    elif op[0] == "unmeter":
        if meter:
            batch.SetStreamMeter(op[1], None)
    else:
        G.drive(batch, op, True)  # (gates, parks and activations: the same on both batches)


class Contract:
    """per row: a MeterRef or None, and the gate's reference where the row is gated"""

    def __init__(self, rows=H.ROWS):
        self.rows = rows
        self.meter = {s: None for s in range(rows)}
        self.gates = G.Contract(rows)

    def apply(self, op):
        if op[0] == "meter":
            self.meter[op[1]] = MeterRef(op[2])
        elif op[0] == "unmeter":
            self.meter[op[1]] = None
        else:
            if op[0] == "park":
                self.meter[op[1]] = None
            self.gates.apply(op)

    def step(self, x, y):
        """x: this call's input rows; y: the rows the caller receives (the twin's)"""
        gated = {s: ref for s, ref in self.gates.gate.items() if ref is not None and s not in self.gates.parked}
        before = {s: len(self.gates.gains[s]) for s in gated}
        self.gates.step(x, y)  # (moves the gate references on; the twin has applied its gates itself)
        for s, ref in self.meter.items():
            if ref is not None:
                ref.feed(x[s], y[s], self.gates.gains[s][before[s]] if s in gated else None)


def run_scenario(na, models, x, calls, ops, path="process", resample=None, hook=None, gate=False, sync=True):
    """The batch under test through `path` beside its twin -- the same batch without the meter stage: every row of every call must be
    the twin's, bit for bit, and after every call (sync: behind a synchronise) every metered row's reading the reference's newest.
    hook(batch, contract, i) runs after call i.  Returns (rows, the twin's rows, the contract, the readings after the last call)."""
    twin = make_batch(na, models, meter=False, gate=gate, resample=resample)
    yts, pos = [], 0
    for i, n in enumerate(calls):
        for op in ops.get(i, ()):
            drive(twin, op, False)
        yts.append(twin.Process(np.ascontiguousarray(x[:, pos:pos + n])))
        pos += n
    twin.close()
    b = make_batch(na, models, meter=True, gate=gate, resample=resample)
    runner, contract = H.Runner(na, b, path), Contract()
    got, pos, last = [], 0, {}
    try:
        for i, n in enumerate(calls):
            for op in ops.get(i, ()):
                drive(b, op, True)
                contract.apply(op)
            xs = x[:, pos:pos + n]
            y = runner.call(xs)
            for s in range(y.shape[0]):
                assert np.array_equal(y[s], yts[i][s]), (path, "call", i, "n", n, "row", s, "differs from the twin")
            contract.step(xs, yts[i])
            if sync:
                b.Synchronize()
                for s, ref in contract.meter.items():
                    if ref is not None:
                        last[s] = norm(b.ReadStreamMeter(s))
                        assert last[s] == ref.latest(), (path, "call", i, "n", n, "row", s, last[s], ref.latest())
            got.append(y)
            pos += n
            if hook:
                hook(b, contract, i)
    finally:
        runner.close()
        b.close()
    return np.concatenate(got, axis=1), np.concatenate(yts, axis=1), contract, last
