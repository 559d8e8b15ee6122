"""Shared pieces of tests/test_gate_cpu.py and tests/test_gpu_gate.py: the gate stage's contract (include/neuralaudio_amd.h) restated
in numpy float32 scalars, one sample at a time, the test signal, and the runner that drives a batch with gates beside its twin.

The contract is bit-exact, so everything that is compared is compared with np.array_equal: the expected row of a gated stream is
fl(twin_row * g_ref), of any other stream the twin's row.

A scenario is a list of call lengths and, per call index, the operations issued in front of that call:
  ("gate", stream, params, startOpen)  ("ungate", stream)  and the operations of tests/handover_cases.py ("park", "activate", ...)."""
import numpy as np

import handover_cases as H

F = np.float32
U = 1 << 30
FIELDS = ("openPower", "closePower", "floorGain", "detectorCoeff", "attackSamples", "holdSamples", "releaseSamples")
BASE = dict(openPower=1e-3, closePower=2.5e-4, floorGain=0.0, detectorCoeff=0.05, attackSamples=32, holdSamples=50, releaseSamples=64)
# each variation changes one constant
VARIATIONS = {"floor0": {}, "floor0.1": dict(floorGain=0.1), "hold0": dict(holdSamples=0), "attack1": dict(attackSamples=1)}
BURSTS = [300, 40, 500, 120, 700, 64]  # noise at 0.25 ...
GAPS = [700, 130, 300, 180, 40, 250]   # ... and stretches at 1e-4 behind each, all of different lengths from 40 to 700
TOTAL = sum(BURSTS) + sum(GAPS)


def params(**changes):
    p = dict(BASE)
    p.update(changes)
    return p


def variation(name):
    return params(**VARIATIONS[name])


def gate_signal(seed, total=TOTAL, lead=0):
    """noise bursts at 0.25 alternating with stretches at 1e-4; `lead` samples of the quiet level in front"""
    rng = np.random.default_rng(7000 + seed)
    level = np.full(total + sum(BURSTS) + sum(GAPS), 1e-4)
    pos = lead
    while pos < total:
        for b, g in zip(BURSTS, GAPS):
            level[pos:pos + b] = 0.25
            pos += b + g
    return np.clip(level[:total] * rng.standard_normal(total), -1.0, 1.0).astype(np.float32)


class GateRef:
    """One stream's gate: the header's step in float32 scalars.  run(x) returns the gains of len(x) more samples and keeps, per sample,
    the state behind it (self.trace: p, hold, open, u) and the events the coverage conditions ask for."""

    def __init__(self, p, start_open=True):
        self._consts(p)
        self.p, self.hold, self.open, self.u = F(0), (self.H if start_open else 0), (1 if start_open else 0), (U if start_open else 0)
        self.force_open, self.left = False, 0
        self.retired = False
        self.trace, self.ran_out, self.rearmed = [], 0, 0
        self.last_g = F(1) if start_open else self.floor

    def _consts(self, p):
        self.params = dict(p)
        self.a, self.Po, self.Pc, self.floor = F(p["detectorCoeff"]), F(p["openPower"]), F(p["closePower"]), F(p["floorGain"])
        self.span = F(F(1) - self.floor)
        self.H, self.A, self.R = int(p["holdSamples"]), int(p["attackSamples"]), int(p["releaseSamples"])
        self.step_up, self.step_down = -(-U // self.A), -(-U // self.R)

    def set(self, p):
        """new constants on the kept state (also during the tail of a removal: the gate is re-armed)"""
        self._consts(p)
        self.hold = min(self.hold, self.H)
        self.force_open, self.left = False, 0

    def remove(self):
        if not self.force_open:
            self.force_open, self.left = True, self.A

    def gain_of(self, u):
        if u == U:
            return F(1)
        pos = F(F(u) * F(2.0 ** -30))  # F(int) rounds to nearest even
        return F(self.floor + F(self.span * pos))

    def step(self, x):
        x = F(x)
        xa = F(0) if np.isnan(x) else min(F(abs(x)), F(1e18))
        s = F(xa * xa)
        d = F(s - self.p)
        self.p = F(self.p + F(self.a * d))
        if self.p >= self.Po:
            if self.open and self.hold < self.H:
                self.rearmed += 1
            self.open, self.hold = 1, self.H
        elif self.p < self.Pc:
            if self.hold > 0:
                self.hold -= 1
            else:
                if self.open:
                    self.ran_out += 1
                self.open = 0
        if self.force_open:
            self.open = 1
        self.u = min(U, self.u + self.step_up) if self.open else (self.u - self.step_down if self.u > self.step_down else 0)
        g = self.gain_of(self.u)
        self.trace.append((self.p, self.hold, self.open, self.u))
        self.last_g = g
        return g

    def run(self, x):
        """len(x) samples of one call; a removal that has produced its attackSamples samples retires behind the call (host rule)"""
        assert not self.retired
        g = np.array([self.step(v) for v in x], np.float32)
        if self.force_open:
            self.left -= min(self.left, len(x))
            if self.left == 0 and len(x) > 0:
                assert self.u == U, "a removal ends at u == U by construction"
                self.retired = True
        return g


def coverage(ref, g):
    """what the gain sequence g of reference `ref` contains, by name"""
    floor = ref.floor
    partial = (g != F(1)) & (g != floor) if floor != F(1) else np.zeros(len(g), bool)
    rising = bool(np.any(partial[1:] & (g[1:] > g[:-1])))
    falling = bool(np.any(partial[1:] & (g[1:] < g[:-1])))
    return {"open": bool(np.any(g == F(1))), "floor": bool(np.any(g == floor)), "rising": rising, "falling": falling,
            "ran_out": ref.ran_out > 0, "rearmed": ref.rearmed > 0,
            "jump_open": bool(np.any((g[1:] == F(1)) & (g[:-1] < F(1)))), "reopened_falling": _reopened_falling(g)}


def _reopened_falling(g):
    d = np.sign(np.diff(g.astype(np.float64)))
    d = d[d != 0]
    return bool(np.any((d[:-1] < 0) & (d[1:] > 0)))


def required(p):
    """The conditions on the inputs: every gated row's reference gains contain g == 1, g == floor, a rising partial value, a falling
    partial value, a hold that ran out and a hold that was re-armed before running out.  Two of them cannot happen for one variation
    each, whatever the signal: with attackSamples = 1 the gain position goes from any value to U in one sample, so no rising value
    lies strictly between floor and 1 -- that row must show the one-sample jump to 1 instead; with holdSamples = 0 there is no count to
    re-arm -- that row must instead show a gate that closed partly and opened again (a falling ramp turned round)."""
    names = ["open", "floor", "rising", "falling", "ran_out", "rearmed"]
    if p["attackSamples"] == 1:
        names[names.index("rising")] = "jump_open"
    if p["holdSamples"] == 0:
        names[names.index("rearmed")] = "reopened_falling"
    return names


def assert_covered(ref, g, what):
    have = coverage(ref, g)
    for name in required(ref.params):
        assert have[name], (what, "the reference's gains lack", name, have)


# ---- the batch under test and its twin (the twelve rows of handover_cases) ----

def drive(batch, op, stage):
    if op[0] == "gate":
        if stage:
            batch.SetStreamGate(op[1], op[2], op[3])
    elif op[0] == "ungate":
        if stage:
            batch.SetStreamGate(op[1], None)
    else:
        H.drive(batch, op, False)  # (park / activate: the same on both batches)


class Contract:
    """per row: a GateRef or None; who is parked"""

    def __init__(self, rows=H.ROWS, live=H.LIVE):
        self.rows = rows
        self.gate = {s: None for s in range(rows)}
        self.parked = set(range(rows)) - set(live)
        self.gains = {s: [] for s in range(rows)}

    def apply(self, op):
        if op[0] == "gate":
            _, s, p, start_open = op
            if self.gate[s] is None:
                self.gate[s] = GateRef(p, start_open)
            else:
                self.gate[s].set(p)
        elif op[0] == "ungate":
            if self.gate[op[1]] is not None:
                self.gate[op[1]].remove()
        elif op[0] == "park":
            self.gate[op[1]] = None
            self.parked.add(op[1])
        elif op[0] == "activate":
            self.parked.discard(op[1])
        else:
            raise KeyError(op)

    def step(self, x, yt):
        """x: this call's input rows, yt: the twin's rows.  Returns the expected rows."""
        e = yt.copy()
        for s in range(self.rows):
            ref = self.gate[s]
            if s in self.parked:
                e[s] = 0.0
            elif ref is not None:
                g = ref.run(x[s])
                self.gains[s].append(g)
                e[s] = (yt[s] * g).astype(np.float32)  # one f32 multiplication per sample
                if ref.retired:
                    self.gate[s] = None
        return e


def make_batch(na, models, stage, resample=None, hip_stream=None):
    b = H.make_batch(na, models, stage=False, resample=resample, hip_stream=hip_stream)
    if stage:
        b.EnableGateStage()
    return b


def run_scenario(na, models, x, calls, ops, path="process", resample=None, hook=None):
    """The batch under test through `path` against its twin and the contract: every row of every call, bit for bit.  hook(batch,
    contract, i) runs after call i.  Returns (rows [ROWS, total], the twin's rows, the contract)."""
    twin = make_batch(na, models, stage=False, resample=resample)
    yts, pos = [], 0
    for i, n in enumerate(calls):
        for op in ops.get(i, ()):
            drive(twin, op, False)
        yts.append(twin.Process(np.ascontiguousarray(x[:, pos:pos + n])))
        pos += n
    twin.close()
    b = make_batch(na, models, stage=True, resample=resample)
    runner, contract = H.Runner(na, b, path), Contract()
    got, pos = [], 0
    try:
        for i, n in enumerate(calls):
            for op in ops.get(i, ()):
                drive(b, op, True)
                contract.apply(op)
            xs = x[:, pos:pos + n]
            y = runner.call(xs)
            e = contract.step(xs, yts[i])
            for s in range(y.shape[0]):
                assert np.array_equal(y[s], e[s]), (path, "call", i, "n", n, "row", s, int(np.count_nonzero(y[s] != e[s])), "samples differ, first at",
                                                    int(np.flatnonzero(y[s] != e[s])[0]))
            got.append(y)
            pos += n
            if hook:
                hook(b, contract, i)
    finally:
        runner.close()
        b.close()
    return np.concatenate(got, axis=1), np.concatenate(yts, axis=1), contract
