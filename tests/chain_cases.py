"""Shared pieces of tests/test_chain_cases_cpu.py and tests/test_gpu_chain.py: the whole per-stream stage chain of a batch, checked
rung by rung.

The chain, as GpuBatch::StageId states it: gate, EQ, cabinet, compressor, modulation, delay, reverb, output gain, mix, then the meter's
and the tuner's taps.  Two of the audio stages are not bit-exact by contract (cabinet: cabinet_cases.conv_bound; output stage:
handover_cases.REL / ABS), so a pure composition of the restatements would drift away behind them.  The LADDER avoids that: rung k is a
batch with the first k audio stages enabled, every rung gets the same input and the same operations, and stage k's own restatement is
evaluated on rung k-1's GPU rows of the same call -- with that stage's own criterion and nothing looser.  The top rung adds meter and
tuner, which write no audio.

Nothing here restates arithmetic: every adaptor (class ...Rung) wraps the contract class of its stage's own *_cases.py behind
apply(op) / leave(row) / step(x, rows_below).  Chain holds one adaptor per stage and who is parked; Chain.compose runs them as a pure
composition (what the CPU file does on stand-in rows), the GPU file calls Chain.step_stage with the rows of the rung below.

Operations, per call index, issued in front of that call:
  ("gate", s, params, startOpen)  ("ungate", s)  ("eq", s, sections, N)  ("ir", s, name or None, N)  ("comp", s, params or None, N)
  ("mod", s, params or None, N)  ("delay", s, params or None, N)  ("reverb", s, name or None, wet, dry, N)  ("gain", s, gain, R)
  ("handover", from, to, N)  ("mix", streams, gains, taps, R)  ("meter", s, params)  ("tuner", s, params)  ("park", s)  ("activate", s)
and ("park", s, True): the MIRRORED park -- the park of `from` that the output stage performs by itself at the top of the call behind
a fade's last sample.  Rungs without the output stage are told to park explicitly, at the same call, so every rung has the same live
set and the same entries (with_mirrored_parks)."""
import numpy as np

import cabinet_cases as CB
import compressor_cases as CK
import delay_cases as D
import eq_cases as E
import gate_cases as G
import handover_cases as H
import meter_cases as MT
import mix_cases as MX
import mod_cases as K
import reverb_cases as R
import tuner_cases as T

F = np.float32
AUDIO = ("gate", "eq", "cabinet", "compressor", "mod", "delay", "reverb", "output", "mix")  # StageId order
TAPS = ("meter", "tuner")
OUT = AUDIO.index("output")
TOP = len(AUDIO) + len(TAPS)                     # the rung with every stage
RUNGS = list(range(len(AUDIO) + 1)) + [TOP]      # rung k: the first k stages of the chain
STAGE_OF = {"gate": 0, "ungate": 0, "eq": 1, "ir": 2, "comp": 3, "mod": 4, "delay": 5, "reverb": 6, "gain": 7, "handover": 7, "mix": 8,
            "meter": 9, "tuner": 10}
CAB_TAPS, MOD_DELAY, DELAY_MAX, REV_TAPS = 512, 512, 300, 2048  # what the Enable calls are given
RING = 4096  # the delay and modulation rings of these maxima: the smallest power of two >= maximum + a piece of 2048


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


class Expect:
    """What a stage makes of a call: e [rows, n], the rows it rewrote (`touched`: the others keep the bits below) and, for the two
    stages with a bound, limit [rows, n] (None: the rows are compared on the bits)."""

    def __init__(self, e, touched, limit=None):
        self.e, self.touched, self.limit = e, set(touched), limit

    def rows(self):
        with np.errstate(over="ignore"):
            return np.ascontiguousarray(self.e, F)


# ---- one adaptor per stage: apply(op), leave(row), step(x, rows_below), entries() ----

class GateRung:
    name, kinds = "gate", ("gate", "ungate")

    def __init__(self, rows, **_):
        self.c = G.Contract(rows, live=range(rows))
        self.refs, self.last = {}, {}

    def apply(self, op):
        self.c.apply(op)
        if op[0] == "gate":
            self.refs[op[1]] = self.c.gate[op[1]]

    def leave(self, row):
        self.c.gate[row] = None

    def entries(self):
        return {s for s, ref in self.c.gate.items() if ref is not None}

    def step(self, x, below):
        touched = self.entries()
        before = {s: len(self.c.gains[s]) for s in touched}
        e = self.c.step(x, below)
        self.last = {s: self.c.gains[s][before[s]] for s in touched}  # this call's gains: what the meter's GATE reading follows
        return Expect(e, touched)


class EqRung:
    name, kinds = "eq", ("eq",)

    def __init__(self, rows, **_):
        self.refs = {s: E.EqRef() for s in range(rows)}

    def apply(self, op):
        self.refs[op[1]].set(op[2], op[3])

    def leave(self, row):
        self.refs[row].leave()

    def entries(self):
        return {s for s, ref in self.refs.items() if ref.is_entry}

    def step(self, x, below):
        touched, e = self.entries(), below.copy()
        for s in touched:
            e[s] = self.refs[s].run(below[s])
        return Expect(e, touched)


class CabRung:
    name, kinds = "cabinet", ("ir",)

    def __init__(self, rows, irs=None, **_):
        self.c = CB.CabContract(rows, irs or {})

    def apply(self, op):
        self.c.set_ir(op[1], op[2], op[3])

    def leave(self, row):
        self.c.leave(row)

    def entries(self):
        return {s for s, st in self.c.state.items() if st is not None}

    def step(self, x, below):
        touched = self.entries()
        e, bound, exact = self.c.step(below)
        assert touched == {s for s in range(len(exact)) if not exact[s]}
        return Expect(e, touched, bound)


class CompRung:
    name, kinds = "compressor", ("comp",)

    def __init__(self, rows, **_):
        self.refs = {s: CK.CompRef() for s in range(rows)}
        self.gains = {s: [] for s in range(rows)}
        self.left = []  # (row, ref, gains) of the entries that parked

    def apply(self, op):
        assert self.refs[op[1]].set(op[2], op[3]), ("the scenario sets during a fade", op)

    def leave(self, row):
        if self.refs[row].has:
            self.left.append((row, self.refs[row], self.gains[row]))
        self.refs[row], self.gains[row] = CK.CompRef(), []

    def entries(self):
        return {s for s, ref in self.refs.items() if ref.has}

    def step(self, x, below):
        touched, e = self.entries(), below.copy()
        for s in touched:
            g = self.refs[s].run(below[s])
            self.gains[s].append(g)
            e[s] = (below[s] * g).astype(F)  # one f32 multiplication per sample
        return Expect(e, touched)


class _LineRung:
    """modulation and delay: a reference per row and the samples each entry has produced since its T0 (its ring position)"""

    def __init__(self, rows, **_):
        self.refs = {s: self.Ref() for s in range(rows)}
        self.age = {s: 0 for s in range(rows)}
        self.oldest = 0

    def leave(self, row):
        self.refs[row].leave()

    def step(self, x, below):
        touched, e = self.entries(), below.copy()
        for s in touched:
            e[s] = self.run(self.refs[s], below[s])
            self.age[s] += below.shape[1]
            self.oldest = max(self.oldest, self.age[s])
        for s in set(self.refs) - self.entries():
            self.age[s] = 0
        return Expect(e, touched)


class ModRung(_LineRung):
    name, kinds, Ref = "mod", ("mod",), K.ModRef

    def apply(self, op):
        assert self.refs[op[1]].set(op[2], op[3]) is True, ("the scenario's set call is refused", op)

    def entries(self):
        return {s for s, ref in self.refs.items() if ref.has}

    def run(self, ref, row):
        return ref.run(row)


class DelayRung(_LineRung):
    name, kinds, Ref = "delay", ("delay",), D.DelayRef

    def apply(self, op):
        self.refs[op[1]].set(op[2], op[3])

    def entries(self):
        return {s for s, ref in self.refs.items() if ref.on}

    def run(self, ref, row):
        return ref.process(row)


class RevRung:
    name, kinds = "reverb", ("reverb",)

    def __init__(self, rows, rev_irs=None, tw=None, **_):
        self.c = R.RevContract(rows, rev_irs or {}, tw)

    def apply(self, op):
        self.c.set(op[1], op[2], op[3], op[4], op[5])

    def leave(self, row):
        self.c.leave(row)

    def entries(self):
        return {s for s, st in self.c.state.items() if st is not None}

    def step(self, x, below):
        touched = self.entries()
        e, exact = self.c.step(below)
        assert touched == {s for s in range(len(exact)) if not exact[s]}
        return Expect(e, touched)


class OutRung:
    name, kinds = "output", ("gain", "handover", "activate")

    def __init__(self, rows, live=H.LIVE, **_):
        self.c = H.Contract(rows, live)

    def apply(self, op):
        assert op[0] != "handover" or op[3] > 0, "the ladder's hand-overs fade"
        self.c.apply(op)

    def leave(self, row):
        self.c.apply(("park", row))

    def finished(self):
        """the rows the stage parks by itself at the top of the next call"""
        return list(self.c.finished)

    def entries(self):
        c = self.c
        return {s for s, r in c.ramp.items() if r["b"] != 1.0 or r["k"] < r["R"]} | {s for fd in c.fades for s in (fd["f"], fd["t"])}

    def step(self, x, below):
        assert not self.c.finished, "the chain mirrors the stage's own parks in front of the call"
        e, bound, exact = self.c.step(below)
        return Expect(e, {s for s in range(len(exact)) if not exact[s]}, H.REL * bound + H.ABS)


class MixRung:
    name, kinds = "mix", ("mix",)

    def __init__(self, rows, **_):
        self.refs = []

    def apply(self, op):
        _, streams, gains, taps, ramp = op
        for ref in self.refs:
            if ref.streams == list(streams):  # the member list of an existing group: a gain change from the gains reached
                ref.set(gains, ramp)
                return
        assert not any(set(ref.streams) & set(streams) for ref in self.refs), "a stream belongs to one group"
        self.refs.append(MX.MixRef(streams, gains, taps=taps, R=ramp))

    def leave(self, row):
        self.refs = [ref for ref in self.refs if row not in ref.streams]  # the group that names it goes at once

    def entries(self):
        """the rows the stage rewrites"""
        return {s for ref in self.refs for s in ref.streams[:ref.D]}

    def members(self):
        return {s for ref in self.refs for s in ref.streams}

    def step(self, x, below):
        return Expect(MX.run_groups(self.refs, below, x), self.entries())


RUNG_CLASSES = {c.name: c for c in (GateRung, EqRung, CabRung, CompRung, ModRung, DelayRung, RevRung, OutRung, MixRung)}


class Chain:
    """One adaptor per audio stage in `order`, the meter and tuner references, and who is parked."""

    def __init__(self, irs, rev_irs, tw, order=AUDIO, rows=H.ROWS, live=H.LIVE):
        self.rows = rows
        self.stages = [RUNG_CLASSES[name](rows, irs=irs, rev_irs=rev_irs, tw=tw, live=live) for name in order]
        self.by_name = {st.name: st for st in self.stages}
        self.parked = set(range(rows)) - set(live)
        self.meters, self.tuners = {}, {}
        self.had = {st.name: set() for st in self.stages}      # (per stage) the rows that ever had an entry in a call ...
        self.changed = {st.name: set() for st in self.stages}  # ... and those whose bits its restatement changed

    def apply(self, op):
        kind = op[0]
        if kind == "park":
            for st in self.stages:
                st.leave(op[1])
            self.meters.pop(op[1], None)
            self.tuners.pop(op[1], None)
            self.parked.add(op[1])
            return
        if kind == "meter":
            self.meters[op[1]] = MT.MeterRef(op[2])
            return
        if kind == "tuner":
            self.tuners[op[1]] = T.TunerRef(op[2])
            return
        if kind in ("activate", "handover"):
            self.parked.discard(op[2] if kind == "handover" else op[1])
        for st in self.stages:
            if kind in st.kinds:
                st.apply(op)

    def mirrored(self):
        out = self.by_name.get("output")
        return [("park", f, True) for f in out.finished()] if out else []

    def step_stage(self, name, x, below):
        """stage `name` on the rows below it; parked rows are silence whatever the stage says"""
        st = self.by_name[name]
        below = np.ascontiguousarray(below, F)
        exp = st.step(np.ascontiguousarray(x, F), below)
        exp.touched -= self.parked
        for s in exp.touched:
            self.had[name].add(s)
            if not same_bits(exp.rows()[s], below[s]):
                self.changed[name].add(s)
        return exp

    def compose(self, x, rows0):
        """the pure composition of the restatements on rows0 (the rows in front of the chain), in the chain's order"""
        rows = np.ascontiguousarray(rows0, F).copy()
        rows[sorted(self.parked)] = 0.0
        for st in self.stages:
            rows = self.step_stage(st.name, x, rows).rows()
            rows[sorted(self.parked)] = 0.0
        return rows

    def taps(self, x, y):
        """the meter's and the tuner's references take the call: x the input rows, y the rows the caller receives"""
        gate = self.by_name.get("gate")
        for s, ref in self.meters.items():
            ref.feed(x[s], y[s], gate.last.get(s) if gate else None)
        for s, ref in self.tuners.items():
            ref.feed(x[s])

    def readings(self):
        return ({s: ref.latest() for s, ref in self.meters.items()}, {s: ref.latest() for s, ref in self.tuners.items()})

    def entries(self):
        """per stage name: the rows that have an entry now (mix: the members of a group)"""
        out = {st.name: (st.members() if st.name == "mix" else st.entries()) for st in self.stages}
        out["meter"], out["tuner"] = set(self.meters), set(self.tuners)
        return out

    # ---- the coverage conditions, on the reference side ----
    def assert_covered(self, what=()):
        gate, comp = self.by_name["gate"], self.by_name["compressor"]
        for s in FULL_ROWS:
            G.assert_covered(gate.refs[s], np.concatenate(gate.c.gains[s]), what + ("gate", s))
        done = {row: (ref, gains) for row, ref, gains in comp.left}
        done.update({s: (comp.refs[s], comp.gains[s]) for s in comp.entries()})
        for s in FULL_ROWS:
            CK.assert_inputs_reach_every_case(done[s][0], done[s][1], what + ("compressor", s))
        for name in ("mod", "delay"):
            assert self.by_name[name].oldest > RING, (what, name, "no ring wraps: the oldest entry has produced", self.by_name[name].oldest)
        for name in AUDIO:
            assert FULL_ROWS <= self.had[name], (what, name, "rows with an entry", self.had[name])
            assert self.had[name] == self.changed[name], (what, name, "the restatement left rows as they were", self.had[name] - self.changed[name])


# ---- the scenario ----

FULL_ROWS = {0, 4, 8}  # one per family: an entry in every audio stage
TAIL = [300, 200, 200]
CALLS = list(H.RAGGED) + [255, 256, 257, 2049] + TAIL
# The issue's list adds up to 3471 samples, and the smallest delay and modulation ring is 4096: three plain calls behind it take the
# entries of rows 0 and 8 (T0 at samples 33 and 225) past the wrap.  They are also the stretch without operations that Submit needs.


def irs():
    rng = np.random.default_rng(77)
    return {"a": (0.3 * R.decaying(rng, 200)).astype(F), "b": (0.25 * R.decaying(rng, 300)).astype(F)}  # more than one slice of 128 taps


def rev_irs():
    rng = np.random.default_rng(78)
    return {"room": (0.3 * R.decaying(rng, 600)).astype(F), "plate": (0.3 * R.decaying(rng, 300)).astype(F)}  # partitions and tails


def signal(total, seed=0):
    """[ROWS, total]: bursts at 0.25 and quiet stretches behind 60 quiet samples (the gate tests' signal), every row from its own noise;
    row 6 is fed row 4's input (the host contract of a hand-over)"""
    x = np.stack([G.gate_signal(500 * seed + r, total, lead=60) for r in range(H.ROWS)])
    x[6] = x[4]
    return x


def stand_in(total, seed=0):
    """rows that stand in for model outputs on the CPU: clipped noise at the level of H.noise"""
    return np.stack([H.noise(total, 9000 + 100 * seed + r) for r in range(H.ROWS)])


SLOW = dict(attack=1e-37, release=0.02)  # a follower that creeps up through the subnormals (see ops)
COMP = {0: CK.params(0.3, 0.02, threshold_db=-60.0, ratio=4.0, knee_db=6.0, makeup_db=3.0), 4: CK.params(0.5, 0.05, threshold_db=-50.0, ratio=8.0, knee_db=0.0),
        8: CK.params(0.2, 0.25, threshold_db=-55.0, ratio=2.5, knee_db=12.0, makeup_db=6.0), 6: CK.params(0.3, 0.1, threshold_db=-50.0, ratio=4.0, knee_db=6.0)}
TREMOLO = K.params(30.0, 10.0, K.phase_inc(6.0), K.SINE, 1, wet=0.5, dry=1.0, tremolo=0.8)
METER, TUNER = MT.params(48, 0.2, 0.2), T.params(2, 100, 2, 64, 37)


def ops(dry=True):
    """The operations per call (calls start at samples 0, 1, 16, 33, 97, 225, 354, 654, 909, 1165, 1422, 3471, 3771, 3971).  The gates
    of rows 0, 4 and 8 start closed with a floor of 0, so everything behind them is exact zeros until the first burst opens them; the
    compressors are set inside that silence with an attack coefficient of 1e-37: their followers start at zero and creep through the
    subnormals once the gate opens, and the mid-run change gives them ordinary coefficients.  Fade lengths are chosen so that every fade
    is still running at the next call's start.  dry=False: the mix groups' third member is an OUT tap -- a resampling batch refuses DRY
    taps (its rows lag the input by the resampler's latency), so the ladder behind the resampler mixes row 5's output instead."""
    third = MX.DRY if dry else MX.OUT
    slow = lambda s: dict(COMP[s], attackCoeff=float(F(SLOW["attack"])))
    mixA = [[0.8, 0.3, 0.2], [0.25, 0.7, -0.4]]
    mixB = [[0.5, 0.5, 0.0], [0.1, 0.9, 0.3]]
    return {
        0: [("gate", s, G.params(), False) for s in (0, 4, 8)] + [("gate", 1, G.params(floorGain=0.1), True)],
        1: [("comp", 0, slow(0), 40), ("eq", 0, E.cascade(3, 1), 20)],
        2: [("comp", 4, slow(4), 100), ("eq", 4, E.cascade(8, 2), 100), ("ir", 0, "a", 30), ("gain", 0, 0.7, 50), ("delay", 1, D.params(40, 0.4), 0),
            ("eq", 5, E.cascade(2, 5), 0), ("meter", 0, METER), ("meter", 4, METER), ("meter", 8, MT.params(100, 0.1, 0.3))],
        3: [("comp", 8, slow(8), 70), ("eq", 8, E.cascade(1, 3), 200), ("ir", 4, "b", 100), ("mod", 0, K.chorus(), 100), ("delay", 0, D.filtered(90), 100),
            ("tuner", 0, TUNER), ("tuner", 4, T.params(1, 64, 2, 40, 16, 3)), ("tuner", 8, TUNER)],
        4: [("comp", 0, COMP[0], 200), ("ir", 8, "a", 150), ("mod", 4, K.flanger(48.0, 20.0, 0.7), 200), ("delay", 4, D.params(250, 0.5), 200),
            ("reverb", 0, "room", 0.3, 1.0, 150), ("reverb", 5, "plate", 0.5, 0.8, 150), ("gain", 4, 0.8, 200), ("mix", [0, 4, 5], mixA, [MX.OUT, MX.OUT, third], 200)],
        5: [("gate", 0, G.params(holdSamples=40, releaseSamples=48), True), ("comp", 4, COMP[4], 200), ("mod", 8, TREMOLO, 150), ("delay", 8, D.filtered(120, 0.5), 150),
            ("reverb", 4, "plate", 0.4, 0.9, 200), ("gain", 8, 0.9, 150), ("park", 1)],
        6: [("gate", 4, G.params(attackSamples=24, releaseSamples=80), True), ("comp", 8, COMP[8], 350), ("eq", 0, E.cascade(2, 4), 350), ("eq", 4, E.cascade(3, 7), 320),
            ("ir", 4, "a", 320), ("reverb", 8, "room", 0.25, 1.0, 350), ("gain", 4, 0.6, 350), ("gain", 5, 0.5, 400)],
        7: [("gate", 8, G.params(holdSamples=30, attackSamples=48), True), ("ir", 0, "b", 300), ("mod", 4, K.flanger(30.0, 10.0, -0.5), 300),
            ("delay", 0, D.filtered(200, 0.4), 300), ("delay", 4, D.params(100, 0.6, wet=0.5), 300), ("mix", [0, 4, 5], mixB, [MX.OUT, MX.OUT, third], 300), ("activate", 1)],
        8: [("eq", 8, E.cascade(4, 8), 300), ("mod", 0, K.chorus(depth=100.0, base=300.0, rate_hz=3.0), 300), ("reverb", 4, "room", 0.3, 1.0, 300), ("gain", 0, 1.3, 300),
            ("gate", 1, G.params(), True), ("delay", 1, D.filtered(60), 50), ("handover", 4, 6, 400)],
        9: [("ir", 8, "b", 300), ("mod", 8, K.params(60.0, 20.0, K.phase_inc(2.0), K.TRIANGLE, 2, (0, 0x80000000, 0, 0), [0.6, 0.4, 0, 0], 0.0, 0.8, 0.7), 300),
            ("delay", 8, D.params(300, 0.3), 300), ("reverb", 0, "plate", 0.4, 0.9, 300), ("gain", 8, 0.5, 400),
            ("gate", 6, G.params(), True), ("eq", 6, E.cascade(3, 6), 300), ("ir", 6, "a", 300), ("comp", 6, COMP[6], 300), ("mod", 6, K.chorus(rate_hz=5.0), 300),
            ("delay", 6, D.filtered(150), 300), ("reverb", 6, "plate", 0.3, 1.0, 300), ("gain", 6, 0.8, 300), ("meter", 6, METER), ("tuner", 6, TUNER)],
        10: [("reverb", 8, "plate", 0.35, 0.9, 2100)],
        11: [("mix", [8, 0, 5], mixA, [MX.OUT, MX.OUT, third], 350)],
    }


REACTIVATED = (1, 7)  # row 1 comes back in front of call 7 and runs that call without an entry in any stage


def with_mirrored_parks(calls, ops):
    """ops with ("park", from, True) in front of the operations of the call whose top the output stage parks `from` at.  The positions of
    a fade do not depend on the samples, so the output stage's contract on silence tells."""
    out, contract = {}, H.Contract()
    for i, n in enumerate(calls):
        mirrored = [("park", f, True) for f in contract.finished]
        for op in ops.get(i, ()):
            if op[0] in OutRung.kinds + ("park",):
                contract.apply(op)
        contract.step(np.zeros((H.ROWS, n), F))
        out[i] = mirrored + list(ops.get(i, ()))
    return out


def live_sets(calls, sched, k):
    """The rows that are live in each call on rung k, as the operations leave them: a rung with the output stage parks `from` by itself
    (its own contract, advanced on silence), the others are told to."""
    has_out = k > OUT
    live, contract, out = set(H.LIVE), H.Contract(), []
    for i, n in enumerate(calls):
        for op in sched.get(i, ()):
            mirrored = len(op) > 2 and op[0] == "park" and op[2] is True
            if op[0] == "park" and not (mirrored and has_out):
                live.discard(op[1])
            elif op[0] == "activate" or op[0] == "handover":
                live.add(op[2] if op[0] == "handover" else op[1])
            if has_out and not mirrored and op[0] in OutRung.kinds + ("park",):
                contract.apply(op)
        if has_out:
            live -= set(contract.finished)  # (parked at the top of this call)
            contract.step(np.zeros((H.ROWS, n), F))
        out.append(frozenset(live))
    return out


# ---- the batches ----

def enable(b, k, cab=None, rev=None):
    """the first k stages of the chain on batch b, and the IRs loaded: returns {"cab": name -> id, "rev": name -> id}"""
    calls = [b.EnableGateStage, b.EnableEqStage, lambda: b.EnableCabinetStage(CAB_TAPS), b.EnableCompressorStage, lambda: b.EnableModStage(MOD_DELAY),
             lambda: b.EnableDelayStage(DELAY_MAX), lambda: b.EnableReverbStage(REV_TAPS), b.EnableOutputStage, b.EnableMixStage, b.EnableMeterStage, b.EnableTunerStage]
    for call in calls[:k]:
        call()
    ids = {"cab": {}, "rev": {}}
    if k > AUDIO.index("cabinet"):
        ids["cab"] = {name: b.LoadIR(taps) for name, taps in (irs() if cab is None else cab).items()}
    if k > AUDIO.index("reverb"):
        ids["rev"] = {name: b.LoadReverbIR(taps) for name, taps in (rev_irs() if rev is None else rev).items()}
    return ids


def drive(b, op, k, ids):
    """one operation on the batch of rung k: a stage the rung does not have ignores its operations (a hand-over is then the activation
    alone), and a rung with the output stage performs the mirrored park by itself"""
    kind, s = op[0], op[1]
    if kind == "park":
        if not (len(op) > 2 and op[2] is True and k > OUT):
            b.ParkStream(s)
        return
    if kind == "activate":
        b.ActivateStream(s, 1.0)
        return
    if STAGE_OF[kind] >= k:
        if kind == "handover":
            b.ActivateStream(op[2], 1.0)
        return
    if kind == "gate":
        b.SetStreamGate(s, op[2], op[3])
    elif kind == "ungate":
        b.SetStreamGate(s, None)
    elif kind == "eq":
        b.SetStreamEq(s, op[2], op[3])
    elif kind == "ir":
        b.SetStreamIR(s, -1 if op[2] is None else ids["cab"][op[2]], op[3])
    elif kind == "comp":
        b.SetStreamCompressor(s, op[2], op[3])
    elif kind == "mod":
        b.SetStreamMod(s, op[2], op[3])
    elif kind == "delay":
        b.SetStreamDelay(s, op[2], op[3])
    elif kind == "reverb":
        b.SetStreamReverb(s, -1 if op[2] is None else ids["rev"][op[2]], op[3], op[4], op[5])
    elif kind == "gain":
        b.SetStreamGain(s, op[2], op[3])
    elif kind == "handover":
        b.Handover(op[1], op[2], 1.0, op[3])
    elif kind == "mix":
        b.SetMixGroup(op[1], op[2], len(op[2]), op[3], op[4])
    elif kind == "meter":
        b.SetStreamMeter(s, op[2])
    elif kind == "tuner":
        b.SetStreamTuner(s, op[2])
    else:
        raise KeyError(op)


def stage_entries(b):
    """what every stage's Get call reports for every row of an all-stage batch: per stage name the rows that have an entry"""
    rows = range(b.NumStreams())
    return {"gate": {s for s in rows if b.GetStreamGate(s) is not None}, "eq": {s for s in rows if b.GetStreamEq(s) or b.StreamEqFadeRemaining(s)},
            "cabinet": {s for s in rows if b.GetStreamIR(s) != -1 or b.IRFadeRemaining(s)}, "compressor": {s for s in rows if b.GetStreamCompressor(s) is not None},
            "mod": {s for s in rows if b.GetStreamMod(s) is not None}, "delay": {s for s in rows if b.GetStreamDelay(s) is not None},
            "reverb": {s for s in rows if b.GetStreamReverb(s)[0] != -1 or b.ReverbFadeRemaining(s)},
            "output": {s for s in rows if b.GetStreamGain(s) != 1.0 or b.HandoverRemaining(s)}, "mix": {s for s in rows if b.GetStreamMix(s) is not None},
            "meter": {s for s in rows if b.GetStreamMeter(s) is not None}, "tuner": {s for s in rows if b.GetStreamTuner(s) is not None}}


def check_rows(y, below, exp, parked, what):
    """one rung's rows of one call against the stage's expectation on the rows below: every row, every sample.  Returns the samples
    compared."""
    assert y.shape == below.shape == exp.e.shape
    for s in range(y.shape[0]):
        where = what + ("row", s)
        if s in parked:
            assert not np.any(y[s]), where + ("a parked row is silence",)
        elif s not in exp.touched:
            assert same_bits(y[s], below[s]), where + ("no entry: the bits of the rung below", int(np.count_nonzero(bits(y[s]) != bits(below[s]))))
        elif exp.limit is None:
            diff = np.flatnonzero(bits(y[s]) != bits(exp.e[s]))
            assert len(diff) == 0, where + ("first at", int(diff[0]), float(y[s][diff[0]]), float(exp.e[s][diff[0]]), "of", len(diff))
        else:
            err = np.abs(y[s].astype(np.float64) - exp.e[s])
            assert np.all(err <= exp.limit[s]), where + ("sample", int(np.argmax(err - exp.limit[s])), float(np.max(err)), float(np.max(err / exp.limit[s])))
    return y.size
