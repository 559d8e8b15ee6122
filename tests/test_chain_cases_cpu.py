"""The ladder's helper (tests/chain_cases.py) without a device, on stand-in rows -- clipped noise at the level of H.noise where the
GPU file has the rows of the rung below: every adaptor returns what its stage's own contract class returns, the scenario meets its
coverage conditions, adjacent stages do not commute on the scenario's rows (which is what lets the ladder tell a swapped chain from a
correct one), and the mirrored park leaves every rung with the same live set."""
import numpy as np
import pytest

import cabinet_cases as CB
import chain_cases as CC
import compressor_cases as CK
import delay_cases as D
import eq_cases as E
import gate_cases as G
import handover_cases as H
import mix_cases as MX
import mod_cases as K
import reverb_cases as R

F = np.float32
TW = R.twiddles_numpy()
CALLS = CC.CALLS
STARTS = np.concatenate([[0], np.cumsum(CALLS)])


@pytest.fixture(scope="module")
def scen():
    total = sum(CALLS)
    return dict(x=CC.signal(total), rows=CC.stand_in(total), sched=CC.with_mirrored_parks(CALLS, CC.ops()))


def compose(scen, order, each=None):
    """the composition in `order` over the whole scenario; each(chain, i) runs behind the operations of call i.  Returns (rows, chain)."""
    chain = CC.Chain(CC.irs(), CC.rev_irs(), TW, order=order)
    out = []
    for i in range(len(CALLS)):
        lo, hi = STARTS[i], STARTS[i + 1]
        if "output" in order:
            assert chain.mirrored() == [op for op in scen["sched"][i] if op[0] == "park" and len(op) > 2], ("call", i)
        for op in scen["sched"][i]:
            chain.apply(op)
        if each:
            each(chain, i)
        out.append(chain.compose(scen["x"][:, lo:hi], scen["rows"][:, lo:hi]))
    return np.concatenate(out, axis=1), chain


class Direct:
    """One stage's own contract class driven by the scenario without the adaptor: what the composer must return for that stage alone."""

    def __init__(self, name):
        self.name, self.parked = name, set(range(H.ROWS)) - set(H.LIVE)
        per_row = {"eq": E.EqRef, "compressor": CK.CompRef, "mod": K.ModRef, "delay": D.DelayRef}
        self.refs = {s: per_row[name]() for s in range(H.ROWS)} if name in per_row else None
        self.c = {"gate": lambda: G.Contract(H.ROWS, range(H.ROWS)), "cabinet": lambda: CB.CabContract(H.ROWS, CC.irs()),
                  "reverb": lambda: R.RevContract(H.ROWS, CC.rev_irs(), TW), "output": H.Contract, "mix": list}.get(name, lambda: None)()

    def apply(self, op):
        kind, name = op[0], self.name
        if kind == "park":
            s = op[1]
            self.parked.add(s)
            if self.refs:
                self.refs[s] = type(self.refs[s])()
            elif name == "gate":
                self.c.gate[s] = None
            elif name in ("cabinet", "reverb"):
                self.c.leave(s)
            elif name == "output":
                self.c.apply(("park", s))
            else:
                self.c = [ref for ref in self.c if s not in ref.streams]
        elif kind in ("activate", "handover"):
            self.parked.discard(op[2] if kind == "handover" else op[1])
            if name == "output":
                self.c.apply(op)
        elif CC.STAGE_OF[kind] >= len(CC.AUDIO) or CC.AUDIO[CC.STAGE_OF[kind]] != name:
            return  # (another stage's operation)
        elif name in ("gate", "output"):
            self.c.apply(op)
        elif name == "cabinet":
            self.c.set_ir(op[1], op[2], op[3])
        elif name == "reverb":
            self.c.set(op[1], op[2], op[3], op[4], op[5])
        elif name == "mix":
            old = [ref for ref in self.c if ref.streams == list(op[1])]
            if old:
                old[0].set(op[2], op[4])
            else:
                self.c.append(MX.MixRef(op[1], op[2], taps=op[3], R=op[4]))
        elif name == "delay":
            self.refs[op[1]].set(op[2], op[3])
        elif name == "eq":
            self.refs[op[1]].set(op[2], op[3])
        else:
            assert self.refs[op[1]].set(op[2], op[3]) is True

    def step(self, x, rows):
        rows, name = rows.copy(), self.name
        rows[sorted(self.parked)] = 0.0
        if name == "gate":
            e = self.c.step(x, rows)
        elif name == "cabinet":
            e = self.c.step(rows)[0]
        elif name == "reverb":
            e = self.c.step(rows)[0]
        elif name == "output":
            e = self.c.step(rows)[0]
        elif name == "mix":
            e = MX.run_groups(self.c, rows, x)
        else:
            e = rows.copy()
            for s, ref in self.refs.items():
                if name == "eq" and ref.is_entry:
                    e[s] = ref.run(rows[s])
                elif name == "compressor" and ref.has:
                    e[s] = (rows[s] * ref.run(rows[s])).astype(F)
                elif name == "mod" and ref.has:
                    e[s] = ref.run(rows[s])
                elif name == "delay" and ref.on:
                    e[s] = ref.process(rows[s])
        with np.errstate(over="ignore"):
            e = np.ascontiguousarray(e, F)
        e[sorted(self.parked)] = 0.0
        return e


@pytest.mark.parametrize("name", CC.AUDIO)
def test_one_stage_alone_is_its_own_contract(scen, name):
    """With entries in one stage only the composer returns, on the bits, what that stage's contract class returns when the scenario
    drives it directly; and the stage does something to every row it has an entry on."""
    y, chain = compose(scen, (name,))
    direct, out = Direct(name), []
    for i in range(len(CALLS)):
        lo, hi = STARTS[i], STARTS[i + 1]
        for op in scen["sched"][i]:
            direct.apply(op)
        out.append(direct.step(scen["x"][:, lo:hi], scen["rows"][:, lo:hi]))
    e = np.concatenate(out, axis=1)
    for s in range(H.ROWS):
        assert CC.same_bits(y[s], e[s]), (name, "row", s)
    assert CC.FULL_ROWS <= chain.had[name] == chain.changed[name]
    untouched = set(range(H.ROWS)) - chain.had[name] - {1, 4, 6}  # (rows 1, 4 and 6 are parked for a while)
    assert 9 in untouched and all(CC.same_bits(y[s], scen["rows"][s] if s in H.LIVE else 0 * y[s]) for s in untouched)


def test_the_scenario_meets_its_coverage_conditions(scen):
    """The whole chain composed on the stand-in rows: the gates close and reopen, the compressors reach every case, the delay and
    modulation rings wrap, the IRs are longer than a slice and than the reverb's head, every restatement changes every row it has an
    entry on, rows 0, 4 and 8 have an entry in every audio stage, row 9 in none; row 1 comes back with no entry anywhere and row 6
    gets its entries behind the call that activates it."""
    seen = {}

    def each(chain, i):
        seen[i] = (chain.entries(), set(chain.parked))

    y, chain = compose(scen, CC.AUDIO, each)
    chain.assert_covered()
    assert all(len(h) > 128 for h in CC.irs().values()) and all(len(h) > R.P for h in CC.rev_irs().values())  # (a cabinet slice: 128 taps)
    assert max(CALLS) > K.PIECE and CALLS[:11] == list(H.RAGGED) + [255, 256, 257, 2049]
    assert not any(9 in rows for rows in chain.had.values()) and CC.same_bits(y[9], scen["rows"][9])
    assert chain.had["gate"] >= {1} and chain.had["delay"] >= {1} and chain.had["eq"] >= {5} and chain.had["reverb"] >= {5} and chain.had["output"] >= {5}
    row, call = CC.REACTIVATED
    assert row in seen[call - 1][1] and row not in seen[call][1] and not any(row in rows for rows in seen[call][0].values())
    assert CC.same_bits(y[row, STARTS[call]:STARTS[call + 1]], scen["rows"][row, STARTS[call]:STARTS[call + 1]])
    assert {"gate", "delay"} <= {name for name, rows in seen[call + 1][0].items() if row in rows}
    first = min(i for i in seen if 6 not in seen[i][1])
    assert not any(6 in rows for name, rows in seen[first][0].items() if name != "output") and all(6 in seen[first + 1][0][name] for name in CC.AUDIO[:CC.OUT])
    faded = {}
    for i, v in scen["sched"].items():  # every fade of rows 0, 4 and 8 set in front of call i is still running when call i + 1 starts
        for op in v:
            if op[0] in ("eq", "ir", "comp", "mod", "delay", "reverb", "gain", "mix", "handover") and op[-1] > 0 and (op[0] == "mix" or op[1] in CC.FULL_ROWS):
                assert op[-1] > CALLS[i], ("call", i, op[0])
                faded.setdefault(CC.AUDIO[CC.STAGE_OF[op[0]]], set()).update(op[1] if op[0] == "mix" else [op[1]])
    assert all(CC.FULL_ROWS <= faded[name] for name in CC.AUDIO if name != "gate"), faded  # (the gate has no fade)


@pytest.mark.parametrize("pair", list(zip(CC.AUDIO[:-1], CC.AUDIO[1:])), ids="-".join)
def test_adjacent_stages_do_not_commute(scen, pair):
    """Two adjacent stages alone, composed in StageId order and swapped: every row that has an entry in both gets different bits."""
    y, chain = compose(scen, pair)
    z, _ = compose(scen, pair[::-1])
    both = chain.had[pair[0]] & chain.had[pair[1]]
    assert CC.FULL_ROWS <= both
    for s in both:
        assert not CC.same_bits(y[s], z[s]), (pair, "row", s)


def test_the_mirrored_park_gives_every_rung_the_same_live_set(scen):
    """Rungs with the output stage park `from` by themselves at the top of the call behind the fade's last sample; the others are told
    to at the same call: every rung has the same live rows in every call, row 4 leaves in front of the long call and row 6 has joined."""
    sets = {k: CC.live_sets(CALLS, scen["sched"], k) for k in CC.RUNGS}
    for k in CC.RUNGS:
        assert sets[k] == sets[0], ("rung", k)
    assert [op for op in scen["sched"][10] if op[0] == "park"] == [("park", 4, True)]
    assert 4 in sets[0][9] and 4 not in sets[0][10] and 6 not in sets[0][7] and 6 in sets[0][8]
    without = CC.live_sets(CALLS, CC.ops(), 0)
    assert 4 in without[10], "without the mirrored park the lower rungs keep row 4 running"


def test_the_resampling_variant_differs_in_the_third_tap_alone():
    """A resampling batch refuses DRY taps, so the ladder behind the resampler runs ops(dry=False): the same operations, the mix groups'
    third member an OUT tap; the mix adaptor still rewrites rows 0, 4 and 8 and changes their bits."""
    a, b = CC.ops(), CC.ops(dry=False)
    assert a.keys() == b.keys()
    mixes = 0
    for i in a:
        assert len(a[i]) == len(b[i])
        for p, q in zip(a[i], b[i]):
            if p[0] == "mix":
                assert p[:3] == q[:3] and p[4] == q[4] and p[3] == [MX.OUT, MX.OUT, MX.DRY] and q[3] == [MX.OUT] * 3
                mixes += 1
            else:
                assert p[0] == q[0] and p[1] == q[1] and repr(p) == repr(q)
    assert mixes == 3
    total = sum(CALLS)
    scen = dict(x=CC.signal(total), rows=CC.stand_in(total), sched=CC.with_mirrored_parks(CALLS, b))
    y, chain = compose(scen, ("mix",))
    assert CC.FULL_ROWS <= chain.had["mix"] == chain.changed["mix"]
