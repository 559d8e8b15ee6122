"""GPU tests of the whole per-stream stage chain at once: gate, EQ, cabinet, compressor, modulation, delay, reverb,
output gain, mix, and the meter's and the tuner's taps, all enabled and all with entries on the same rows.

Part 1 is the LADDER of tests/chain_cases.py on the twelve-row batch of tests/handover_cases.py: rung k has the first k audio stages,
and stage k's own restatement is evaluated on rung k-1's rows of the same call -- bits where the contract fixes them, the cabinet's and
the output stage's own bounds where it does not; no tolerance is introduced here.  Part 2 runs the all-stage batch through every entry
point against the top rung's bits.  Part 3 grows a plain batch with live rings in every stage, removes a row that has an entry in
every stage and recycles its slot."""
import os

import numpy as np
import pytest

import chain_cases as CC
import delay_cases as D
import eq_cases as E
import gate_cases as G
import handover_cases as H
import meter_cases as MT
import mix_cases as MX
import mod_cases as K
import reverb_cases as R
import tuner_cases as T

FORCED = bool(os.environ.get("NA_WN_KERNEL") or os.environ.get("NA_WN_PACK") or os.environ.get("NA_WN_SPEC") or os.environ.get("NA_SP_T")
              or os.environ.get("NA_SP_GEN") or os.environ.get("NA_WN_PAD"))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(FORCED, reason="forced kernel family")]

F = np.float32
COUNTERS = {"gate": "NA_DebugGateLaunches", "eq": "NA_DebugEqLaunches", "cabinet": "NA_DebugCabinetLaunches", "compressor": "NA_DebugCompressorLaunches",
            "mod": "NA_DebugModLaunches", "delay": "NA_DebugDelayLaunches", "reverb": "NA_DebugReverbLaunches", "mix": "NA_DebugMixLaunches",
            "stash": "NA_DebugMixStashLaunches", "meter": "NA_DebugMeterLaunches", "tuner": "NA_DebugTunerLaunches"}  # (the output stage has none)
ENABLED_FROM = {"gate": 1, "eq": 2, "cabinet": 3, "compressor": 4, "mod": 5, "delay": 6, "reverb": 7, "mix": 9, "stash": 9, "meter": 10, "tuner": 11}
LADDER = {}


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


@pytest.fixture(scope="module")
def models(na):
    return H.load_models(na)


def counters():
    from neuralaudio_amd import capi
    lib = capi.load_library()
    return {name: int(getattr(lib, call)()) for name, call in COUNTERS.items()}


def delta(before):
    return {name: count - before[name] for name, count in counters().items()}


def readings(b):
    rows = range(b.NumStreams())
    return {s: MT.norm(b.ReadStreamMeter(s)) for s in rows}, {s: b.ReadStreamTuner(s) for s in rows}


class Rung:
    """what one batch of the ladder gave, call by call"""

    def __init__(self):
        self.rows, self.parked, self.entries, self.reads, self.rings = [], [], [], [], None


def run_rung(na, models, k, x, calls, sched, resample=None, path="process"):
    """The twelve-row batch with the first k stages of the chain through `path`, the operations of sched[i] in front of call i."""
    b = H.make_batch(na, models, stage=False, resample=resample)
    out, pos = Rung(), 0
    runner = H.Runner(na, b, path)
    try:
        ids = CC.enable(b, k)
        if k == CC.TOP:
            out.rings = (b.GetModInfo()["ringSamples"], b.GetDelayInfo()["ringSamples"])
        for i, n in enumerate(calls):
            for op in sched[i]:
                CC.drive(b, op, k, ids)
            if k == CC.TOP:
                out.entries.append(CC.stage_entries(b))
            out.rows.append(runner.call(x[:, pos:pos + n]))
            out.parked.append({s for s in range(H.ROWS) if b.IsParked(s)})
            if k == CC.TOP:
                b.Synchronize()
                out.reads.append(readings(b))
            pos += n
    finally:
        runner.close()
        b.close()
    return out


def ladder(na, models, rate):
    """Runs and checks the ladder at `rate` once; returns the top rung and what it was fed."""
    if rate in LADDER:
        return LADDER[rate]
    resample = None if rate == 48000 else rate
    calls, total = CC.CALLS, sum(CC.CALLS)
    x, sched = CC.signal(total), CC.with_mirrored_parks(CC.CALLS, CC.ops(dry=resample is None))
    rungs = {}
    for k in CC.RUNGS:
        before = counters()
        rungs[k] = run_rung(na, models, k, x, calls, sched, resample)
        for name, count in delta(before).items():  # a rung launches the kernels of its own stages only; rung 0 launches none
            runs = k >= ENABLED_FROM[name] and (name != "stash" or resample is None)  # (no DRY tap behind the resampler: nothing to stash)
            assert (count > 0) == runs, (rate, "rung", k, name, count)
    assert rungs[CC.TOP].rings == (CC.RING, CC.RING)
    chain = CC.Chain(CC.irs(), CC.rev_irs(), R.library_twiddles())
    compared, pos = {k: 0 for k in CC.RUNGS}, 0
    for i, n in enumerate(calls):
        what = (rate, "call", i, "n", n)
        assert chain.mirrored() == [op for op in sched[i] if op[0] == "park" and len(op) > 2], what
        # (the batch parks the rows of a mirrored park inside the call: in front of it they still have their entries, and their mix group stands)
        leaving = {op[1] for op in sched[i] if op[0] == "park" and len(op) > 2}
        going = {"mix": {s for ref in chain.by_name["mix"].refs if leaving & set(ref.streams) for s in ref.streams}}
        for op in sched[i]:
            chain.apply(op)
        for k in CC.RUNGS:
            assert rungs[k].parked[i] == chain.parked, what + ("rung", k, "parked", rungs[k].parked[i], chain.parked)
        reported = {name: rows - leaving - going.get(name, set()) for name, rows in rungs[CC.TOP].entries[i].items()}
        assert reported == chain.entries(), what + ("the entries the Get calls report", reported, chain.entries())
        xs = x[:, pos:pos + n]
        assert not np.any(rungs[0].rows[i][sorted(chain.parked)]), what
        compared[0] += rungs[0].rows[i].size
        for k, name in enumerate(CC.AUDIO, 1):
            below = rungs[k - 1].rows[i]
            compared[k] += CC.check_rows(rungs[k].rows[i], below, chain.step_stage(name, xs, below), chain.parked, what + (name,))
        top, mix = rungs[CC.TOP].rows[i], rungs[len(CC.AUDIO)].rows[i]
        assert CC.same_bits(top, mix), what + ("the meter and the tuner write no audio",)
        compared[CC.TOP] += top.size
        chain.taps(xs, top)
        meters, tuners = chain.readings()
        got_meters, got_tuners = rungs[CC.TOP].reads[i]
        for s in range(H.ROWS):
            assert got_meters[s] == meters.get(s), what + ("meter", s, got_meters[s], meters.get(s))
            assert got_tuners[s] == tuners.get(s), what + ("tuner", s, got_tuners[s], tuners.get(s))
        pos += n
    assert all(count == H.ROWS * total for count in compared.values()), compared
    chain.assert_covered((rate,))
    assert all(ref.windows > 3 for ref in chain.meters.values()) and all(ref.evaluations > 3 for ref in chain.tuners.values())
    row, call = CC.REACTIVATED
    assert CC.same_bits(rungs[CC.TOP].rows[call][row], rungs[0].rows[call][row]) and np.any(rungs[0].rows[call][row])
    assert CC.same_bits(np.concatenate(rungs[CC.TOP].rows, axis=1)[9], np.concatenate(rungs[0].rows, axis=1)[9])
    LADDER[rate] = dict(x=x, calls=calls, sched=sched, top=rungs[CC.TOP])
    return LADDER[rate]


# ================================================================================================ 1: the ladder

@pytest.mark.parametrize("rate", [48000, 44100])
def test_the_ladder(na, models, rate):
    """The scenario of chain_cases.ops on eleven batches -- no stage, gate, gate + EQ, ... up to all eleven stages --, at the models' rate
    and behind the resampler of a 44.1 kHz host (there the mix groups' third member is an OUT tap: a resampling batch refuses DRY taps).  Per call and rung: the live set, every row against the stage's restatement on the
    rung below (bits; the cabinet's and the output stage's own bounds), rows without an entry the bits below, parked rows silence; on
    the top rung the bits of the mix rung, every stage's Get call against the reference's entries, and the meter and tuner readings of
    MeterRef (input rows, the top rung's own rows, the gate restatement's gains) and TunerRef (input rows).  The coverage conditions are
    asserted on the reference side, and every rung launches the kernels of its own stages only (rung 0: none)."""
    ladder(na, models, rate)


# ================================================================================================ 2: every entry point

def run_submit(na, models, x, calls, sched, expected):
    """three buffers in flight wherever no operation stands in front of a call; operations are issued with nothing in flight, where the
    readings must be those behind the last call"""
    b = H.make_batch(na, models, stage=False)
    rows, flight, most, pos = {}, [], 0, 0

    def drain(upto=0):
        while len(flight) > upto:
            ticket, i = flight.pop(0)
            rows[i] = b.Collect(ticket)

    try:
        ids = CC.enable(b, CC.TOP)
        for i, n in enumerate(calls):
            if any(len(op) == 2 or op[0] != "park" for op in sched[i]):  # (the mirrored park is the batch's own)
                drain()
                if i:
                    b.Synchronize()
                    assert readings(b) == expected.reads[i - 1], ("submit", "behind call", i - 1)
                for op in sched[i]:
                    CC.drive(b, op, CC.TOP, ids)
            drain(2)
            flight.append((b.Submit(np.ascontiguousarray(x[:, pos:pos + n])), i))
            most = max(most, len(flight))
            pos += n
        drain()
        b.Synchronize()
        assert readings(b) == expected.reads[-1] and most == 3
    finally:
        b.close()
    return [rows[i] for i in range(len(calls))]


def run_in_place(na, models, x, calls, sched, expected):
    """NA_BatchProcessDevice with dIn == dOut: the gate's detector, the mix stash, the meter's IN tap and the tuner read the rows the
    models then overwrite"""
    import torch
    dev = torch.device("cuda", 0)
    b = H.make_batch(na, models, stage=False)
    rows, pos = [], 0
    try:
        ids = CC.enable(b, CC.TOP)
        for i, n in enumerate(calls):
            for op in sched[i]:
                CC.drive(b, op, CC.TOP, ids)
            buf = torch.from_numpy(np.ascontiguousarray(x[:, pos:pos + n])).to(dev)
            torch.cuda.synchronize(dev)
            b.ProcessDevice(buf.data_ptr(), buf.data_ptr(), n, n, n)
            b.Synchronize()
            y = buf.cpu().numpy()
            y[[s for s in range(H.ROWS) if b.IsParked(s)]] = 0.0  # (device rows of parked streams are left alone: here, the input)
            rows.append(y)
            assert readings(b) == expected.reads[i], ("in place", "call", i)
            pos += n
    finally:
        b.close()
    return rows


@pytest.mark.parametrize("path", ["submit", "registered", "device", "device-odd", "in-place"])
def test_every_entry_point_gives_the_ladders_bits(na, models, path):
    """The all-stage batch and the ladder's scenario through Submit / Collect (three buffers in flight across the plain calls),
    registered host buffers, device pointers with aligned and with odd row strides (zeros behind every row must stay zeros) and device
    pointers with dIn == dOut: every call's rows are the top rung's Process bits, and the meter and tuner readings are the same."""
    ref = ladder(na, models, 48000)
    x, calls, sched, top = ref["x"], ref["calls"], ref["sched"], ref["top"]
    if path == "submit":
        rows = run_submit(na, models, x, calls, sched, top)
    elif path == "in-place":
        rows = run_in_place(na, models, x, calls, sched, top)
    else:
        got = run_rung(na, models, CC.TOP, x, calls, sched, path=path)
        rows = got.rows
        assert got.reads == top.reads and got.parked == top.parked
    for i in range(len(calls)):
        for s in range(H.ROWS):
            diff = np.flatnonzero(CC.bits(rows[i][s]) != CC.bits(top.rows[i][s]))
            assert len(diff) == 0, (path, "call", i, "row", s, "first at", int(diff[0]), "of", len(diff))


# ================================================================================================ 3: growth, removal, recycled rows

NANO_ROWS, LSTM_ROWS, GROWN = 3, 3, 14
WITH = (1, 4)  # a nano and an LSTM row with an entry in every stage


def plain(na, models, counts, k):
    b = na.Batch(0)
    for name, count in counts:
        b.AddStreams(models[name], count)
    return b, CC.enable(b, k)


def entry_ops(row, dry, fade, seed):
    """an entry in every stage for `row`; its mix group's second member is the DRY tap of row `dry`"""
    return [("gate", row, G.params(), True), ("eq", row, E.cascade(3, seed), fade), ("ir", row, "a", fade), ("comp", row, CC.COMP[0], fade),
            ("mod", row, K.flanger(48.0, 20.0, 0.7), fade), ("delay", row, D.filtered(90), fade), ("reverb", row, "room", 0.3, 1.0, fade), ("gain", row, 0.7, fade),
            ("meter", row, CC.METER), ("tuner", row, CC.TUNER), ("mix", [row, dry], [[0.8, 0.3]], [MX.OUT, MX.DRY], fade)]


def test_growth_removal_and_recycled_rows_with_every_stage(na, models):
    """A plain AddStreams batch of three nano and three LSTM rows with all eleven stages, rows 1 and 4 with an entry in every stage.
    Growth: fourteen more rows join between calls 1 and 2 (past every stage's first capacity of 16, so every ring moves at once); the
    old rows go on bit for bit as in a batch that had twenty rows from the start, and so do the readings.  A call of that batch
    launches, per stage, what the stage's own tests count.  Removal: row 4 goes, its slot is recycled; the new stream has no entry in
    any stage and its row is the row of a fresh batch without stages.  Given fresh entries it equals, bit for bit, the same row of a
    fresh all-stage batch with the same entries: nothing of the old history shows."""
    calls, tail = [300, 129, 300, 257], [200, 300]
    total, rows = sum(calls) + sum(tail), NANO_ROWS + LSTM_ROWS + GROWN
    x = np.stack([G.gate_signal(900 + r, total) for r in range(rows)])
    start = [(H.NANO, NANO_ROWS), (H.LSTM, LSTM_ROWS)]
    first = [op for s in WITH for op in entry_ops(s, s + 1, 100, s)]

    def run(b, ids, lo, n):
        y = b.Process(np.ascontiguousarray(x[:b.NumStreams(), lo:lo + n]))
        b.Synchronize()
        return y

    # -- growth
    grown, whole = plain(na, models, start, CC.TOP), plain(na, models, start + [(H.LSTM, GROWN)], CC.TOP)
    tuner, counted = T.TunerRef(CC.TUNER), None
    try:
        for b, ids in (grown, whole):
            for op in first:
                CC.drive(b, op, CC.TOP, ids)
        pos = 0
        for i, n in enumerate(calls):
            if i == 2:
                assert grown[0].AddStreams(models[H.LSTM], GROWN) == NANO_ROWS + LSTM_ROWS
            ya = run(*grown, pos, n)
            before = counters()
            yb = run(*whole, pos, n)
            if i == 2:
                ends = tuner.evaluations
                tuner.feed(x[1, pos:pos + n])
                counted = (delta(before), {"gate": 2, "eq": 1, "cabinet": 2, "compressor": 1, "mod": 1, "delay": 1, "reverb": R.expected_launches(pos, [n], True),
                                           "mix": 1, "stash": 1, "meter": 2, "tuner": 1 + (tuner.evaluations > ends)})
            else:
                tuner.feed(x[1, pos:pos + n])
            for s in range(NANO_ROWS + LSTM_ROWS):
                assert CC.same_bits(ya[s], yb[s]), ("growth", "call", i, "row", s)
            ra, rb = readings(grown[0]), readings(whole[0])
            assert all(ra[t][s] == rb[t][s] and ra[t][s] is not None for t in (0, 1) for s in WITH), ("growth", "call", i)
            pos += n
        assert counted[0] == counted[1], counted
        assert CC.stage_entries(grown[0]) == CC.stage_entries(whole[0]) and all(set(WITH) <= rows_ for rows_ in CC.stage_entries(grown[0]).values())
        # -- removal and the recycled slot
        b, ids = grown
        b.RemoveStreams(4, 1)
        assert b.AddStreams(models[H.LSTM], 1) == 4
        entries = CC.stage_entries(b)
        assert not any(4 in rows_ for rows_ in entries.values()) and entries["mix"] == {1, 2} and all(1 in rows_ for rows_ in entries.values())  # (row 4's group went with it)
        layout = [(H.NANO, NANO_ROWS), (H.LSTM, LSTM_ROWS + GROWN)]
        bare, fresh = plain(na, models, layout, 0), plain(na, models, layout, CC.TOP)
        try:
            y1, y1_bare, y1_fresh = run(b, ids, pos, tail[0]), run(*bare, pos, tail[0]), run(*fresh, pos, tail[0])
            assert CC.same_bits(y1[4], y1_bare[4]) and CC.same_bits(y1[4], y1_fresh[4]) and np.any(y1[4]), "a recycled row has no entry in any stage"
            assert readings(b)[0][4] is None and readings(b)[1][4] is None
            again = entry_ops(4, 5, 50, 11)
            for batch, its in ((b, ids), fresh):
                for op in again:
                    CC.drive(batch, op, CC.TOP, its)
            y2, y2_fresh = run(b, ids, pos + tail[0], tail[1]), run(*fresh, pos + tail[0], tail[1])
            diff = np.flatnonzero(CC.bits(y2[4]) != CC.bits(y2_fresh[4]))
            assert len(diff) == 0, ("the recycled row with fresh entries", "first at", int(diff[0]), "of", len(diff))
            assert not CC.same_bits(y2[4], run(*bare, pos + tail[0], tail[1])[4])
            ra, rb = readings(b), readings(fresh[0])
            assert all(ra[t][4] == rb[t][4] and ra[t][4] is not None for t in (0, 1))
        finally:
            bare[0].close()
            fresh[0].close()
    finally:
        grown[0].close()
        whole[0].close()
