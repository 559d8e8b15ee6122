"""CPU-side tests of the gate stage (NA_GateParamsFromDb / NA_BatchEnableGateStage / GetGateInfo / SetStreamGate / GetStreamGate /
StreamGateGain): the binding list, the header, NA_GateParamsFromDb's arithmetic, what the calls do where there is no device, and
csrc/gate_stage.h -- the step function and the host book the kernels and the batch are built on -- run without a device
(tests/gate_cases.cpp) against the numpy float32 restatement of the contract (tests/gate_cases.py), bit for bit.  Everything that runs
on the device is in tests/test_gpu_gate.py."""
import ctypes as C
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import gate_cases as G
import handover_cases as H
import na_oracle as O

STAGE = ["NA_GateParamsFromDb", "NA_BatchEnableGateStage", "NA_BatchGetGateInfo", "NA_BatchSetStreamGate", "NA_BatchGetStreamGate",
         "NA_BatchStreamGateGain"]
HOOKS = ["NA_DebugGateLaunches"]
STEP = ["x' = (x is NaN) ? 0 : min(|x|, 1e18f)",
        "s = fl(x' * x');  d = fl(s - p);  p = fl(p + fl(a * d))",
        "if      p >= Po:  open = 1, hold = H",
        "else if p <  Pc:  if hold > 0: hold -= 1  else: open = 0",
        "u = open ? min(U, u + stepUp) : (u > stepDown ? u - stepDown : 0)",
        "g = (u == U) ? 1.0f : fl(floor + fl(span * fl((float)u * 2^-30)))",
        "y = fl(y * g)"]


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    return neuralaudio_amd


def test_the_gate_stage_is_bound_declared_and_exported(na):
    """The six calls are public: in capi.NA_SYMBOLS, declared outside the header's test-build block and exported by the library the
    tests load; the hook is declared inside that block; Batch has the methods; the header holds the step's formulas word for word."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    header = open(os.path.join(O.ROOT, "include", "neuralaudio_amd.h")).read()
    public, hooks = header.split("#ifndef NA_RELEASE")[0], header.split("#ifndef NA_RELEASE")[1]
    declared = set(re.findall(r"NA_EXTERN[^;(]*?\b(NA_[A-Za-z0-9]+)\(", public))
    debug = set(re.findall(r"NA_EXTERN[^;(]*?\b(NA_[A-Za-z0-9]+)\(", hooks))
    for name in STAGE:
        assert name in capi.NA_SYMBOLS and name in declared, name
        getattr(lib, name)
    for name in HOOKS:
        assert name in capi.NA_SYMBOLS and name in debug and name not in declared, name
        getattr(lib, name)
    for method in ("EnableGateStage", "GetGateInfo", "SetStreamGate", "GetStreamGate", "StreamGateGain"):
        assert callable(getattr(na.Batch, method))
    assert callable(na.gate_params_from_db)
    assert ("typedef struct NA_GateParams { float openPower, closePower, floorGain, detectorCoeff; int attackSamples, holdSamples, releaseSamples; } "
            "NA_GateParams;") in public
    assert "typedef struct NA_GateInfo { int gainSamples, numGates; long long deviceBytes; } NA_GateInfo;" in public
    for text in STEP + ["span = fl(1 - floor)", "U = 2^30", "stepUp = ceil(U / A)", "stepDown = ceil(U / R)", "no FMA contraction"]:
        assert text in public, text
    kernel_header = open(os.path.join(O.ROOT, "neuralaudio_amd", "csrc", "gate_stage.h")).read()
    for text in STEP:
        assert text in kernel_header, text
    assert [name for name, _ in capi.NA_GateParams._fields_] == list(G.FIELDS)
    assert [name for name, _ in capi.NA_GateInfo._fields_] == ["gainSamples", "numGates", "deviceBytes"]


def test_gate_params_from_db_matches_its_formulas(na):
    """power = 10^(dB/10) / 2 rounded once, floorGain = 10^(dB/20) with -inf -> 0, detectorCoeff = 1 - exp(-1 / (ms * rate / 1000)) in
    double rounded once, sample counts max(1, round(ms * rate / 1000)) with hold allowed to be 0; every bad field is refused by name."""
    f32 = lambda v: float(np.float32(v))
    for rate, odb, cdb, fdb, det, att, hold, rel in ((48000, -40.0, -46.0, -60.0, 1.0, 0.5, 40.0, 120.0), (44100, -27.5, -33.25, float("-inf"), 2.5, 0.001, 0.0, 3.0),
                                                     (96000, -10.0, -10.0, 0.0, 0.01, 10.0, 0.004, 0.02)):
        p = na.gate_params_from_db(rate, odb, cdb, fdb, det, att, hold, rel)
        assert p["openPower"] == f32(10.0 ** (float(np.float32(odb)) / 10.0) / 2.0) and p["closePower"] == f32(10.0 ** (float(np.float32(cdb)) / 10.0) / 2.0)
        assert p["floorGain"] == (0.0 if fdb == float("-inf") else f32(10.0 ** (fdb / 20.0)))
        assert p["detectorCoeff"] == f32(1.0 - math.exp(-1.0 / (float(np.float32(det)) * rate / 1000.0)))
        count = lambda ms, least: max(least, int(math.floor(float(np.float32(ms)) * rate / 1000.0 + 0.5)))
        assert (p["attackSamples"], p["holdSamples"], p["releaseSamples"]) == (count(att, 1), count(hold, 0), count(rel, 1))
    assert na.gate_params_from_db(48000, -40, -46, hold_ms=0.0)["holdSamples"] == 0
    assert na.gate_params_from_db(48000, -40, -46, attack_ms=0.0)["attackSamples"] == 1
    good = dict(sample_rate=48000, open_db=-40.0, close_db=-46.0, floor_db=-60.0, detector_ms=1.0, attack_ms=1.0, hold_ms=50.0, release_ms=100.0)
    for change, field in ((dict(open_db=float("nan")), "openPower"), (dict(close_db=float("inf")), "closePower"), (dict(close_db=-30.0), "openPower must be >= closePower"),
                          (dict(floor_db=6.0), r"floorGain must lie in \[0, 1\]"), (dict(floor_db=float("nan")), "floorGain"), (dict(detector_ms=0.0), "detectorCoeff"),
                          (dict(detector_ms=-1.0), "detectorCoeff"), (dict(attack_ms=1e9), r"attackSamples must lie in \[1, 1 << 20\]"),
                          (dict(hold_ms=1e9), r"holdSamples must lie in \[0, 1 << 24\]"), (dict(release_ms=float("inf")), "releaseSamples"),
                          (dict(release_ms=1e9), r"releaseSamples must lie in \[1, 1 << 20\]")):
        args = dict(good)
        args.update(change)
        with pytest.raises(na.NeuralAudioError, match=field):
            na.gate_params_from_db(**args)


def test_without_a_batch_the_calls_fail_loudly(na):
    """The stage lives in a batch and a batch needs a device: on the batch that does not exist every call fails with the library's
    "no HIP device" error instead of crashing."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    info, p = capi.NA_GateInfo(), capi.NA_GateParams()
    calls = [(lambda: lib.NA_BatchEnableGateStage(None), lambda rc: rc != 0),
             (lambda: lib.NA_BatchGetGateInfo(None, C.byref(info)), lambda rc: rc != 0),
             (lambda: lib.NA_BatchSetStreamGate(None, 0, C.byref(p), 1), lambda rc: rc != 0),
             (lambda: lib.NA_BatchSetStreamGate(None, 0, None, 1), lambda rc: rc != 0),
             (lambda: lib.NA_BatchGetStreamGate(None, 0, C.byref(p)), lambda rc: rc < 0),
             (lambda: lib.NA_BatchStreamGateGain(None, 0), lambda rc: rc < 0)]
    for call, failed in calls:
        assert failed(call())
        assert "no HIP device" in capi.last_error()


# ---- csrc/gate_stage.h without a device ----

def _hex(v):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(np.float32(v))))[0]


def _f32(hexes):
    return np.array([int(h, 16) for h in hexes], np.uint32).view(np.float32)


class Program:
    """builds a script for tests/gate_cases.cpp and parses its answers"""
    ROWS = 4

    def __init__(self, exe):
        self.exe, self.lines, self.kinds = exe, [], []

    def set(self, row, p, start_open=True):
        self.lines.append("S %d %s %s %s %s %d %d %d %d" % (row, _hex(p["openPower"]), _hex(p["closePower"]), _hex(p["floorGain"]), _hex(p["detectorCoeff"]),
                                                            p["attackSamples"], p["holdSamples"], p["releaseSamples"], 1 if start_open else 0))
        self.kinds.append("S")

    def remove(self, row):
        self.lines.append("R %d" % row)
        self.kinds.append("R")

    def leave(self, row):
        self.lines.append("L %d" % row)
        self.kinds.append("L")

    def call(self, x):
        self.lines.append("X %d" % x.shape[1])
        self.lines += [" ".join("%08x" % v for v in row.view(np.uint32)) for row in np.ascontiguousarray(x, np.float32)]
        self.kinds.append("X")

    def run(self):
        """one answer per command: ("E", entries, [has gate per row]) or ("!", text); an X answers (gains {row: (g, state)}, E)"""
        out = subprocess.run([str(self.exe)], input="\n".join(self.lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        answers, i = [], 0
        for kind in self.kinds:
            gains = {}
            while out[i].startswith("G "):
                left, right = out[i].split(" | ")
                words, st = left.split(), right.split()
                gains[int(words[1])] = (_f32(words[2:]), (_f32(st[:1])[0], int(st[1]), int(st[2]), int(st[3])))
                i += 1
            if out[i].startswith("!"):
                answers.append(("!", out[i][2:]))
            else:
                words = out[i].split()
                assert words[0] == "E"
                e = ("E", int(words[1]), [int(w) for w in words[2:]])
                answers.append((gains, e) if kind == "X" else e)
            i += 1
        assert i == len(out)
        return answers


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("gate") / "gate_cases"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(O.ROOT, "neuralaudio_amd", "csrc"),
                    os.path.join(O.ROOT, "tests", "gate_cases.cpp"), "-o", str(path)], check=True)
    return path


ROW_OF = {"floor0": 0, "floor0.1": 1, "hold0": 2, "attack1": 3}


def _signal():
    return np.stack([G.gate_signal(10 + r) for r in range(Program.ROWS)])


def _cuts(total, kind):
    if kind == "one":
        return [total]
    return H.ragged(total)


@pytest.mark.parametrize("cut", ["one", "ragged"])
def test_the_step_and_the_book_equal_the_numpy_reference_bit_for_bit(exe, cut):
    """The four variations on four rows over the whole test signal, in one call and in RAGGED cuts: every gain and the state behind
    every call equal the reference's bits.  First the condition on the inputs: every row's reference gains show every case."""
    x = _signal()
    refs = {row: G.GateRef(G.variation(name)) for name, row in ROW_OF.items()}
    prog = Program(exe)
    for name, row in ROW_OF.items():
        prog.set(row, G.variation(name))
    calls = _cuts(x.shape[1], cut)
    pos = 0
    for n in calls:
        prog.call(x[:, pos:pos + n])
        pos += n
    answers = prog.run()[len(ROW_OF):]
    pos, whole = 0, {row: [] for row in refs}
    for n, (gains, e) in zip(calls, answers):
        assert e[1] == 4 and e[2] == [1, 1, 1, 1]
        for row, ref in refs.items():
            g = ref.run(x[row, pos:pos + n])
            whole[row].append(g)
            got, state = gains[row]
            assert np.array_equal(got.view(np.uint32), g.view(np.uint32)), (cut, row, pos)
            p, hold, opn, u = ref.trace[-1]
            assert (np.float32(state[0]).view(np.uint32), state[1], state[2], state[3]) == (np.float32(p).view(np.uint32), hold, opn, u), (cut, row, pos)
        pos += n
    for row, ref in refs.items():
        G.assert_covered(ref, np.concatenate(whole[row]), ("row", row))


def test_set_change_remove_and_park_in_the_book(exe):
    """The entry count goes up and down with set, park and retire; a start closed begins at the floor; new constants keep the state
    with hold = min(hold, H); a removal retires after exactly attackSamples samples with u == U, however the calls are cut; a set call
    during the tail re-arms the gate on the kept state; refused constants name their field."""
    x = _signal()[:, :1400]
    p0, p1 = G.params(floorGain=0.1), G.params(floorGain=0.1, holdSamples=7, attackSamples=48, openPower=2e-3)
    prog = Program(exe)
    refs = {0: G.GateRef(p0, False), 1: G.GateRef(p0, True), 2: G.GateRef(p0, True)}
    prog.set(0, p0, False)
    prog.set(1, p0, True)
    prog.set(2, p0, True)
    script = [("X", 0, 100), ("S", 1, p1), ("X", 100, 420), ("L", 2), ("X", 420, 800), ("R", 0), ("R", 1), ("X", 800, 810), ("X", 810, 831), ("S", 1, p0), ("X", 831, 832),
              ("X", 832, 1000), ("bad",), ("X", 1000, 1400)]
    for step in script:
        if step[0] == "X":
            prog.call(x[:, step[1]:step[2]])
        elif step[0] == "S":
            prog.set(step[1], step[2])
        elif step[0] == "L":
            prog.leave(step[1])
        elif step[0] == "R":
            prog.remove(step[1])
        else:
            prog.set(3, G.params(detectorCoeff=0.0))
    answers = prog.run()
    assert [a[1] for a in answers[:3]] == [1, 2, 3]
    answers = answers[3:]
    live = {0, 1, 2}
    for step, ans in zip(script, answers):
        if step[0] == "X":
            gains, e = ans
            xs = x[:, step[1]:step[2]]
            assert set(gains) == live, step
            for row in sorted(live):
                g = refs[row].run(xs[row])
                assert np.array_equal(gains[row][0].view(np.uint32), g.view(np.uint32)), (step, row)
                assert gains[row][1][1:] == refs[row].trace[-1][1:], (step, row)
                if refs[row].retired:
                    assert gains[row][1][3] == G.U
                    live.discard(row)
            assert e[1] == len(live), step
        elif step[0] == "S":
            refs[step[1]].set(step[2])
            assert ans[1] == len(live) and ans[2][step[1]] == 1
        elif step[0] == "L":
            live.discard(step[1])
            assert ans[1] == len(live) and ans[2][step[1]] == 0
        elif step[0] == "R":
            refs[step[1]].remove()
            assert ans[1] == len(live) and ans[2][step[1]] == 0, "a gate that is being taken away counts as an entry, not as a gate"
        else:
            assert ans == ("!", "detectorCoeff must lie in (0, 1]")
    # row 0 (attackSamples 32) was removed at sample 800: an entry through the call that holds sample 831, gone behind it;
    # row 1 (attackSamples 48 by then) was re-armed at 831 and is still there
    assert live == {1}
    assert refs[0].retired and len(refs[0].trace) == 832
    assert refs[0].trace[0][3] == 0 and np.float32(refs[0].gain_of(0)) == np.float32(0.1), "started closed: at the floor"
