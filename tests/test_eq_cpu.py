"""CPU-side tests of the EQ stage (NA_EqSectionFromDesign / NA_BatchEnableEqStage / GetEqInfo / SetStreamEq / GetStreamEq /
StreamEqFadeRemaining): the binding list, the header, the design function's arithmetic and refusals, what the calls do where there is no
device, and csrc/eq_stage.h -- the step function, the parameter check and the host book the kernel and the batch are built on -- run
without a device (tests/eq_cases.cpp) against the Python restatement of the contract (tests/eq_cases.py), bit for bit.  Everything that
runs on the device is in tests/test_gpu_eq.py."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import eq_cases as E
import na_oracle as O

STAGE = ["NA_EqSectionFromDesign", "NA_BatchEnableEqStage", "NA_BatchGetEqInfo", "NA_BatchSetStreamEq", "NA_BatchGetStreamEq",
         "NA_BatchStreamEqFadeRemaining"]
HOOKS = ["NA_DebugEqLaunches", "NA_DebugRunEqStage"]
STEP = ["acc = fl(b0*v); acc = fl(acc + fl(b1*x1)); acc = fl(acc + fl(b2*x2));",
        "acc = fl(acc - fl(a1*y1)); acc = fl(acc - fl(a2*y2));",
        "x2 = x1; x1 = v; y2 = y1; y1 = acc; v = acc",
        "x' = isnan(x) ? 0 : clamp(x, +-1e18f)",
        "fl32(fl32(fl32(1 - w) * o_A) + fl32(w * o_B))"]


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    return neuralaudio_amd


def test_the_eq_stage_is_bound_declared_and_exported(na):
    """The six calls are public: in capi.NA_SYMBOLS, declared outside the header's test-build block and exported by the library the
    tests load; the two hooks are declared inside that block; Batch has the methods; the header holds the step's formulas word for
    word and says what is not provided."""
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
    for method in ("EnableEqStage", "GetEqInfo", "SetStreamEq", "GetStreamEq", "StreamEqFadeRemaining"):
        assert callable(getattr(na.Batch, method))
    assert callable(na.eq_section)
    assert "#define NA_EQ_MAX_SECTIONS 8" in public
    assert "typedef struct NA_EqSection { double b0, b1, b2, a1, a2; } NA_EqSection;" in public
    assert "typedef struct NA_EqInfo { int maxSections, numEntries; long long deviceBytes; } NA_EqInfo;" in public
    for text in STEP + ["no FMA contraction", "subnormals are kept", "the stage on NA_Multi* batches", "the one-stream NeuralModel", "more than 8 sections",
                        "coefficient\n * interpolation"]:
        assert text in public, text
    kernel_header = open(os.path.join(O.ROOT, "neuralaudio_amd", "csrc", "eq_stage.h")).read()
    for text in STEP:
        assert text in kernel_header, text
    assert [name for name, _ in capi.NA_EqSection._fields_] == list(E.FIELDS)
    assert [name for name, _ in capi.NA_EqInfo._fields_] == ["maxSections", "numEntries", "deviceBytes"]
    assert C.sizeof(capi.NA_EqSection) == 40 and capi.NA_EQ_MAX_SECTIONS == E.MAX_SECTIONS


def test_without_a_batch_the_calls_fail_loudly(na):
    """The stage lives in a batch and a batch needs a device: on the batch that does not exist every call fails with the library's
    "no HIP device" error instead of crashing."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    info, sec = capi.NA_EqInfo(), (capi.NA_EqSection * 8)()
    calls = [(lambda: lib.NA_BatchEnableEqStage(None), lambda rc: rc != 0),
             (lambda: lib.NA_BatchGetEqInfo(None, C.byref(info)), lambda rc: rc != 0),
             (lambda: lib.NA_BatchSetStreamEq(None, 0, sec, 3, 0), lambda rc: rc != 0),
             (lambda: lib.NA_BatchSetStreamEq(None, 0, None, 0, 0), lambda rc: rc != 0),
             (lambda: lib.NA_BatchGetStreamEq(None, 0, sec, 8), lambda rc: rc < 0),
             (lambda: lib.NA_BatchStreamEqFadeRemaining(None, 0), lambda rc: rc < 0)]
    for call, failed in calls:
        assert failed(call())
        assert "no HIP device" in capi.last_error()
    assert lib.NA_DebugRunEqStage(None, None, 0, 0) != 0


def test_the_design_function_matches_the_cookbook(na):
    """NA_EqSectionFromDesign against the Python restatement of the RBJ cookbook to 1e-12 relative, five kinds at three rates; every
    design is one the set call would take; every refusal is named."""
    for kind, fs, f, q, db in E.DESIGNS:
        got, want = na.eq_section(kind, fs, f, q, db), E.design(kind, fs, f, q, db)
        for name in E.FIELDS:
            assert abs(got[name] - want[name]) <= 1e-12 * abs(want[name]), (kind, fs, f, name, got[name], want[name])
        assert abs(got["a2"]) < 1.0 and abs(got["a1"]) < 1.0 + got["a2"]
    assert na.eq_section("peaking", 48000, 1000, 1.0, 0.0) == na.eq_section(4, 48000, 1000, 1.0, 0.0)
    flat = na.eq_section(4, 48000, 1000, 1.0, 0.0)
    assert flat["b0"] == 1.0 and flat["b1"] == flat["a1"] and flat["b2"] == flat["a2"], "a peak of 0 dB is the identity"
    nan, inf = float("nan"), float("inf")
    for args, text in (((5, 48000, 1000, 1, 0), "unknown kind"), ((-1, 48000, 1000, 1, 0), "unknown kind"),
                       ((0, nan, 1000, 1, 0), "every argument must be finite"), ((0, 48000, inf, 1, 0), "every argument must be finite"),
                       ((0, 48000, 1000, nan, 0), "every argument must be finite"), ((2, 48000, 1000, 1, -inf), "every argument must be finite"),
                       ((0, 0.0, 1000, 1, 0), "sampleRate must be > 0"), ((0, 48000, 0.0, 1, 0), r"freqHz must lie in \(0, sampleRate / 2\)"),
                       ((0, 48000, 24000.0, 1, 0), r"freqHz must lie in \(0, sampleRate / 2\)"), ((0, 48000, -5.0, 1, 0), r"freqHz must lie in \(0, sampleRate / 2\)"),
                       ((0, 48000, 1000, 0.0, 0), "q must be > 0"), ((0, 48000, 1000, -1.0, 0), "q must be > 0"),
                       ((2, 48000, 1000, 1, 20000.0), "every coefficient must be finite"),
                       ((0, 48000, 1000, 1e-300, 0), r"must be stable \(\|a2\| < 1 and \|a1\| < 1 \+ a2\)")):
        with pytest.raises(na.NeuralAudioError, match="NA_EqSectionFromDesign: " + text):
            na.eq_section(*args)


# ---- csrc/eq_stage.h without a device ----

def _h32(v):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(np.float32(v))))[0]


def _h64(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def _f32(hexes):
    return np.array([int(h, 16) for h in hexes], np.uint32).view(np.float32)


def _f64(hexes):
    return [struct.unpack("<d", struct.pack("<Q", int(h, 16)))[0] for h in hexes]


class Program:
    """builds a script for tests/eq_cases.cpp and parses its answers"""
    ROWS = 4

    def __init__(self, exe):
        self.exe, self.lines, self.kinds = exe, [], []

    def set(self, row, sections, fade=0, count=None):
        sections = sections or []
        words = [_h64(s[name]) for s in sections for name in E.FIELDS]
        self.lines.append("S %d %d %d %s" % (row, fade, len(sections) if count is None else count, " ".join(words)))
        self.kinds.append("S")

    def leave(self, row):
        self.lines.append("L %d" % row)
        self.kinds.append("L")

    def call(self, x):
        self.lines.append("X %d" % x.shape[1])
        self.lines += [" ".join("%08x" % v for v in row.view(np.uint32)) for row in np.ascontiguousarray(x, np.float32)]
        self.kinds.append("X")

    @staticmethod
    def _entries(line):
        head, sections, fades = line.split(" | ")
        assert head.split()[0] == "E"
        return ("E", int(head.split()[1]), [int(w) for w in sections.split()], [int(w) for w in fades.split()])

    def run(self):
        """one answer per command: ("E", entries, [sections per row], [fade remaining per row]) or ("!", text); an X answers
        (rows {row: outputs}, (units, sets), states {row: [[x1 x2 y1 y2] per section]}, E)"""
        out = subprocess.run([str(self.exe)], input="\n".join(self.lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        answers, i = [], 0
        for kind in self.kinds:
            if out[i].startswith("!"):
                answers.append(("!", out[i][2:]))
                i += 1
                continue
            if kind != "X":
                answers.append(self._entries(out[i]))
                i += 1
                continue
            rows, states = {}, {}
            while out[i].startswith("Y "):
                words = out[i].split()
                rows[int(words[1])] = _f32(words[2:])
                i += 1
            assert out[i].startswith("U ")
            upload = tuple(int(w) for w in out[i].split()[1:])
            i += 1
            while out[i].startswith("T "):
                words = out[i].split()
                vals = _f64(words[2:])
                states[int(words[1])] = [vals[k:k + 4] for k in range(0, len(vals), 4)]
                i += 1
            answers.append((rows, upload, states, self._entries(out[i])))
            i += 1
        assert i == len(out)
        return answers


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("eq") / "eq_cases"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(O.ROOT, "neuralaudio_amd", "csrc"),
                    os.path.join(O.ROOT, "tests", "eq_cases.cpp"), "-o", str(path)], check=True)
    return path


def _signal(total, seed=0):
    return np.stack([E.noise(total, 50 * seed + r) for r in range(Program.ROWS)])


def _bits64(values):
    return [struct.pack("<d", float(v)) for v in values]


@pytest.mark.parametrize("cut", ["one", "ragged", "ones"])
def test_the_step_and_the_book_equal_the_restatement_bit_for_bit(exe, cut):
    """Cascades of 1, 3 and 8 sections and a row without one over 700 samples, in one call, in calls of the case list's sizes and in
    calls of one sample: every output and the state of every section behind every call equal the restatement's bits."""
    total = 700
    x = _signal(total, 1)
    calls = {"one": [total], "ragged": E.ragged(total), "ones": [1] * total}[cut]
    prog, refs = Program(exe), {}
    for row, S in enumerate(E.SECTION_COUNTS):
        prog.set(row, E.cascade(S, row))
        refs[row] = E.EqRef()
        refs[row].set(E.cascade(S, row))
    pos = 0
    for n in calls:
        prog.call(x[:, pos:pos + n])
        pos += n
    answers = prog.run()
    assert [a[1] for a in answers[:3]] == [1, 2, 3] and answers[2][2] == [1, 3, 8, 0]
    pos = 0
    for i, (n, (rows, upload, states, e)) in enumerate(zip(calls, answers[3:])):
        assert set(rows) == {0, 1, 2} and e[1] == 3
        assert upload == ((3 + 3 * 5, 3) if i == 0 else (3, 0)), "the coefficients travel once: behind the entries of the first call"
        for row, ref in refs.items():
            want = ref.run(x[row, pos:pos + n])
            assert E.same_bits(rows[row], want), (cut, row, pos)
            assert [_bits64(s) for s in states[row]] == [_bits64(s) for s in ref.state], (cut, row, pos)
        pos += n


def test_set_change_fade_to_flat_and_park_in_the_book(exe):
    """Flat -> EQ with a fade, a coefficient change on kept state (N = 0) to more and to fewer sections, EQ -> EQ with a fade across
    calls, two set calls in front of one call, a set call during a fade refused, a fade to flat that retires the entry, a park that
    drops the state at once: outputs, section counts, fade positions and entry counts are the restatement's."""
    x = _signal(1200, 2)
    c3, c8, c1, c2 = E.cascade(3, 5), E.cascade(8, 6), E.cascade(1, 7), E.cascade(2, 8)
    script = [("S", 0, c3, 5), ("S", 1, c8, 0), ("S", 2, c1, 200), ("X", 0, 3), ("X", 3, 130), ("refused", 2), ("S", 1, c3, 0), ("S", 0, c8, 0), ("X", 130, 300),
              ("X", 300, 301), ("S", 1, c8, 128), ("S", 2, c2, 0), ("S", 2, c8, 1), ("X", 301, 428), ("X", 428, 430),
              ("S", 0, None, 200), ("S", 1, None, 0), ("S", 3, None, 64), ("X", 430, 600), ("L", 2), ("X", 600, 700), ("S", 2, c3, 0), ("X", 700, 1200)]
    prog = Program(exe)
    for step in script:
        if step[0] == "X":
            prog.call(x[:, step[1]:step[2]])
        elif step[0] == "S":
            prog.set(step[1], step[2], step[3])
        elif step[0] == "L":
            prog.leave(step[1])
        else:
            prog.set(step[1], c3, 0)
    class Tracked(E.EqRef):
        """... and which of its cascades' coefficients have not travelled yet: a set per cascade of the next call that is new"""
        new_to = new_from = False

        def set(self, sections, N=0):
            if N > 0:
                self.new_from = self.new_to and bool(self.sec)
            super().set(sections, N)
            self.new_to = bool(self.sec)

        def sets(self):
            return (int(self.new_to) + int(self.fading and self.new_from)) if self.is_entry else 0

    refs = {r: Tracked() for r in range(Program.ROWS)}
    for step, ans in zip(script, prog.run()):
        if step[0] == "X":
            rows, upload, _, e = ans
            live = {r for r, ref in refs.items() if ref.is_entry}
            sets = sum(ref.sets() for ref in refs.values())
            assert set(rows) == live, step
            for r in sorted(live):
                assert E.same_bits(rows[r], refs[r].run(x[r, step[1]:step[2]])), (step, r)
                refs[r].new_to = refs[r].new_from = False
            assert upload == (len(live) + 5 * sets, sets), (step, "an entry per stream with one, and the sets of the set calls since the last call")
            assert e[1] == sum(ref.is_entry for ref in refs.values()), step
            assert e[2] == [len(refs[r].sec) for r in range(4)] and e[3] == [refs[r].remaining for r in range(4)], step
        elif step[0] == "S":
            refs[step[1]].set(step[2], step[3])
            assert ans[0] == "E" and ans[1] == sum(ref.is_entry for ref in refs.values()), step
            assert ans[2][step[1]] == len(step[2] or []) and ans[3][step[1]] == refs[step[1]].remaining, step
        elif step[0] == "L":
            refs[step[1]].leave()
            assert ans[1] == sum(ref.is_entry for ref in refs.values()) and ans[2][step[1]] == 0
        else:
            assert ans == ("!", "an EQ fade is running")
    assert not refs[0].is_entry and not refs[1].is_entry and not refs[3].is_entry and len(refs[2].sec) == 3


def test_the_stability_rule_at_its_edges(exe, na):
    """|a2| < 1 and |a1| < 1 + a2: a2 = +-(1 - 2^-40) passes with an a1 just inside, a2 = +-1 and |a1| = 1 + a2 exactly are refused
    with the section's index; non-finite coefficients, a bad count and a bad fade length are refused by name."""
    eps = 2.0 ** -40
    ok = dict(b0=1.0, b1=0.0, b2=0.0, a1=0.0, a2=0.0)
    good = [dict(ok, a2=1.0 - eps, a1=1.9), dict(ok, a2=1.0 - eps, a1=-(2.0 - 2 * eps)), dict(ok, a2=-(1.0 - eps), a1=eps / 2), dict(ok, a2=-(1.0 - eps), a1=-eps / 2),
            dict(ok, a2=0.25, a1=np.nextafter(1.25, 0.0)), dict(ok, b0=1e300, b1=-1e300, b2=5e-324)]
    bad = [(dict(ok, a2=1.0), "must be stable"), (dict(ok, a2=-1.0), "must be stable"), (dict(ok, a2=1.0 - eps, a1=2.0 - eps), "must be stable"),
           (dict(ok, a2=1.0 - eps, a1=-(2.0 - eps)), "must be stable"), (dict(ok, a2=-(1.0 - eps), a1=eps), "must be stable"),
           (dict(ok, a2=-(1.0 - eps), a1=-eps), "must be stable"), (dict(ok, a2=0.25, a1=1.25), "must be stable"), (dict(ok, a2=-0.5, a1=-0.5), "must be stable"),
           (dict(ok, b1=float("nan")), "every coefficient must be finite"), (dict(ok, a1=float("inf")), "every coefficient must be finite"),
           (dict(ok, a2=float("nan")), "every coefficient must be finite"), (dict(ok, b0=float("-inf")), "every coefficient must be finite")]
    prog = Program(exe)
    for s in good:
        prog.set(0, [ok, s])
    for s, _ in bad:
        prog.set(1, [ok, ok, s])
    prog.set(2, [ok] * 9)
    prog.set(2, [], count=-1)
    prog.set(2, [ok], fade=(1 << 20) + 1)
    prog.set(2, [ok], fade=-1)
    prog.set(2, [ok] * 8, fade=1 << 20)
    answers = prog.run()
    for ans in answers[:len(good)]:
        assert ans[0] == "E" and ans[2][0] == 2, ans
    for (_, text), ans in zip(bad, answers[len(good):]):
        assert ans[0] == "!" and ans[1].startswith("section 2: ") and text in ans[1], ans
    tail = answers[len(good) + len(bad):]
    assert tail[0] == ("!", "numSections must lie in [0, 8]") and tail[1] == ("!", "numSections must lie in [0, 8]")
    assert tail[2] == ("!", "fadeSamples must lie in [0, 1 << 20]") and tail[3] == ("!", "fadeSamples must lie in [0, 1 << 20]")
    assert tail[4][0] == "E" and tail[4][2][2] == 8 and tail[4][3][2] == 1 << 20


def test_two_known_answers(exe):
    """Independent of the restatement.  {1, 1, 1, 0, 0} on small integers gives exact moving sums.  {1, 0, 0, -0.5, 0} on a unit impulse
    gives exactly 2^-t, down through the f32 subnormals to 2^-149 and then 0, while its f64 state runs on through the f64 subnormals over
    1200 further zero samples to 2^-1074 and then 0: subnormals are kept on both sides.  Bad samples: NaN reads as 0, +-inf as +-1e18."""
    n = 150 + 1200
    x = np.zeros((Program.ROWS, n), np.float32)
    rng = np.random.default_rng(3)
    x[0] = rng.integers(-1000, 1000, n).astype(np.float32)
    x[1, 0] = 1.0
    x[2, :6] = [1.0, np.nan, np.inf, -np.inf, 2.0, 0.5]
    prog = Program(exe)
    prog.set(0, [dict(b0=1.0, b1=1.0, b2=1.0, a1=0.0, a2=0.0)])
    prog.set(1, [dict(b0=1.0, b1=0.0, b2=0.0, a1=-0.5, a2=0.0)])
    prog.set(2, [dict(b0=1.0, b1=0.0, b2=0.0, a1=0.0, a2=0.0)])
    cuts = [0, 100, 149, 150, 151, 1074, 1075, 1076, n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        prog.call(x[:, a:b])
    answers = prog.run()[3:]
    y = {r: np.concatenate([a[0][r] for a in answers]) for r in range(3)}
    padded = np.concatenate([np.zeros(2, np.float32), x[0]])
    assert np.array_equal(y[0], padded[2:] + padded[1:-1] + padded[:-2])
    t = np.arange(n)
    want = np.where(t <= 149, np.ldexp(np.float64(1.0), -np.minimum(t, 149)), 0.0).astype(np.float32)
    assert want[149] == np.float32(1.401298464324817e-45) and want[150] == 0.0
    assert E.same_bits(y[1], want)
    for a, b, ans in zip(cuts[:-1], cuts[1:], answers):
        y1 = ans[2][1][0][2]
        assert y1 == (np.ldexp(1.0, -(b - 1)) if b - 1 <= 1074 else 0.0), (b, y1)
    assert answers[5][2][1][0][2] == 5e-324 and answers[6][2][1][0][2] == 0.0
    assert E.same_bits(y[2][:6], np.array([1.0, 0.0, 1e18, -1e18, 2.0, 0.5], np.float32))
