"""CPU-side tests of the tuner stage (NA_BatchEnableTunerStage / GetTunerInfo / SetStreamTuner / GetStreamTuner / ReadStreamTuner,
NA_TunerParamsFromRange, NA_TunerPitch): the binding list, the header and the export split, the limits, what the calls do where there
is no device, the two host helpers against their Python restatements, and csrc/tuner_stage.h -- the quantiser, the group and lag sums,
the selection and the host book the kernels and the batch are built on -- run without a device (tests/tuner_cases.cpp) against the
numpy restatement of the contract (tests/tuner_cases.py), field for field.  Everything that runs on the device is in
tests/test_gpu_tuner.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import na_oracle as O
import tuner_cases as T

STAGE = ["NA_BatchEnableTunerStage", "NA_BatchGetTunerInfo", "NA_BatchSetStreamTuner", "NA_BatchGetStreamTuner", "NA_BatchReadStreamTuner",
         "NA_TunerParamsFromRange", "NA_TunerPitch"]
HOOKS = ["NA_DebugTunerLaunches"]
ROWS = 4


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    return neuralaudio_amd


def test_the_tuner_stage_is_bound_declared_and_exported(na):
    """The seven calls are public: in capi.NA_SYMBOLS, declared outside the header's test-build block and exported by the library the
    tests load; the hook is declared inside that block; Batch has the methods; the header holds the structs and the contract's lines
    word for word and says what is not provided, and csrc/tuner_stage.h repeats the lines."""
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
    for method in ("EnableTunerStage", "GetTunerInfo", "SetStreamTuner", "GetStreamTuner", "ReadStreamTuner"):
        assert callable(getattr(na.Batch, method))
    for text in T.STRUCTS + T.CONTRACT + [T.NOT_ENABLED, "polyphonic detection", "a tap behind the gate", "note\n * names", "NA_Multi*", "one-stream NeuralModel"]:
        assert text in public, text
    for text in ("/* REAL-TIME SAFE; NULL: the tuner goes at once */", "/* REAL-TIME SAFE; 1 / 0 / < 0 as the meter's */", "/* host arithmetic; 0 when lag == 0 */"):
        assert text in public, text
    kernel_header = open(os.path.join(O.ROOT, "neuralaudio_amd", "csrc", "tuner_stage.h")).read()
    for text in T.CONTRACT:
        assert text in kernel_header, text
    assert [name for name, _ in capi.NA_TunerParams._fields_] == list(T.FIELDS[:7]) + ["reserved", "minEnergy"]
    assert [name for name, _ in capi.NA_TunerReading._fields_] == list(T.READING)
    assert [name for name, _ in capi.NA_TunerInfo._fields_] == ["numTuners", "deviceBytes"]
    assert (C.sizeof(capi.NA_TunerParams), C.sizeof(capi.NA_TunerReading), C.sizeof(capi.NA_TunerInfo)) == (40, 80, 16)


def test_the_release_library_exports_the_calls_and_not_the_hook():
    """make release: the seven public calls are in the dynamic symbol table of dist/libNeuralAudioCAPI.so, the hook is not."""
    subprocess.run(["make", "-C", os.path.join(O.ROOT, "neuralaudio_amd", "csrc"), "-j8", "release"], check=True, capture_output=True)
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(O.ROOT, "dist", "libNeuralAudioCAPI.so")], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in names.splitlines() if line.strip()}
    for name in STAGE:
        assert name in exported, name
    for name in HOOKS:
        assert name not in exported, name


def test_without_a_batch_the_calls_fail_loudly():
    """The stage lives in a batch and a batch needs a device: on the batch that does not exist every call fails with the library's
    "no HIP device" error instead of crashing."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    info, p, r = capi.NA_TunerInfo(), capi.NA_TunerParams(), capi.NA_TunerReading()
    calls = [(lambda: lib.NA_BatchEnableTunerStage(None), lambda rc: rc != 0),
             (lambda: lib.NA_BatchGetTunerInfo(None, C.byref(info)), lambda rc: rc != 0),
             (lambda: lib.NA_BatchSetStreamTuner(None, 0, C.byref(p)), lambda rc: rc != 0),
             (lambda: lib.NA_BatchSetStreamTuner(None, 0, None), lambda rc: rc != 0),
             (lambda: lib.NA_BatchGetStreamTuner(None, 0, C.byref(p)), lambda rc: rc < 0),
             (lambda: lib.NA_BatchReadStreamTuner(None, 0, C.byref(r)), lambda rc: rc < 0)]
    for call, failed in calls:
        assert failed(call())
        assert "no HIP device" in capi.last_error()


# ---- the host helpers ----

def test_params_from_range_equals_its_restatement(na):
    """Guitar, bass, a 44.1 kHz host, a high range that keeps D at 1, and a range whose maxLag would pass 1024: every field equals the
    restatement's (integers), and every result passes the limits."""
    cases = [(48000, 41.2, 1320, 30), (48000, 70, 1400, 50), (44100, 82.4, 660, 20), (96000, 110, 6000, 25), (48000, 27.5, 500, 1000), (48000, 300, 3000.0001, 1.0),
             (192000, 25, 1500, 40), (48000, 5.0, 500, 30), (48000, 20, 20000, 30)]
    seen = set()
    for case in cases:
        want = T.params_from_range(*case)
        if want is None:
            with pytest.raises(na.NeuralAudioError, match="NA_TunerParamsFromRange: .*maxLag above 1024"):
                na.tuner_params_from_range(*case)
            seen.add(None)
            continue
        got = na.tuner_params_from_range(*case)
        assert got == want, (case, got, want)
        seen.add(got["decimation"])
    assert None in seen and {1, 2, 8} <= seen
    assert T.params_from_range(48000, 41.2, 1320, 30) == T.params(2, 1755, 17, 585, 800, 0, 922, 1755 * 66 * 66)
    with pytest.raises(na.NeuralAudioError, match="NA_TunerParamsFromRange"):
        na.tuner_params_from_range(48000, 0.0, 100, 30)


def test_pitch_equals_its_restatement_to_1e_12(na):
    """NA_TunerPitch on readings of the restatement (tones, a sawtooth, a reading at the lag limits) and on made-up ones that hit the
    clamps, the zero denominator and den >= 0: hz and clarity within 1e-12 relative; lag 0 gives 0."""
    readings = []
    for f0 in (82.41, 440.0):
        ref = T.TunerRef(T.params(2, 2048, 2, 640, 1024, 0, 922))
        ref.feed(T.harmonic_tone(f0, 48000.0, 8192, 0.5))
        readings.append(ref.latest())
    ref = T.TunerRef(T.params(1, 256, 2, 130, 400))
    ref.feed(T.sawtooth(800, 50))
    readings.append(ref.latest())
    base = dict(evaluations=3, position=300, e0=1000, decimation=3, lag=40)
    readings += [dict(base, r=[900, 950, 100], e=[1000, 1000, 1000]), dict(base, r=[100, 950, 949], e=[1000, 1000, 0]), dict(base, r=[5, 4, 5], e=[10, 10, 10]),
                 dict(base, r=[1, 2, 1], e=[0, 0, 0], e0=0), dict(base, r=[-(1 << 46), (1 << 46) + 12345, 1 << 45], e=[1 << 46, (1 << 46) + 99999, 1 << 47], e0=(1 << 46) + 7)]
    for r in readings:
        assert r["lag"] > 0
        got, want = na.tuner_pitch(r, 48000.0), T.pitch(r, 48000.0)
        for g, w in zip(got, want):
            assert abs(g - w) <= 1e-12 * abs(w), (r, got, want)
    assert na.tuner_pitch(dict(base, lag=0, r=[0, 0, 0], e=[0, 0, 0]), 48000.0) is None


# ---- csrc/tuner_stage.h without a device ----

class Program:
    """builds a script for tests/tuner_cases.cpp and parses its answers"""

    def __init__(self, exe):
        self.exe, self.lines, self.kinds = exe, [], []

    def set(self, row, p):
        self.lines.append("S %d " % row + " ".join(str(p[name]) for name in T.FIELDS))
        self.kinds.append("S")

    def remove(self, row):
        self.lines.append("R %d" % row)
        self.kinds.append("R")

    def leave(self, row):
        self.lines.append("L %d" % row)
        self.kinds.append("L")

    def arrive(self, row, gen, evaluations):
        self.lines.append("A %d %d %d" % (row, gen, evaluations))
        self.kinds.append("A")

    def call(self, x):
        self.lines.append("X %d" % x.shape[1])
        self.lines += [" ".join("%08x" % v for v in row.view(np.uint32)) for row in np.ascontiguousarray(x, np.float32)]
        self.kinds.append("X")

    def run(self):
        """one answer per command: ("E", entries, [has], [gen]), ("!", text) or ("A", taken); an X answers ({row: reading or None}, E, evaluating)"""
        out = subprocess.run([str(self.exe)], input="\n".join(self.lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        answers, i = [], 0
        for kind in self.kinds:
            readings = {}
            while out[i].startswith("T "):
                w = out[i].split()
                v = [int(t) for t in w[3:]]
                readings[int(w[1])] = None if w[2] == "0" else {"evaluations": v[0], "position": v[1], "lag": v[2], "decimation": v[3], "e0": v[4], "r": v[5:8], "e": v[8:11]}
                i += 1
            if out[i].startswith("!"):
                answers.append(("!", out[i][2:]))
            elif out[i].startswith("A"):
                answers.append(("A", int(out[i].split()[1])))
            else:
                parts = out[i].split(" | ")
                words = parts[0].split()
                assert words[0] == "E"
                e = ("E", int(words[1]), [int(w) for w in words[2:]], [int(w) for w in parts[1].split()])
                answers.append((readings, e, int(parts[2])) if kind == "X" else e)
            i += 1
        assert i == len(out)
        return answers


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("tuner") / "tuner_cases"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(O.ROOT, "neuralaudio_amd", "csrc"),
                    os.path.join(O.ROOT, "tests", "tuner_cases.cpp"), "-o", str(path)], check=True)
    return path


def test_every_limit_is_refused_with_its_field_named(exe):
    prog = Program(exe)
    for change, _ in T.LIMITS:
        prog.set(0, T.params(**change))
    prog.set(0, T.params(1, 32, 2, 4, 16, 15, 512, 0))
    prog.set(1, T.params(8, 2048, 1024, 1024, 65536, 65535, 1024, (1 << 64) - 1))
    answers = prog.run()
    assert answers[:len(T.LIMITS)] == [("!", text) for _, text in T.LIMITS]
    assert answers[-2][1] == 1 and answers[-1][1] == 2


def _run_cases(exe, x, calls, cases):
    """cases in groups of ROWS over the rows of x: after every call every reading equals the restatement's newest; returns the refs"""
    refs_all = []
    for first in range(0, len(cases), ROWS):
        group = cases[first:first + ROWS]
        prog = Program(exe)
        for row, p in enumerate(group):
            prog.set(row, p)
        pos = 0
        for n in calls:
            prog.call(x[:ROWS, pos:pos + n])
            pos += n
        answers = prog.run()[len(group):]
        refs = [T.TunerRef(p) for p in group]
        pos = 0
        for n, (readings, e, evaluating) in zip(calls, answers):
            assert e[1] == len(group)
            ends = 0
            for row, ref in enumerate(refs):
                before = ref.evaluations
                ref.feed(x[row, pos:pos + n])
                ends += ref.evaluations > before
                assert readings[row] == ref.latest(), (calls[:3], row, pos, ref.p, readings[row], ref.latest())
            assert evaluating == ends, "the evaluate launch runs over the entries with an evaluation end in the call, and over no other"
            pos += n
        refs_all += refs
    return refs_all


@pytest.mark.parametrize("cut", list(T.CUTS))
def test_the_header_equals_the_restatement_on_the_gpu_cases(exe, cut):
    """The 24 tuners of the GPU suite -- D 1, 2, 3, 8; (W, maxLag) around one and two waves of lags; H 16, 37, W; phase 0, H - 1 -- over
    its 1200-sample signal with the special inputs, in each of its cuts: every reading after every call, every field.  First the
    conditions on the cases: most of them find a pitch, H = 16 in calls of 333 skips evaluations and counts them."""
    x = T.cut_signal()[[4, 8, 0, 5]]
    refs = _run_cases(exe, x, T.CUTS[cut], T.cut_cases())
    assert sum(ref.latest() is not None for ref in refs) >= 22 and sum(ref.latest() is not None and ref.latest()["lag"] > 0 for ref in refs) >= 12
    if cut == "333":
        skipping = [ref for ref in refs if ref.p["hopSamples"] == 16]
        assert skipping and all(ref.latest()["evaluations"] == ref.evaluations > len(ref.computed()) == 4 for ref in skipping)


@pytest.mark.parametrize("period,decimation", [(50, 1), (50, 2), (37, 1), (96, 3)])
def test_an_integer_sawtooth_lands_on_its_period(exe, period, decimation):
    """W 256, maxLag 130: a sawtooth of period P on the quantiser's grid reads lag P / D, in one call and in calls of 100."""
    p = T.params(decimation, 256, 2, 130, 300, 0, 922)
    total = 400 * decimation
    x = np.stack([T.sawtooth(total, period)] * ROWS)
    for calls in ([total], [100] * (total // 100)):
        ref = _run_cases(exe, x, calls, [p])[0]
        assert ref.latest()["lag"] * decimation == period and ref.latest()["evaluations"] == 1


def test_a_constant_row_silence_and_a_quiet_row_read_lag_0(exe):
    """A constant row has no zero crossing of r, silence and a row below minEnergy fail the energy test: lag 0, r and e zero, e0 kept."""
    total = 600
    x = np.zeros((ROWS, total), np.float32)
    x[0] = 0.25
    x[2] = T.pitched(total, 40.0, 1, level=0.0005, noise=0.0)
    x[3] = T.pitched(total, 40.0, 1, level=0.5, noise=0.0)
    p = T.params(1, 256, 2, 130, 500, 0, 922)
    refs = _run_cases(exe, x, [total], [p] * ROWS)
    for row in (0, 1, 2):
        r = refs[row].latest()
        assert r["lag"] == 0 and r["r"] == [0, 0, 0] and r["e"] == [0, 0, 0] and r["evaluations"] == 1
    assert refs[0].latest()["e0"] == 256 * 8191 ** 2 and refs[1].latest()["e0"] == 0 and 0 < refs[2].latest()["e0"] < p["minEnergy"]
    assert refs[3].latest()["lag"] == 40


def test_a_full_scale_square_at_the_limits(exe):
    """D 8, W 2048, maxLag 1024, a full-scale square of 16 x 500 samples a period (lag 1000): sums next to 2^47 -- e0 = 2048 * (8 * 32767)^2
    -- through a call of several pieces."""
    p = T.params(8, 2048, 2, 1024, 3100, 0, 922)
    total = 8 * 3100 + 5
    sq = np.where((np.arange(total) // 4000) % 2 == 0, np.float32(1.0), np.float32(-1.0)).astype(np.float32)
    x = np.stack([sq, -sq, sq, sq])
    x[1, ::3] = np.inf
    refs = _run_cases(exe, x, [total], [p, p])
    r = refs[0].latest()
    assert r["lag"] == 1000 and r["e0"] == 2048 * (8 * 32767) ** 2 and r["e0"] > 1 << 46 and r["r"][1] == r["e0"]


def test_accuracy_of_the_restatement_and_the_pitch_helper(na):
    """Five-harmonic tones (0.6, 1.0, 0.7, 0.4, 0.3) at the twelve notes from 41.20 to 523.25 Hz, 48 kHz, peaks 0.5 and 0.01, D 2, W 2048,
    minLag 2, maxLag 640, thresholdQ10 922, 8192 samples with the one evaluation at their end: NA_TunerPitch of the restatement's
    reading stays within 0.25 cent of f0 on every case (worst here: 0.083 cent, at 523.25 Hz; below 300 Hz 0.006 cent).  What this
    does not show: the rule picks the peak of r, not of r over its energies, and at a few positions of the window against a low note's
    phase -- 4 of 32 hops of 300 at 41.2 Hz, 1 of 16 at 55 and 61.74 Hz -- that peak lies a sample and a half from the period, the
    parabola's offset clamps at 1 and the reading is 1.2 to 1.6 cent off."""
    p = T.params(2, 2048, 2, 640, 4096, 0, 922)
    worst = 0.0
    for peak in (0.5, 0.01):
        for f0 in T.NOTES:
            ref = T.TunerRef(p)
            ref.feed(T.harmonic_tone(f0, 48000.0, 8192, peak))
            r = ref.latest()
            assert r["lag"] > 0, (f0, peak)
            hz, clarity = na.tuner_pitch(r, 48000.0)
            err = abs(T.cents(hz, f0))
            worst = max(worst, err)
            print("f0 %.2f peak %g: lag %d hz %.4f (%.4f cent) clarity %.4f" % (f0, peak, r["lag"], hz, T.cents(hz, f0), clarity))
            assert err <= 0.25, (f0, peak, hz)
            assert abs(T.cents(T.pitch(r, 48000.0)[0], f0)) <= 0.25
    print("worst error %.4f cent" % worst)


def test_set_restart_remove_and_leave_in_the_book(exe):
    """set -> restart -> remove -> set again; leave.  A restart begins at position 0 -- nothing the earlier tuner took in is read, no
    reading until its first evaluation ends; every set and every removal gives the row a generation it never had, and a record that
    carries an earlier one -- or no evaluation -- is not taken."""
    x = T.cut_signal(1)[:ROWS, :600]
    p = T.params(2, 100, 2, 64, 37, 5)
    prog = Program(exe)
    script = [("S", 0, p), ("S", 1, p), ("X", 0, 101), ("S", 0, p), ("A", 0, 1, 2), ("X", 101, 150), ("X", 150, 201), ("R", 0), ("A", 0, 3, 1),
              ("X", 201, 240), ("S", 0, T.params(3, 32, 2, 4, 16, 0)), ("A", 0, 3, 1), ("A", 0, 5, 0), ("A", 0, 5, 1), ("X", 240, 403), ("L", 1), ("A", 1, 2, 3), ("X", 403, 600)]
    for step in script:
        if step[0] == "S":
            prog.set(step[1], step[2])
        elif step[0] == "R":
            prog.remove(step[1])
        elif step[0] == "L":
            prog.leave(step[1])
        elif step[0] == "A":
            prog.arrive(*step[1:])
        else:
            prog.call(x[:, step[1]:step[2]])
    answers = prog.run()
    refs, gens, seen = {}, {0: 0, 1: 0}, []
    for step, ans in zip(script, answers):
        if step[0] == "S":
            refs[step[1]] = T.TunerRef(step[2])
            assert ans[3][step[1]] not in seen and ans[3][step[1]] > gens[step[1]]
        elif step[0] in ("R", "L"):
            refs.pop(step[1], None)
            assert ans[2][step[1]] == 0 and ans[3][step[1]] not in seen
        elif step[0] == "A":
            continue
        else:
            readings, ans, _ = ans
            assert set(readings) == set(refs), step
            for row, ref in refs.items():
                ref.feed(x[row, step[1]:step[2]])
                assert readings[row] == ref.latest(), (step, row)
        seen += ans[3]
        gens = {0: ans[3][0], 1: ans[3][1]}
        assert ans[1] == len(refs)
    by_step = dict(zip(range(len(script)), answers))
    # the restart of row 0 at sample 101 (an odd position: inside a group of the first tuner): 49 samples hold no evaluation end
    assert by_step[2][0][0]["evaluations"] == 1 and by_step[5][0][0] is None and by_step[6][0][0]["evaluations"] == 1 and by_step[6][0][1]["evaluations"] == 2
    assert by_step[6][0][0]["position"] == 84
    assert by_step[4] == ("A", 0), "a record of the tuner before the restart"
    assert by_step[8] == ("A", 0), "a record of a tuner that was taken away"
    assert by_step[11] == ("A", 0) and by_step[12] == ("A", 0) and by_step[13] == ("A", 1), "only this tuner's generation, only with an evaluation"
    assert by_step[16] == ("A", 0), "a parked stream's tuner is gone"
