"""CPU-side tests of the meter stage (NA_BatchEnableMeterStage / GetMeterInfo / SetStreamMeter / GetStreamMeter / ReadStreamMeter): the
binding list, the header and the export split, the params check, what the calls do where there is no device, and csrc/meter_stage.h --
the sample / merge / fold functions and the host book the kernels and the batch are built on -- run without a device
(tests/meter_cases.cpp) against the numpy restatement of the contract (tests/meter_cases.py), bit for bit.  Everything that runs on the
device is in tests/test_gpu_meter.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import meter_cases as M
import na_oracle as O

STAGE = ["NA_BatchEnableMeterStage", "NA_BatchGetMeterInfo", "NA_BatchSetStreamMeter", "NA_BatchGetStreamMeter", "NA_BatchReadStreamMeter"]
HOOKS = ["NA_DebugMeterLaunches"]
ROWS = 4


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    return neuralaudio_amd


def test_the_meter_stage_is_bound_declared_and_exported(na):
    """The five calls are public: in capi.NA_SYMBOLS, declared outside the header's test-build block and exported by the library the
    tests load; the hook is declared inside that block; Batch has the methods; the header holds the structs and the contract's lines
    word for word, and csrc/meter_stage.h repeats the lines."""
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
    for method in ("EnableMeterStage", "GetMeterInfo", "SetStreamMeter", "GetStreamMeter", "ReadStreamMeter"):
        assert callable(getattr(na.Batch, method))
    for text in M.STRUCTS + M.CONTRACT + ["sqrt(energy / W) / 2^21", "meter stage not enabled (NA_BatchEnableMeterStage)"]:
        assert text in public, text
    kernel_header = open(os.path.join(O.ROOT, "neuralaudio_amd", "csrc", "meter_stage.h")).read()
    for text in M.CONTRACT:
        assert text in kernel_header, text
    assert [name for name, _ in capi.NA_MeterParams._fields_] == list(M.FIELDS)
    assert [name for name, _ in capi.NA_MeterTap._fields_] == list(M.TAP) + ["reserved"]
    assert [name for name, _ in capi.NA_MeterReading._fields_] == ["windows", "in_", "out", "gateGainMin", "gateGainLast", "windowSamples", "reserved"]
    assert [name for name, _ in capi.NA_MeterInfo._fields_] == ["numMeters", "deviceBytes"]
    assert (C.sizeof(capi.NA_MeterTap), C.sizeof(capi.NA_MeterReading), C.sizeof(capi.NA_MeterInfo)) == (32, 88, 16)


def test_the_release_library_exports_the_calls_and_not_the_hook():
    """make release: the five public calls are in the dynamic symbol table of dist/libNeuralAudioCAPI.so, the hook is not."""
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
    info, p, r = capi.NA_MeterInfo(), capi.NA_MeterParams(), capi.NA_MeterReading()
    calls = [(lambda: lib.NA_BatchEnableMeterStage(None), lambda rc: rc != 0),
             (lambda: lib.NA_BatchGetMeterInfo(None, C.byref(info)), lambda rc: rc != 0),
             (lambda: lib.NA_BatchSetStreamMeter(None, 0, C.byref(p)), lambda rc: rc != 0),
             (lambda: lib.NA_BatchSetStreamMeter(None, 0, None), lambda rc: rc != 0),
             (lambda: lib.NA_BatchGetStreamMeter(None, 0, C.byref(p)), lambda rc: rc < 0),
             (lambda: lib.NA_BatchReadStreamMeter(None, 0, C.byref(r)), lambda rc: rc < 0)]
    for call, failed in calls:
        assert failed(call())
        assert "no HIP device" in capi.last_error()


# ---- csrc/meter_stage.h without a device ----

def _hex(v):
    return "%08x" % M.bits(v)


class Program:
    """builds a script for tests/meter_cases.cpp and parses its answers"""

    def __init__(self, exe):
        self.exe, self.lines, self.kinds = exe, [], []

    def set(self, row, p):
        self.lines.append("S %d %d %s %s" % (row, p["windowSamples"], _hex(p["clipLevelIn"]), _hex(p["clipLevelOut"])))
        self.kinds.append("S")

    def remove(self, row):
        self.lines.append("R %d" % row)
        self.kinds.append("R")

    def leave(self, row):
        self.lines.append("L %d" % row)
        self.kinds.append("L")

    def arrive(self, row, gen, windows):
        self.lines.append("A %d %d %d" % (row, gen, windows))
        self.kinds.append("A")

    def call(self, x, y, g):
        """g: {row: gains}; the other rows are not gated"""
        self.lines.append("X %d" % x.shape[1])
        for block in (x, y):
            self.lines += [" ".join("%08x" % v for v in row.view(np.uint32)) for row in np.ascontiguousarray(block, np.float32)]
        self.lines += [" ".join("%08x" % v for v in np.asarray(g[r], np.float32).view(np.uint32)) if r in g else "-" for r in range(ROWS)]
        self.kinds.append("X")

    def run(self):
        """one answer per command: ("E", entries, [has], [gen]), ("!", text) or ("A", taken); an X answers ({row: reading or None}, E)"""
        out = subprocess.run([str(self.exe)], input="\n".join(self.lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        answers, i = [], 0
        for kind in self.kinds:
            readings = {}
            while out[i].startswith("M "):
                head, tin, tout, tail = [part.split() for part in out[i].split(" | ")]
                tap = lambda w: dict(energy=int(w[0]), oversTotal=int(w[1]), peak=int(w[2], 16), peakHold=int(w[3], 16), overs=int(w[4]))
                readings[int(head[1])] = None if head[2] == "0" else {"windows": int(head[3]), "in": tap(tin), "out": tap(tout), "gateGainMin": int(tail[0], 16),
                                                                     "gateGainLast": int(tail[1], 16), "windowSamples": int(tail[2])}
                i += 1
            if out[i].startswith("!"):
                answers.append(("!", out[i][2:]))
            elif out[i].startswith("A"):
                answers.append(("A", int(out[i].split()[1])))
            else:
                left, right = out[i].split(" | ")
                words = left.split()
                assert words[0] == "E"
                e = ("E", int(words[1]), [int(w) for w in words[2:]], [int(w) for w in right.split()])
                answers.append((readings, e) if kind == "X" else e)
            i += 1
        assert i == len(out)
        return answers


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("meter") / "meter_cases"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(O.ROOT, "neuralaudio_amd", "csrc"),
                    os.path.join(O.ROOT, "tests", "meter_cases.cpp"), "-o", str(path)], check=True)
    return path


def test_the_params_check_names_each_bad_field(exe):
    prog = Program(exe)
    cases = [(dict(window=31), "windowSamples must lie in [32, 32768]"), (dict(window=32769), "windowSamples must lie in [32, 32768]"),
             (dict(clip_in=0.0), "clipLevelIn must be finite and > 0"), (dict(clip_in=np.inf), "clipLevelIn must be finite and > 0"),
             (dict(clip_in=np.nan), "clipLevelIn must be finite and > 0"), (dict(clip_out=-1.0), "clipLevelOut must be finite and > 0"),
             (dict(clip_out=np.nan), "clipLevelOut must be finite and > 0")]
    for change, _ in cases:
        prog.set(0, M.params(**change))
    prog.set(0, M.params(window=32, clip_in=1e-45, clip_out=3e38))
    prog.set(1, M.params(window=32768))
    answers = prog.run()
    assert answers[:len(cases)] == [("!", text) for _, text in cases]
    assert answers[-2][1] == 1 and answers[-1][1] == 2


def _rows(total, seed, clip):
    """[ROWS, total] x 2: noise scaled so that both taps run over `clip`, with the special inputs strewn over rows 0 and 1"""
    rng = np.random.default_rng(seed)
    x = (0.4 * rng.standard_normal((ROWS, total))).astype(np.float32)
    y = (0.6 * rng.standard_normal((ROWS, total))).astype(np.float32)
    sp = M.special_inputs(clip)
    for block, row, offset in ((x, 0, 5), (y, 0, 11), (x, 1, 0), (y, 1, 40)):
        at = offset + 7 * np.arange(len(sp))
        at = at[at < total]
        block[row, at] = sp[:len(at)]
    return x, y


def _cut(total, kind):
    if kind == "ones":
        return [1] * total
    calls, left, i = [], total, 0
    while left > 0:
        n = min([128, 17, 300, 128][i % 4], left)
        calls.append(n)
        left -= n
        i += 1
    return calls


@pytest.mark.parametrize("cut", ["list", "ones"])
def test_the_fold_and_the_book_equal_the_numpy_reference_bit_for_bit(exe, cut):
    """W = 32, 48, 100 and 1024 on four rows over 2300 samples that hold every special input, in cuts of [128, 17, 300, 128] and in cuts
    of 1; rows 1 and 3 are gated.  After every call every reading equals the reference's newest, every field.  First the conditions on
    the inputs: both taps count overs, and the special inputs lie inside completed windows."""
    total = 2300 if cut == "list" else 700
    clip = 0.5
    x, y = _rows(total, 3, clip)
    rng = np.random.default_rng(4)
    g = {1: rng.integers(0, 3, total).astype(np.float32) * np.float32(0.5), 3: rng.random(total).astype(np.float32)}
    windows = {0: 32, 1: 48, 2: 100, 3: 1024}
    refs = {row: M.MeterRef(M.params(W, clip, clip)) for row, W in windows.items()}
    prog = Program(exe)
    for row, W in windows.items():
        prog.set(row, M.params(W, clip, clip))
    calls, pos = _cut(total, cut), 0
    for n in calls:
        prog.call(x[:, pos:pos + n], y[:, pos:pos + n], {r: g[r][pos:pos + n] for r in g})
        pos += n
    answers = prog.run()[ROWS:]
    pos = 0
    for n, (readings, e) in zip(calls, answers):
        assert e[1] == ROWS
        for row, ref in refs.items():
            ref.feed(x[row, pos:pos + n], y[row, pos:pos + n], g[row][pos:pos + n] if row in g else None)
            assert readings[row] == ref.latest(), (cut, row, pos, readings[row], ref.latest())
        pos += n
    for row in (0, 1):
        last = refs[row].latest()
        assert last["in"]["oversTotal"] > 10 and last["out"]["oversTotal"] > 10 and last["in"]["peakHold"] == M.bits(1e18)
    assert refs[1].latest()["gateGainMin"] == 0 and refs[0].latest()["gateGainMin"] == M.bits(1.0)
    if cut == "list":
        assert refs[3].windows == 2 and 0 < refs[3].latest()["gateGainMin"] < M.bits(1.0)


def test_a_full_window_at_the_energy_limit_is_two_to_the_63(exe):
    """W = 32768 of samples >= 8.0 (8, 1e30, inf, 9.5 in turn): energy == 2^63 exactly -- the carry between the two words is right --
    while the peak does not saturate; one sample below 2^-21 adds nothing."""
    W = 32768
    x = np.tile(np.array([8.0, -1e30, np.inf, 9.5], np.float32), W // 4)
    y = x.copy()
    y[4] = 2.0 ** -22
    p = M.params(W, 8.0, 1e18)
    prog = Program(exe)
    prog.set(2, p)
    block = np.zeros((ROWS, W), np.float32)
    xs, ys = block.copy(), block.copy()
    xs[2], ys[2] = x, y
    prog.call(xs[:, :30000], ys[:, :30000], {})
    prog.call(xs[:, 30000:], ys[:, 30000:], {})
    (first, _), (second, _) = prog.run()[1:]
    ref = M.MeterRef(p)
    ref.feed(x, y)
    assert first[2] is None and second[2] == ref.latest()
    assert second[2]["in"]["energy"] == 1 << 63 and second[2]["out"]["energy"] == (1 << 63) - (1 << 48)
    assert second[2]["in"]["peak"] == M.bits(1e18) and second[2]["in"]["overs"] == W and second[2]["out"]["overs"] == W // 2


def test_set_restart_remove_and_leave_in_the_book(exe):
    """set -> restart inside a window -> remove -> set again; leave.  A restart begins at position 0 with holds and totals cleared and
    no reading until its first window completes; every set and every removal gives the row a generation it never had, and a record
    that carries an earlier one -- or no completed window -- is not taken."""
    clip = 0.5
    x, y = _rows(400, 8, clip)
    p = M.params(48, clip, clip)
    prog = Program(exe)
    script = [("S", 0, p), ("S", 1, p), ("X", 0, 100), ("S", 0, p), ("A", 0, 1, 2), ("X", 100, 130), ("X", 130, 160), ("R", 0), ("A", 0, 3, 1),
              ("X", 160, 200), ("S", 0, M.params(32, clip, clip)), ("A", 0, 3, 1), ("A", 0, 5, 0), ("A", 0, 5, 1), ("X", 200, 300), ("L", 1), ("A", 1, 2, 3), ("X", 300, 400)]
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
            prog.call(x[:, step[1]:step[2]], y[:, step[1]:step[2]], {})
    answers = prog.run()
    refs, gens, seen = {}, {0: 0, 1: 0}, []
    for step, ans in zip(script, answers):
        if step[0] == "S":
            refs[step[1]] = M.MeterRef(step[2])
            assert ans[3][step[1]] not in seen and ans[3][step[1]] > gens[step[1]]
        elif step[0] in ("R", "L"):
            refs.pop(step[1], None)
            assert ans[2][step[1]] == 0 and ans[3][step[1]] not in seen
        elif step[0] == "A":
            continue
        else:
            readings, ans = ans
            assert set(readings) == set(refs), step
            for row, ref in refs.items():
                ref.feed(x[row, step[1]:step[2]], y[row, step[1]:step[2]])
                assert readings[row] == ref.latest(), (step, row)
        seen += ans[3]
        gens = {0: ans[3][0], 1: ans[3][1]}
        assert ans[1] == len(refs)
    by_step = dict(zip(range(len(script)), answers))
    # the restart of row 0 at sample 100 (generation 3; 4 inside window 2 of the first meter): nothing until 48 samples have gone by
    assert by_step[5][0][0] is None and by_step[6][0][0]["windows"] == 1 and by_step[6][0][1]["windows"] == 3
    assert by_step[4] == ("A", 0), "a record of the meter before the restart"
    assert by_step[8] == ("A", 0), "a record of a meter that was taken away"
    assert by_step[11] == ("A", 0) and by_step[12] == ("A", 0) and by_step[13] == ("A", 1), "only this meter's generation, only with a completed window"
    assert by_step[16] == ("A", 0), "a parked stream's meter is gone"
