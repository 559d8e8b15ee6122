"""CPU-side tests of the delay stage (NA_DelayParamsFromMs / NA_BatchEnableDelayStage / GetDelayInfo / SetStreamDelay / GetStreamDelay /
StreamDelayFadeRemaining): the binding list, the header, NA_DelayParamsFromMs's arithmetic, what the calls do where there is no device,
and csrc/delay_stage.h -- the step function and the host book the kernel and the batch are built on -- run without a device
(tests/delay_cases.cpp) against the numpy float32 restatement of the contract (tests/delay_cases.py), bit for bit.  Everything that
runs on the device is in tests/test_gpu_delay.py."""
import ctypes as C
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import delay_cases as D
import na_oracle as O

F = np.float32
STAGE = ["NA_DelayParamsFromMs", "NA_BatchEnableDelayStage", "NA_BatchGetDelayInfo", "NA_BatchSetStreamDelay", "NA_BatchGetStreamDelay",
         "NA_BatchStreamDelayFadeRemaining"]
HOOKS = ["NA_DebugDelayLaunches", "NA_DebugRunDelayStage"]


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    return neuralaudio_amd


def test_the_delay_stage_is_bound_declared_and_exported(na):
    """The calls are public: in capi.NA_SYMBOLS, declared outside the header's test-build block and exported by the library the tests
    load; the two hooks are declared inside that block; Batch has the methods; the struct layouts match; the header and delay_stage.h
    hold the step's lines word for word."""
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
    for method in ("EnableDelayStage", "GetDelayInfo", "SetStreamDelay", "GetStreamDelay", "StreamDelayFadeRemaining"):
        assert callable(getattr(na.Batch, method))
    assert callable(na.delay_params_from_ms)
    assert ("typedef struct NA_DelayParams { int delaySamples; float feedback, lowpassCoeff, highpassCoeff, wet, dry; } NA_DelayParams;") in public
    assert "typedef struct NA_DelayInfo   { int maxDelaySamples, ringSamples, pieceSamples, numDelays; long long deviceBytes; } NA_DelayInfo;" in public
    for text in D.STEP + ["no FMA\n * contraction", "model -> gate -> EQ -> cabinet -> delay -> reverb -> output gain -> mix",
                          "fl(g_A + fl(fl(g_B - g_A) * wk))", "fl(fl(fl(1 - wk) * w[t - D_A]) + fl(wk * w[t - D_B]))", "f32 subnormals are kept",
                          "delay stage not enabled (NA_BatchEnableDelayStage)", "fractional or modulated delay times", "ping-pong across rows",
                          "tempo helpers", "512 MB for 1024 rows"]:
        assert text in public, text
    kernel_header = open(os.path.join(O.ROOT, "neuralaudio_amd", "csrc", "delay_stage.h")).read()
    for text in D.STEP:
        assert text in kernel_header, text
    assert [name for name, _ in capi.NA_DelayParams._fields_] == list(D.FIELDS)
    assert [t for _, t in capi.NA_DelayParams._fields_] == [C.c_int] + [C.c_float] * 5 and C.sizeof(capi.NA_DelayParams) == 24
    assert [name for name, _ in capi.NA_DelayInfo._fields_] == ["maxDelaySamples", "ringSamples", "pieceSamples", "numDelays", "deviceBytes"]
    assert C.sizeof(capi.NA_DelayInfo) == 24 and capi.NA_DelayInfo.deviceBytes.offset == 16


def test_the_release_library_exports_the_calls_and_not_the_hooks():
    """make release: the six public calls are in the dynamic symbol table of dist/libNeuralAudioCAPI.so, the hooks are not."""
    subprocess.run(["make", "-C", os.path.join(O.ROOT, "neuralaudio_amd", "csrc"), "-j8", "release"], check=True, capture_output=True)
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(O.ROOT, "dist", "libNeuralAudioCAPI.so")], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in names.splitlines() if line.strip()}
    for name in STAGE:
        assert name in exported, name
    for name in HOOKS:
        assert name not in exported, name


def test_delay_params_from_ms_matches_its_formulas(na):
    """delaySamples = max(1, round(ms * rate / 1000)); lowpassCoeff = 1 when highCutHz <= 0 or >= rate / 2, else 1 - exp(-2 pi f / rate);
    highpassCoeff = 0 when lowCutHz <= 0, else 1 - exp(-2 pi f / rate); wet, dry = 10^(dB / 20) with -inf -> 0: double, rounded once.
    Every bad field is refused by name."""
    f32 = lambda v: float(F(v))
    for rate, ms, fb, lo, hi, wet, dry in ((48000, 375.0, 0.45, 120.0, 4500.0, -6.0, 0.0), (44100, 0.001, -0.99, 0.0, 0.0, float("-inf"), -3.5),
                                           (96000, 2730.6, 0.0, 20.0, 48000.0, 3.0, float("-inf")), (48000, 12.34, 0.99, -5.0, 23999.0, 0.0, 0.0)):
        p = na.delay_params_from_ms(rate, ms, fb, lo, hi, wet, dry)
        assert p["delaySamples"] == max(1, int(math.floor(ms * rate / 1000.0 + 0.5)))
        assert p["feedback"] == f32(fb)
        assert p["lowpassCoeff"] == (1.0 if hi <= 0 or hi >= rate / 2 else f32(1.0 - math.exp(-2.0 * math.pi * hi / rate)))
        assert p["highpassCoeff"] == (0.0 if lo <= 0 else f32(1.0 - math.exp(-2.0 * math.pi * lo / rate)))
        assert p["wet"] == (0.0 if wet == float("-inf") else f32(10.0 ** (wet / 20.0)))
        assert p["dry"] == (0.0 if dry == float("-inf") else f32(10.0 ** (dry / 20.0)))
    assert na.delay_params_from_ms(48000, 0.0)["delaySamples"] == 1
    good = dict(sample_rate=48000, delay_ms=300.0, feedback=0.4, low_cut_hz=100.0, high_cut_hz=5000.0, wet_db=-6.0, dry_db=0.0)
    for change, field in ((dict(sample_rate=0), "sampleRate must be >= 1"), (dict(delay_ms=6000.0), r"delaySamples must lie in \[1, maxDelaySamples\]"),
                          (dict(delay_ms=float("nan")), "delaySamples"), (dict(delay_ms=-1.0), "delaySamples"),
                          (dict(feedback=1.0), r"feedback must lie in \[-0.99, 0.99\]"), (dict(feedback=float("nan")), "feedback"), (dict(feedback=-1.5), "feedback"),
                          (dict(high_cut_hz=float("inf")), r"lowpassCoeff must lie in \(0, 1\]"), (dict(high_cut_hz=1e-20), "lowpassCoeff"),
                          (dict(low_cut_hz=float("nan")), r"highpassCoeff must lie in \[0, 1\)"), (dict(low_cut_hz=1e9), "highpassCoeff"),
                          (dict(wet_db=float("inf")), "wet must be finite"), (dict(wet_db=121.0), "wet must be finite and at most 1e6"),
                          (dict(dry_db=float("nan")), "dry must be finite"), (dict(dry_db=200.0), "dry must be finite and at most 1e6")):
        args = dict(good)
        args.update(change)
        with pytest.raises(na.NeuralAudioError, match=field):
            na.delay_params_from_ms(**args)


def test_without_a_batch_the_calls_fail_loudly(na):
    """The stage lives in a batch and a batch needs a device: on the batch that does not exist every call fails with the library's
    "no HIP device" error instead of crashing."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    info, p = capi.NA_DelayInfo(), capi.NA_DelayParams()
    calls = [(lambda: lib.NA_BatchEnableDelayStage(None, 48000), lambda rc: rc != 0),
             (lambda: lib.NA_BatchGetDelayInfo(None, C.byref(info)), lambda rc: rc != 0),
             (lambda: lib.NA_BatchSetStreamDelay(None, 0, C.byref(p), 0), lambda rc: rc != 0),
             (lambda: lib.NA_BatchSetStreamDelay(None, 0, None, 0), lambda rc: rc != 0),
             (lambda: lib.NA_BatchGetStreamDelay(None, 0, C.byref(p)), lambda rc: rc < 0),
             (lambda: lib.NA_BatchStreamDelayFadeRemaining(None, 0), lambda rc: rc < 0)]
    for call, failed in calls:
        assert failed(call())
        assert "no HIP device" in capi.last_error()


# ---- csrc/delay_stage.h without a device ----

def _hex(v):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(F(v))))[0]


def _f32(hexes):
    return np.array([int(h, 16) for h in hexes], np.uint32).view(F)


class Program:
    """builds a script for tests/delay_cases.cpp and parses its answers"""
    ROWS = 4

    def __init__(self, exe, max_delay):
        self.exe, self.lines, self.kinds = exe, ["C %d" % max_delay], []

    def set(self, row, p, N=0):
        if p is None:
            self.lines.append("N %d %d" % (row, N))
        else:
            self.lines.append("S %d %d %s %s %s %s %s %d" % (row, p["delaySamples"], _hex(p["feedback"]), _hex(p["lowpassCoeff"]), _hex(p["highpassCoeff"]),
                                                             _hex(p["wet"]), _hex(p["dry"]), N))
        self.kinds.append("S")

    def leave(self, row):
        self.lines.append("L %d" % row)
        self.kinds.append("L")

    def call(self, x):
        self.lines.append("X %d" % x.shape[1])
        self.lines += [" ".join("%08x" % v for v in row.view(np.uint32)) for row in np.ascontiguousarray(x, F)]
        self.kinds.append("X")

    def run(self):
        """one answer per command: ("E", entries, [has delay per row], [fade remaining per row]) or ("!", text); an X answers
        (outputs {row: (y, (l, q))}, E)"""
        out = subprocess.run([str(self.exe)], input="\n".join(self.lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        answers, i = [], 0
        for kind in self.kinds:
            rows = {}
            while out[i].startswith("Y "):
                left, right = out[i].split(" | ")
                words = left.split()
                rows[int(words[1])] = (_f32(words[2:]), _f32(right.split()))
                i += 1
            if out[i].startswith("!"):
                answers.append(("!", out[i][2:]))
            else:
                left, right = out[i].split(" | ")
                words = left.split()
                assert words[0] == "E"
                e = ("E", int(words[1]), [int(w) for w in words[2:]], [int(w) for w in right.split()])
                answers.append((rows, e) if kind == "X" else e)
            i += 1
        assert i == len(out)
        return answers


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("delay") / "delay_cases"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(O.ROOT, "neuralaudio_amd", "csrc"),
                    os.path.join(O.ROOT, "tests", "delay_cases.cpp"), "-o", str(path)], check=True)
    return path


def _signal(total, seed):
    x = np.stack([D.noise(total, seed + r) for r in range(Program.ROWS)])
    x[0, 5], x[1, 9], x[2, 11], x[3, 13] = F("nan"), F("inf"), F("-inf"), F(1e30)
    x[0, 17] = F(-0.0)
    return x


def _replay(exe, max_delay, script, x):
    """script: ("X", from, to) | ("S", row, params or None, N) | ("L", row).  The driver and one DelayRef per row run it side by side;
    every output, l and q, the entry count, which rows have a delay and every fade's remainder are compared after every step."""
    prog = Program(exe, max_delay)
    for step in script:
        if step[0] == "X":
            prog.call(x[:, step[1]:step[2]])
        elif step[0] == "S":
            prog.set(step[1], step[2], step[3])
        else:
            prog.leave(step[1])
    answers = prog.run()
    refs = [D.DelayRef() for _ in range(Program.ROWS)]
    for step, ans in zip(script, answers):
        if step[0] == "X":
            rows, e = ans
            live = {r for r in range(Program.ROWS) if refs[r].on}
            assert set(rows) == live, step
            for r in sorted(live):
                y = refs[r].process(x[r, step[1]:step[2]])
                assert D.same_bits(rows[r][0], y), (step, r, D.first_difference(rows[r][0], y))
                if refs[r].on:
                    assert D.same_bits(rows[r][1], np.array([refs[r].l, refs[r].q], F)), (step, r)
        elif step[0] == "S":
            if refs[step[1]].fading():
                assert ans == ("!", "a delay fade of stream %d is running" % step[1]), step
                continue
            refs[step[1]].set(step[2], step[3])
            e = ans
        else:
            refs[step[1]].leave()
            e = ans
        assert e[1] == sum(1 for ref in refs if ref.on), step
        assert e[2] == [1 if ref.target() else 0 for ref in refs], step
        assert e[3] == [ref.remaining() for ref in refs], step
    return refs


@pytest.mark.parametrize("cut", D.CPU_CUTS)
def test_the_step_and_the_book_equal_the_restatement_bit_for_bit(exe, cut):
    """D = 1, 2, 64, 300 on four rows, both filters in the loop, NaN, +-inf, 1e30 and -0 in the input, cut into calls of `cut` samples:
    every output and the filter states behind every call equal the restatement's bits.  6000 samples: the ring of 4096 wraps."""
    total = 6000
    x = _signal(total, 300)
    script = [("S", r, D.filtered(d, feedback=(-0.8 if r == 1 else 0.7)), 0) for r, d in enumerate(D.CPU_DELAYS)]
    script += [("X", pos, min(pos + cut, total)) for pos in range(0, total, cut)]
    refs = _replay(exe, 300, script, x)
    assert all(ref.on and ref.t == total for ref in refs)


def test_set_fade_reset_fade_to_none_and_leave_in_the_book(exe):
    """A delay fades in on an empty line, changes its time with a head cross-fade, changes its mix on one head, is refused a set call
    inside a fade, fades to none and retires with the sample at which the fade ends -- the rest of that call's row is the input's bits --
    and comes back on an empty line although the ring still holds the old one; a parked row loses its delay at once; N = 0 to none
    retires at the set call.  Cuts fall inside every fade."""
    x = _signal(5000, 400)
    a, b = D.filtered(300, 0.7), D.params(64, -0.5, 0.5, 0.0, 0.8, 1.0)
    c = dict(b, wet=0.25, dry=0.5, feedback=0.9)
    script = [("S", 0, a, 100), ("S", 1, a, 0), ("S", 2, b, 1), ("S", 3, None, 50), ("X", 0, 37), ("S", 0, b, 0), ("X", 37, 100), ("X", 100, 101), ("X", 101, 700),
              ("S", 0, b, 257), ("S", 1, D.params(1, 0.99, 1.0, 0.5, -1.0, 0.0), 1000), ("X", 700, 828), ("S", 0, c, 5), ("X", 828, 957), ("X", 957, 1300),
              ("S", 0, c, 600), ("L", 2), ("X", 1300, 2100), ("S", 0, None, 333), ("S", 1, None, 0), ("X", 2100, 2107), ("X", 2107, 2433), ("X", 2433, 2600),
              ("S", 0, a, 0), ("S", 2, D.params(2, 0.5), 64), ("X", 2600, 5000), ("S", 3, dict(a, delaySamples=301), 0), ("S", 3, dict(a, lowpassCoeff=0.0), 0)]
    prog_refs = _replay(exe, 300, script[:-2], x)
    assert prog_refs[0].on and prog_refs[0].t == 2400 and not prog_refs[1].on and prog_refs[2].t == 2400 and not prog_refs[3].on
    prog = Program(exe, 300)
    prog.set(3, dict(a, delaySamples=301))
    prog.set(3, dict(a, lowpassCoeff=0.0))
    prog.set(3, dict(a, highpassCoeff=1.0))
    prog.set(3, dict(a, feedback=0.995))
    prog.set(3, dict(a, wet=float("inf")))
    prog.set(3, dict(a, dry=2e6))
    assert prog.run() == [("!", r"delaySamples must lie in [1, maxDelaySamples]"), ("!", "lowpassCoeff must lie in (0, 1]"), ("!", "highpassCoeff must lie in [0, 1)"),
                          ("!", "feedback must lie in [-0.99, 0.99]"), ("!", "wet must be finite and at most 1e6 in magnitude"),
                          ("!", "dry must be finite and at most 1e6 in magnitude")]


def test_known_answers_of_the_restatement_and_the_header(exe):
    """aL = 1, aH = 0, fb = 0.5, wet = dry = 1, D = 3 on a unit impulse: 1 at 0 and exactly 2^-(m-1) at 3 m; the same line on 2^-120 with
    D = 4 walks through the subnormals to zero; wet = 0, dry = 1 returns x' bit for bit."""
    n = 256
    x = np.zeros((Program.ROWS, n), F)
    x[0, 0], x[1, 0] = 1.0, F(2.0 ** -120)
    x[2] = _signal(n, 500)[0]
    prog = Program(exe, 300)
    prog.set(0, D.params(3, 0.5))
    prog.set(1, D.params(4, 0.5))
    prog.set(2, D.params(5, 0.9, 0.5, 0.1, 0.0, 1.0))
    prog.call(x)
    rows, _ = prog.run()[-1]
    e0 = np.zeros(n, F)
    e0[0] = 1.0
    e0[3::3] = [F(2.0 ** -m) for m in range(len(e0[3::3]))]
    e1 = np.zeros(n, F)
    e1[0] = F(2.0 ** -120)
    e1[4::4] = [F(2.0 ** -(120 + m)) for m in range(len(e1[4::4]))]
    assert 0 < e1[4 * 8] < np.finfo(F).tiny and e1[4 * 30] == F(2.0 ** -149) and e1[4 * 31] == 0.0 and not np.any(e1[4 * 31:])
    for got, e in ((rows[0][0], e0), (rows[1][0], e1), (rows[2][0], D.sanitise(x[2]))):
        assert D.same_bits(got, e), D.first_difference(got, e)
    for row, p in ((0, D.params(3, 0.5)), (1, D.params(4, 0.5))):
        ref = D.DelayRef()
        ref.set(p)
        assert D.same_bits(ref.process(x[row]), rows[row][0])


def test_the_array_path_of_the_restatement_is_the_sample_loop():
    """The restatement computes runs without fade and filters as arrays; a filter coefficient that is one ulp off forces the sample loop.
    With aL = 1 - 2^-24 the bits differ, so the comparison is made on the loop itself: the array path switched off."""
    x = _signal(3000, 600)[0]
    fast, slow = D.DelayRef(), D.DelayRef()
    p = D.params(130, -0.75, 1.0, 0.0, 0.5, 0.25)
    fast.set(p)
    slow.set(p)
    slow._run = None  # (never called: N = 1 << 20 keeps the loop on its fade branch with equal settings)
    slow.set(p, 1 << 20)
    a = np.concatenate([fast.process(x[:7]), fast.process(x[7:])])
    b = slow.process(x)
    assert D.same_bits(a, b), D.first_difference(a, b)
