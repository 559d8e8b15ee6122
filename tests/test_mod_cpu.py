"""CPU-side tests of the modulation stage (NA_ModParamsFromMs / NA_BatchEnableModStage / GetModInfo / SetStreamMod / GetStreamMod /
StreamModFadeRemaining): the binding list, the header, NA_ModParamsFromMs's arithmetic, the two LFO shapes over every value of the
triangle, what the calls do where there is no device, and csrc/mod_stage.h -- the step functions and the host book the kernel and the
batch are built on -- run without a device (tests/mod_cases.cpp, once more under the address and undefined-behaviour sanitizers)
against the numpy float32 restatement of the contract (tests/mod_cases.py), bit for bit.  Everything that runs on the device is in
tests/test_gpu_mod.py."""
import ctypes as C
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import mod_cases as K
import na_oracle as O

F = np.float32
STAGE = ["NA_ModParamsFromMs", "NA_BatchEnableModStage", "NA_BatchGetModInfo", "NA_BatchSetStreamMod", "NA_BatchGetStreamMod", "NA_BatchStreamModFadeRemaining"]
HOOKS = ["NA_DebugRunModStage", "NA_DebugModLaunches"]
PARAMS_TEXT = ("typedef struct NA_ModParams { float baseSamples, depthSamples; unsigned phaseInc; int shape, numVoices;\n"
               "                              unsigned voicePhase[4]; float voiceGain[4]; float feedback, wet, dry, tremoloDepth; } NA_ModParams; /* 68 bytes */")
INFO_TEXT = "typedef struct NA_ModInfo   { int maxDelaySamples, ringSamples, pieceSamples, numMods; long long deviceBytes; } NA_ModInfo;"
# the contract's lines, as include/neuralaudio_amd.h and csrc/mod_stage.h both state them
STEP = ["x'    = isnan(x) ? 0 : clamp(x, +-1e18f)",
        "D   = fl(base + fl(depth * s_v));  Di = (int)D;  fr = fl(D - (float)Di)",
        "a   = w[t - Di];  b = w[t - Di - 1]",
        "tap_v = fl(a + fl(fr * fl(b - a)))",
        "m     = fl(g_0 * tap_0), then m = fl(m + fl(g_v * tap_v)) in voice order",
        "w[t]  = (fb == 0) ? x' : clamp(fl(x' + fl(fb * tap_0)), +-1e30f)",
        "y0    = (wet == 0) ? fl(dry * x') : fl(fl(dry * x') + fl(wet * m))",
        "y     = (td == 0) ? y0 : fl(y0 * fl(1 - fl(td * s_0)))",
        "u_v = phaseAtSet + (unsigned)(k * phaseInc) + voicePhase[v]",
        "h   = (u_v & 0x80000000) ? ~u_v : u_v",
        "tri = fl((float)(h >> 7) * 2^-24)",
        "min(fl(fl(tri * tri) * fl(3 - fl(2 * tri))), 1)",
        "fl(g_A + fl(fl(g_B - g_A) * wk))",
        "s_v = fl(fl(fl(1 - wk) * sA_v) + fl(wk * sB_v))"]


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    return neuralaudio_amd


def test_the_modulation_stage_is_bound_declared_and_exported(na):
    """The six calls are public: in capi.NA_SYMBOLS, declared outside the header's test-build block and exported by the library the
    tests load; the two hooks are declared inside that block; Batch has the methods; the struct layouts match; the header and
    mod_stage.h hold every line of the contract word for word; the chain sentences of the delay and compressor blocks stand."""
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
    for method in ("EnableModStage", "GetModInfo", "SetStreamMod", "GetStreamMod", "StreamModFadeRemaining", "DebugRunModStage"):
        assert callable(getattr(na.Batch, method))
    assert callable(na.mod_params_from_ms) and (na.MOD_TRIANGLE, na.MOD_SINE) == (0, 1)
    assert PARAMS_TEXT in public and INFO_TEXT in public
    assert "#define NA_MOD_TRIANGLE 0" in public and "#define NA_MOD_SINE     1" in public
    kernel_header = open(os.path.join(O.ROOT, "neuralaudio_amd", "csrc", "mod_stage.h")).read()
    for text in STEP:
        assert text in public, text
        assert text in kernel_header, text
    for text in ["no FMA\n * contraction", "subnormals are kept", "model -> gate -> EQ -> cabinet -> compressor -> modulation -> delay -> reverb -> output gain -> mix",
                 "modulation stage not enabled (NA_BatchEnableModStage)", "model -> gate -> EQ -> cabinet -> delay -> reverb -> output gain -> mix",
                 "model -> gate -> EQ -> cabinet -> compressor -> delay -> reverb -> output gain -> mix", "fractional or modulated delay times",
                 "Not provided: the stage on NA_Multi* batches and on the one-stream NeuralModel; more than four voices"]:
        assert text in public, text
    assert "#pragma clang fp contract(off)" in kernel_header and "__host__ __device__" in kernel_header
    assert [name for name, _ in capi.NA_ModParams._fields_] == list(K.FIELDS)
    assert C.sizeof(capi.NA_ModParams) == 68 and capi.NA_ModParams.voicePhase.offset == 20 and capi.NA_ModParams.feedback.offset == 52
    assert [name for name, _ in capi.NA_ModInfo._fields_] == ["maxDelaySamples", "ringSamples", "pieceSamples", "numMods", "deviceBytes"]
    assert C.sizeof(capi.NA_ModInfo) == 24 and capi.NA_ModInfo.deviceBytes.offset == 16


def test_the_release_library_exports_the_calls_and_not_the_hooks():
    """make release: the six public calls are in the dynamic symbol table of dist/libNeuralAudioCAPI.so, the hooks are not."""
    subprocess.run(["make", "-C", os.path.join(O.ROOT, "neuralaudio_amd", "csrc"), "-j8", "release"], check=True, capture_output=True)
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(O.ROOT, "dist", "libNeuralAudioCAPI.so")], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in names.splitlines() if line.strip()}
    for name in STAGE:
        assert name in exported, name
    for name in HOOKS:
        assert name not in exported, name


def test_mod_params_from_ms_matches_double_arithmetic_and_refuses_by_name(na):
    """Three rates, both shapes, one to four voices, -inf dB: every field equals the double formula rounded once.  Every bad field is
    refused by name, the reach beyond the largest line included."""
    inf = float("inf")
    for rate, base, depth, hz, shape, voices, fb, wet, dry, td in ((48000, 7.0, 3.0, 0.8, K.SINE, 3, 0.0, -3.0, 0.0, 0.0), (44100, 1.0, 0.9, 0.25, K.TRIANGLE, 1, 0.7, 0.0, 0.0, 0.0),
                                                                   (96000, 5.0, 0.0, 6.5, K.SINE, 1, 0.0, -inf, 0.0, 0.75), (48000, 20.0, 10.5, 11.0, K.TRIANGLE, 4, -0.95, -6.0, -inf, 1.0),
                                                                   (48000, 4.0, 1.0, 24000.0, K.SINE, 2, 0.3, 20.0, -20.0, 0.0)):
        got = na.mod_params_from_ms(rate, base, depth, hz, shape, voices, fb, wet, dry, td)
        assert got == K.from_ms(rate, base, depth, hz, shape, voices, fb, wet, dry, td), (rate, got)
        assert K.error(got) is None
    p = na.mod_params_from_ms(48000, 7.0, 3.0, 0.8, K.SINE, 3)
    assert p["voicePhase"] == [0, 0x55555555, 0xAAAAAAAA, 0] and p["phaseInc"] == 71583 and p["baseSamples"] == 336.0 and p["depthSamples"] == 144.0
    good = dict(sample_rate=48000, base_ms=7.0, depth_ms=3.0, rate_hz=0.8, shape=K.SINE, voices=3, feedback=0.0, wet_db=0.0, dry_db=0.0, tremolo_depth=0.0)
    nan = float("nan")
    for change, field in ((dict(sample_rate=0), "sampleRate must be >= 1"), (dict(base_ms=0.01), "baseSamples must be finite and at least 2"),
                          (dict(base_ms=nan), "baseSamples must be finite and at least 2"), (dict(depth_ms=-0.1), "depthSamples must be finite and at least 0"),
                          (dict(depth_ms=inf), "depthSamples must be finite and at least 0"), (dict(base_ms=80.0, depth_ms=6.0), "baseSamples \\+ depthSamples must be at most maxDelaySamples - 2"),
                          (dict(rate_hz=-1.0), "rateHz must lie in \\[0, sampleRate / 2\\]"), (dict(rate_hz=24000.5), "rateHz must lie in \\[0, sampleRate / 2\\]"),
                          (dict(rate_hz=nan), "rateHz must lie in \\[0, sampleRate / 2\\]"), (dict(shape=2), "shape must be NA_MOD_TRIANGLE or NA_MOD_SINE"),
                          (dict(voices=0), "numVoices must lie in \\[1, 4\\]"), (dict(voices=5), "numVoices must lie in \\[1, 4\\]"),
                          (dict(feedback=0.96), "feedback must lie in \\[-0.95, 0.95\\]"), (dict(feedback=nan), "feedback must lie in \\[-0.95, 0.95\\]"),
                          (dict(wet_db=121.0), "wet must be finite and at most 1e6 in magnitude"), (dict(wet_db=inf), "wet must be finite and at most 1e6 in magnitude"),
                          (dict(dry_db=nan), "dry must be finite and at most 1e6 in magnitude"), (dict(tremolo_depth=1.5), "tremoloDepth must lie in \\[0, 1\\]"),
                          (dict(tremolo_depth=-0.1), "tremoloDepth must lie in \\[0, 1\\]")):
        args = dict(good)
        args.update(change)
        with pytest.raises(na.NeuralAudioError, match="NA_ModParamsFromMs: " + field):
            na.mod_params_from_ms(**args)


def test_without_a_batch_the_calls_fail_loudly(na):
    """The stage lives in a batch and a batch needs a device: on the batch that does not exist every call fails with the library's
    "no HIP device" error instead of crashing."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    info, p = capi.NA_ModInfo(), capi.NA_ModParams()
    calls = [(lambda: lib.NA_BatchEnableModStage(None, 512), lambda rc: rc != 0),
             (lambda: lib.NA_BatchGetModInfo(None, C.byref(info)), lambda rc: rc != 0),
             (lambda: lib.NA_BatchSetStreamMod(None, 0, C.byref(p), 1), lambda rc: rc != 0),
             (lambda: lib.NA_BatchSetStreamMod(None, 0, None, 1), lambda rc: rc != 0),
             (lambda: lib.NA_BatchGetStreamMod(None, 0, C.byref(p)), lambda rc: rc < 0),
             (lambda: lib.NA_BatchStreamModFadeRemaining(None, 0), lambda rc: rc < 0)]
    for call, failed in calls:
        assert failed(call())
        assert "no HIP device" in capi.last_error()


def test_both_shapes_stay_in_the_unit_interval_for_every_triangle_value():
    """Exhaustive: all 2^24 values of tri = (h >> 7) * 2^-24.  The triangle lies in [0, 1), the smoothstep in [0, 1] before its min --
    so the min never acts and D never leaves [base, base + depth] --, and the phase folds as the contract says.  The
    "sine" against the raised cosine (1 - cos(pi tri)) / 2 in float64: the measured maximum gap is 0.010009 at tri = 0.7215 (and at
    its mirror 0.2785), the figure the header states; the bound is the smoothstep's own, max |3 t^2 - 2 t^3 - (1 - cos(pi t)) / 2| =
    0.0100086 in exact arithmetic, plus four roundings of values below 1."""
    tri = (np.arange(1 << 24, dtype=np.uint32).astype(F) * F(2.0 ** -24)).astype(F)
    assert tri[0] == 0.0 and tri[-1] == F(1.0 - 2.0 ** -24) and np.all(np.diff(tri) > 0)
    raw = ((tri * tri).astype(F) * (F(3.0) - (F(2.0) * tri).astype(F)).astype(F)).astype(F)
    sine = K.shape_of(K.SINE, tri)
    assert raw.min() == 0.0 and raw.max() <= 1.0 and np.array_equal(raw, sine)
    assert sine.min() == 0.0 and sine.max() == 1.0
    assert K.shape_of(K.TRIANGLE, tri) is tri
    gap = np.abs(sine.astype(np.float64) - (1.0 - np.cos(np.pi * tri.astype(np.float64))) / 2.0)
    worst = float(gap.max())
    print("largest gap between the smoothstep and the raised cosine: %.6f at tri = %.4f" % (worst, float(tri[int(gap.argmax())])))
    assert 0.0100 < worst <= 0.0100086 + 4 * 2.0 ** -24 and round(worst, 6) == 0.010009
    # the fold: u and ~u give the same triangle; the top of the ramp is phase 0x7FFFFFFF / 0x80000000
    u = np.array([0, 1, 127, 128, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0xFFFFFF7F, 0x40000000, 0xC0000000], np.uint64)
    assert K.tri_of(u).tolist() == [0.0, 0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24, 0.0, 2.0 ** -24, 0.5, 0.5 - 2.0 ** -24]


# ---- csrc/mod_stage.h without a device ----

def _hex(v):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(np.float32(v))))[0]


def _f32(hexes):
    return np.array([int(h, 16) for h in hexes], np.uint32).view(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Program:
    """builds a script for tests/mod_cases.cpp and parses its answers"""
    ROWS = 4

    def __init__(self, exes, max_delay=K.MAX_DELAY):
        self.exes, self.max_delay, self.lines, self.kinds = exes, max_delay, [], []

    def set(self, row, p, fade=0):
        words = [_hex(p["baseSamples"]), _hex(p["depthSamples"]), str(p["phaseInc"]), str(p["shape"]), str(p["numVoices"])]
        words += [str(v) for v in p["voicePhase"]] + [_hex(g) for g in p["voiceGain"]] + [_hex(p[name]) for name in ("feedback", "wet", "dry", "tremoloDepth")]
        self.lines.append("S %d %d %s" % (row, fade, " ".join(words)))
        self.kinds.append("S")

    def remove(self, row, fade=0):
        self.lines.append("R %d %d" % (row, fade))
        self.kinds.append("R")

    def leave(self, row):
        self.lines.append("L %d" % row)
        self.kinds.append("L")

    def call(self, x):
        self.lines.append("X %d" % x.shape[1])
        self.lines += [" ".join("%08x" % v for v in row.view(np.uint32)) for row in np.ascontiguousarray(x, np.float32)]
        self.kinds.append("X")

    def run(self):
        """one answer per command: ("E", entries, [has per row], [fade remaining per row]) or ("!", text); an X answers ({row: y}, E).
        Every binary -- the plain one and the sanitizer build -- must print the same text."""
        outs = [subprocess.run([str(exe), str(self.max_delay)], input="\n".join(self.lines) + "\n", capture_output=True, text=True) for exe in self.exes]
        for o in outs:
            assert o.returncode == 0 and o.stderr == "", (o.returncode, o.stderr[:2000], o.stdout[-300:])
            assert o.stdout == outs[0].stdout
        out = outs[0].stdout.splitlines()
        answers, i = [], 0
        for kind in self.kinds:
            rows = {}
            while out[i].startswith("Y "):
                words = out[i].split()
                rows[int(words[1])] = _f32(words[2:])
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
def exes(tmp_path_factory):
    """tests/mod_cases.cpp twice: plain, and with -fsanitize=address,undefined (a plain executable: nothing is preloaded)"""
    d = tmp_path_factory.mktemp("mod")
    base = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(O.ROOT, "neuralaudio_amd", "csrc"), os.path.join(O.ROOT, "tests", "mod_cases.cpp")]
    subprocess.run(base + ["-O2", "-o", str(d / "mod_cases")], check=True)
    subprocess.run(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(d / "mod_cases_san")], check=True)
    return [d / "mod_cases", d / "mod_cases_san"]


def _signal(total):
    return np.stack([K.signal(r, total) for r in range(Program.ROWS)])


def _run_script(exes, script, x, max_delay=K.MAX_DELAY):
    """`script`: ("S", row, params, fade[, refusal]) / ("R", row, fade[, refusal]) / ("L", row) / ("X", from, to) / ("bad", params, text).
    Every answer is held against fresh references; returns the references and the counts of refusals and retirements."""
    prog = Program(exes, max_delay)
    for step in script:
        if step[0] == "X":
            prog.call(x[:, step[1]:step[2]])
        elif step[0] == "S":
            prog.set(step[1], step[2], step[3])
        elif step[0] == "R":
            prog.remove(step[1], step[2])
        elif step[0] == "L":
            prog.leave(step[1])
        else:
            prog.set(0, step[1], 0)
    answers = prog.run()
    refs = {row: K.ModRef() for row in range(Program.ROWS)}
    refused = retired = 0
    for step, ans in zip(script, answers):
        if step[0] == "X":
            rows, e = ans
            had = {row for row, r in refs.items() if r.has}
            assert set(rows) == had, step
            for row in had:
                want = refs[row].run(x[row, step[1]:step[2]])
                diff = np.flatnonzero(_bits(rows[row]) != _bits(want))
                assert len(diff) == 0, (step, row, int(diff[0]), float(rows[row][diff[0]]), float(want[diff[0]]))
            retired += len(had - {row for row, r in refs.items() if r.has})
            assert e[1] == sum(1 for r in refs.values() if r.has), step
            assert e[2] == [1 if r.target() is not None else 0 for r in refs.values()], step
            assert e[3] == [r.remaining() for r in refs.values()], step
        elif step[0] in ("S", "R"):
            before = refs[step[1]].remaining()
            ok = refs[step[1]].set(step[2] if step[0] == "S" else None, step[3] if step[0] == "S" else step[2])
            if ok == "fade":
                refused += 1
                assert step[-1] == "fade" and ans == ("!", "fade %d" % before), (step[:2], ans)
            elif ok is not True:
                refused += 1
                assert step[-1] == "phase" and ans == ("!", "phase %d" % ok[1]), (step[:2], ans)
            else:
                assert step[-1] not in ("fade", "phase") and ans[0] == "E" and ans[1] == sum(1 for r in refs.values() if r.has), (step[:2], ans)
                assert ans[3][step[1]] == refs[step[1]].remaining()
        elif step[0] == "L":
            refs[step[1]].leave()
            assert ans[1] == sum(1 for r in refs.values() if r.has) and ans[2][step[1]] == 0
        else:
            assert ans == ("!", step[2]) and K.error(step[1], max_delay) == step[2], (ans, K.error(step[1], max_delay))
    return refs, refused, retired


ROW_PARAMS = [K.chorus(), K.flanger(5.5, 4.25, 0.7), K.params(100.0, 80.5, K.phase_inc(5.0), K.SINE, 2, (0, 0x40000000, 0, 0), [0.5, -0.25, 0, 0], -0.7, 0.9, 0.4, 0.6),
              K.params(24.0, 0.0, K.phase_inc(3.0), K.SINE, 1, wet=0.0, dry=1.0, tremolo=1.0)]


@pytest.mark.parametrize("cut", ["one", "ragged"])
def test_the_step_and_the_book_equal_the_numpy_reference_bit_for_bit(exes, cut):
    """A chorus, two flangers (fb = +-0.7) and a tremolo on four rows over noise with silences, a NaN, infinities and subnormals: in one
    call and in ragged cuts, across a piece's end, every sample equals the reference's bits.  The driver also checks, sample by sample,
    that no tap leaves the entry's reach and no sample reads what its own chunk writes."""
    total = K.PIECE + 300
    x = _signal(total)
    calls = {"one": [total], "ragged": [1, 7, 64, 65, 128, 500, 3, 1283, total - 2051]}[cut]
    assert sum(calls) == total
    script = [("S", row, p, 0) for row, p in enumerate(ROW_PARAMS)]
    pos = 0
    for n in calls:
        script.append(("X", pos, pos + n))
        pos += n
    refs, refused, retired = _run_script(exes, script, x)
    assert refused == 0 and retired == 0 and all(r.has for r in refs.values())


@pytest.mark.parametrize("base,depth", K.FLANGERS)
def test_flangers_at_every_chunk_length(exes, base, depth):
    """fb = +0.7 and -0.7 on two rows at base 2 (the serial extreme: chunks of 1), 5.5 (4), 48 (47), 70 + 30 and 300 + 60 (capped by the
    group's width), and the same settings faded in from none over 100 samples on the other two (the ramp's undershoot of base)."""
    x = _signal(900)
    script = [("S", 0, K.flanger(base, depth, 0.7), 0), ("S", 1, K.flanger(base, depth, -0.7, shape=K.SINE), 0),
              ("S", 2, K.flanger(base, depth, 0.7), 100), ("S", 3, K.flanger(base, depth, -0.7, rate_hz=300.0), 100),
              ("X", 0, 450), ("S", 0, K.flanger(base + 1.75, depth, 0.5), 200), ("X", 450, 900)]
    _run_script(exes, script, x)


@pytest.mark.parametrize("max_delay", [8, 64, 4096])
def test_fades_set_calls_and_retirement_in_the_book(exes, max_delay):
    """None -> A -> B -> none with base, depth, rate and shape changing; a set call during a fade is refused with the samples left; a
    changed voicePhase of a sounding voice is refused, of a silent voice taken; a removal retires with the sample at which its fade
    ends and leaves the rest of that call's row untouched (the reference returns x there); fadeSamples 0 retires at once; park drops
    the entry; a new entry on a retired loud line starts from an empty line.  The bits do not depend on maxDelaySamples: the same
    script runs against the smallest line, a short one (several ring wraps: the ring of maxDelaySamples = 64 is 4096) and the longest."""
    x = _signal(10000)
    with np.errstate(over="ignore"):
        x[0] *= F(1000.0)
    a = K.params(2.5, 1.5, K.phase_inc(40.0), K.TRIANGLE, 2, (0, 0x80000000, 0, 0), [0.75, 0.0, 0, 0], 0.9, 0.8, 1.0)
    b = K.params(3.0, 3.0, K.phase_inc(90.0), K.SINE, 3, (0, 0x12345678, 0x9ABCDEF0, 0), [0.5, 0.5, -0.5, 0], -0.6, 1.0, 0.5, 0.3)
    c = K.params(2.0, 0.0, 0, K.TRIANGLE, 1, wet=1.0, dry=0.0)
    clash = dict(b, voicePhase=[1, 0x12345678, 0x9ABCDEF0, 0])
    script = [("S", 0, a, 100), ("S", 1, b, 0), ("S", 2, c, 1), ("X", 0, 64), ("S", 0, b, 10, "fade"), ("R", 0, 5, "fade"), ("X", 64, 200),
              ("S", 0, b, 300), ("S", 1, clash, 0, "phase"), ("S", 1, dict(a, voicePhase=[0, 77, 0, 0]), 50, "phase"), ("X", 200, 329), ("X", 329, 600), ("S", 1, dict(b, voicePhase=[0, 0x12345678, 5, 9], numVoices=2), 40),
              ("R", 0, 70), ("R", 2, 0), ("X", 600, 650), ("S", 2, a, 0), ("X", 650, 900), ("S", 0, c, 30), ("L", 1), ("X", 900, 4100), ("R", 0, 1), ("X", 4100, 4101),
              ("bad", dict(a, baseSamples=float(F(max_delay - 3.0))), "baseSamples + depthSamples must be at most maxDelaySamples - 2"), ("S", 3, a, 7), ("X", 4101, 10000)]
    refs, refused, retired = _run_script(exes, script, x, max_delay)
    assert refused == 4 and retired == 2, (refused, retired)
    assert [r.has for r in refs.values()] == [False, False, True, True]


def test_refused_constants_name_their_field(exes):
    """every limit of a setting, through the header's own check"""
    good = K.chorus()
    nan, inf = float("nan"), float("inf")
    bad = [(dict(good, baseSamples=1.5), "baseSamples must be finite and at least 2"), (dict(good, baseSamples=nan), "baseSamples must be finite and at least 2"),
           (dict(good, depthSamples=-1.0), "depthSamples must be finite and at least 0"), (dict(good, baseSamples=4000.0), "baseSamples + depthSamples must be at most maxDelaySamples - 2"),
           (dict(good, shape=-1), "shape must be NA_MOD_TRIANGLE or NA_MOD_SINE"), (dict(good, numVoices=0), "numVoices must lie in [1, 4]"), (dict(good, numVoices=5), "numVoices must lie in [1, 4]"),
           (dict(good, voiceGain=[0.1, 0.1, 4.5, 0.0]), "voiceGain[2] must be finite and at most 4 in magnitude"), (dict(good, voiceGain=[0.1, 0.1, 0.1, inf]), "voiceGain[3] must be finite and at most 4 in magnitude"),
           (dict(good, feedback=-0.96), "feedback must lie in [-0.95, 0.95]"), (dict(good, wet=2e6), "wet must be finite and at most 1e6 in magnitude"),
           (dict(good, dry=-inf), "dry must be finite and at most 1e6 in magnitude"), (dict(good, tremoloDepth=1.25), "tremoloDepth must lie in [0, 1]")]
    _run_script(exes, [("bad", p, text) for p, text in bad] + [("S", 0, dict(good, baseSamples=3950.0, depthSamples=144.0), 0)], _signal(4))


def test_the_known_answers(exes):
    """Answers that need no restatement.  depth 0, base 5, one voice of gain 1, wet 1, dry 0, fb 0.5: an impulse of 1 gives 2^-(m-1) at
    5 m, +0 elsewhere, down through the subnormals to the last power of two and then +0.  base 5.5, fb 0: exactly 0.5 at 5 and at 6.
    td 1, wet 0, dry 1 on a constant 1: y = fl(1 - s_0).  wet 0, dry 1, td 0: the row is x' bit for bit."""
    n = 5 * 152
    x = np.zeros((Program.ROWS, n), np.float32)
    x[0, 0] = x[1, 0] = 1.0
    x[2] = 1.0
    x[3] = K.signal(3, n)
    prog = Program(exes)
    prog.set(0, K.params(5.0, 0.0, K.phase_inc(3.0), K.SINE, 1, feedback=0.5, wet=1.0, dry=0.0))
    prog.set(1, K.params(5.5, 0.0, 0, K.TRIANGLE, 1, wet=1.0, dry=0.0))
    prog.set(2, K.params(9.0, 2.0, K.phase_inc(100.0), K.SINE, 1, wet=0.0, dry=1.0, tremolo=1.0))
    prog.set(3, dict(K.chorus(), wet=0.0, dry=1.0))
    prog.call(x)
    rows, _ = prog.run()[4]
    want = np.zeros(n, np.float32)
    m = np.arange(1, 152)
    want[5 * m] = np.ldexp(1.0, -(m - 1)).astype(np.float32)
    assert want[5 * 150] == 2.0 ** -149 and want[5 * 151] == 0.0 and np.count_nonzero(want) == 150
    assert np.array_equal(_bits(rows[0]), _bits(want))
    half = np.zeros(n, np.float32)
    half[5] = half[6] = 0.5
    assert np.array_equal(_bits(rows[1]), _bits(half))
    s0 = K.shape_of(K.SINE, K.tri_of(np.arange(n, dtype=np.uint64) * np.uint64(K.phase_inc(100.0))))
    assert np.array_equal(_bits(rows[2]), _bits((F(1.0) - s0).astype(F))) and rows[2].min() < 0.01 and rows[2].max() == 1.0
    assert np.array_equal(_bits(rows[3]), _bits(K.x_prime(x[3]))) and np.isnan(x[3]).any()
