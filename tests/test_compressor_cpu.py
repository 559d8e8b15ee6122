"""CPU-side tests of the compressor stage (NA_CompressorParamsFromDb / NA_BatchEnableCompressorStage / GetCompressorInfo /
SetStreamCompressor / GetStreamCompressor / StreamCompressorFadeRemaining / StreamCompressorGain): the binding list, the header,
NA_CompressorParamsFromDb's arithmetic and the accuracy of the curve it makes, what the calls do where there is no device, and
csrc/compressor_stage.h -- the step functions and the host book the kernel and the batch are built on -- run without a device
(tests/compressor_cases.cpp, once more under the address and undefined-behaviour sanitizers) against the numpy float32 restatement of
the contract (tests/compressor_cases.py), bit for bit.  Everything that runs on the device is in tests/test_gpu_compressor.py."""
import ctypes as C
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import compressor_cases as K
import handover_cases as H
import na_oracle as O

F = np.float32
STAGE = ["NA_CompressorParamsFromDb", "NA_BatchEnableCompressorStage", "NA_BatchGetCompressorInfo", "NA_BatchSetStreamCompressor",
         "NA_BatchGetStreamCompressor", "NA_BatchStreamCompressorFadeRemaining", "NA_BatchStreamCompressorGain"]
HOOKS = ["NA_DebugCompressorLaunches", "NA_DebugRunCompressorStage"]


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    return neuralaudio_amd


def test_the_compressor_stage_is_bound_declared_and_exported(na):
    """The seven calls are public: in capi.NA_SYMBOLS, declared outside the header's test-build block and exported by the library the
    tests load; the two hooks are declared inside that block; Batch has the methods; the struct layouts match; the header and
    compressor_stage.h hold the struct texts' fields and every line of the step word for word."""
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
    for method in ("EnableCompressorStage", "GetCompressorInfo", "SetStreamCompressor", "GetStreamCompressor", "StreamCompressorFadeRemaining",
                   "StreamCompressorGain", "DebugRunCompressorStage"):
        assert callable(getattr(na.Batch, method))
    assert callable(na.compressor_params_from_db)
    assert "typedef struct NA_CompressorParams { float attackCoeff, releaseCoeff; float curve[513]; } NA_CompressorParams;" in public
    assert "typedef struct NA_CompressorInfo { int curvePoints, numCompressors; long long deviceBytes; } NA_CompressorInfo;" in public
    kernel_header = open(os.path.join(O.ROOT, "neuralaudio_amd", "csrc", "compressor_stage.h")).read()
    for text in K.STEP + ["typedef struct NA_CompressorParams { float attackCoeff, releaseCoeff; float curve[513]; } NA_CompressorParams;",
                          "typedef struct NA_CompressorInfo { int curvePoints, numCompressors; long long deviceBytes; } NA_CompressorInfo;",
                          "every value finite and in [0, 65536]", "Knot i sits at level 2^(-24 + (i >> 4)) * (1 + (i & 15) / 16)",
                          "f32 e (starts at +0) and the last g"]:
        assert text in public, text
        assert text in kernel_header, text
    for text in ["no FMA contraction", "subnormals are kept", "2^(-24 + (i >> 4)) * (1 + (i & 15) / 16)", "e never leaves [0, 2^8), so i + 1 <= 512",
                 "model -> gate -> EQ -> cabinet -> compressor -> delay -> reverb -> output gain -> mix",
                 "compressor stage not enabled (NA_BatchEnableCompressorStage)", "look-ahead", "stereo linking", "side chain"]:
        assert text in public, text
    assert "struct CompParams" in kernel_header and "float attackCoeff = 1.0f, releaseCoeff = 1.0f;" in kernel_header and "float curve[kCompCurvePoints];" in kernel_header
    assert [name for name, _ in capi.NA_CompressorParams._fields_] == ["attackCoeff", "releaseCoeff", "curve"]
    assert C.sizeof(capi.NA_CompressorParams) == 4 * 515 and capi.NA_CompressorParams.curve.offset == 8
    assert [name for name, _ in capi.NA_CompressorInfo._fields_] == ["curvePoints", "numCompressors", "deviceBytes"]
    assert C.sizeof(capi.NA_CompressorInfo) == 16 and capi.NA_CompressorInfo.deviceBytes.offset == 8


def test_the_release_library_exports_the_calls_and_not_the_hooks():
    """make release: the seven public calls are in the dynamic symbol table of dist/libNeuralAudioCAPI.so, the hooks are not."""
    subprocess.run(["make", "-C", os.path.join(O.ROOT, "neuralaudio_amd", "csrc"), "-j8", "release"], check=True, capture_output=True)
    names = subprocess.run(["nm", "-D", "--defined-only", os.path.join(O.ROOT, "dist", "libNeuralAudioCAPI.so")], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in names.splitlines() if line.strip()}
    for name in STAGE:
        assert name in exported, name
    for name in HOOKS:
        assert name not in exported, name


def _design_knot(level, threshold, ratio, knee, makeup):
    """the header's formulas at one level, in Python floats, operation for operation as csrc/compressor_stage.h writes them"""
    o = 20.0 * math.log10(level) - threshold
    s = (0.0 if math.isinf(ratio) else 1.0 / ratio) - 1.0
    if 2.0 * o < -knee:
        G = 0.0
    elif knee > 0.0 and 2.0 * abs(o) <= knee:
        G = s * (o + knee / 2.0) * (o + knee / 2.0) / (2.0 * knee)
    else:
        G = s * o
    return math.pow(10.0, (G + makeup) / 20.0)


def test_compressor_params_from_db_matches_its_formulas(na):
    """Three rates; ratio +inf, knee 0 and a wide knee, attackMs = 0: coefficients 1 - exp(-1 / (ms * rate / 1000)) in double rounded
    once (ms == 0: 1); at every knot the table equals the closed form rounded once.  Every bad field is refused by name."""
    inf = float("inf")
    for rate, thr, ratio, knee, makeup, att, rel in ((48000, -18.0, 4.0, 6.0, 3.0, 5.0, 120.0), (44100, -6.5, inf, 0.0, 0.0, 0.0, 50.0),
                                                     (96000, -30.25, 1.5, 24.0, -2.5, 0.125, 0.0), (48000, -12.0, 1.0, 0.0, 6.0, 1.0, 1.0)):
        p = na.compressor_params_from_db(rate, thr, ratio, knee, makeup, att, rel)
        assert p["attackCoeff"] == float(K.coeff(att, rate)) and p["releaseCoeff"] == float(K.coeff(rel, rate))
        assert (p["attackCoeff"] == 1.0) == (att == 0.0)
        want = np.array([_design_knot(float(l), thr, ratio, knee, makeup) for l in K.LEVELS]).astype(np.float32)
        assert p["curve"].dtype == np.float32 and p["curve"].shape == (K.POINTS,)
        assert np.array_equal(p["curve"], want), (rate, int(np.count_nonzero(p["curve"] != want)))
        # (the vectorised closed form of compressor_cases agrees with the scalar one to a float32 ulp: what the accuracy tests use)
        assert np.allclose(K.closed_form(K.LEVELS, thr, ratio, knee, makeup), want, rtol=2.0 ** -23, atol=0)
    assert np.all(na.compressor_params_from_db(48000, -12.0, 1.0)["curve"] == 1.0), "ratio 1: unity"
    lim = na.compressor_params_from_db(48000, 0.0, inf, 0.0, 0.0, 0.0, 50.0)["curve"]
    assert np.all(lim[:385] == 1.0) and lim[400] == 0.5 and lim[416] == 0.25, "a limiter at 0 dB: 1 up to level 1, 1 / level above"
    good = dict(sample_rate=48000, threshold_db=-18.0, ratio=4.0, knee_db=6.0, makeup_db=0.0, attack_ms=5.0, release_ms=100.0)
    nan = float("nan")
    for change, field in ((dict(sample_rate=0), "sampleRate must be >= 1"), (dict(threshold_db=nan), "thresholdDb must be finite"),
                          (dict(threshold_db=inf), "thresholdDb must be finite"), (dict(ratio=0.5), r"ratio must lie in \[1, \+inf\]"),
                          (dict(ratio=nan), r"ratio must lie in \[1, \+inf\]"), (dict(ratio=-inf), r"ratio must lie in \[1, \+inf\]"),
                          (dict(knee_db=-1.0), "kneeDb must be finite and >= 0"), (dict(knee_db=inf), "kneeDb must be finite and >= 0"),
                          (dict(knee_db=nan), "kneeDb must be finite and >= 0"), (dict(makeup_db=nan), "makeupDb must be finite"),
                          (dict(makeup_db=-inf), "makeupDb must be finite"), (dict(makeup_db=100.0), r"curve\[0\] must lie in \[0, 65536\]"),
                          (dict(attack_ms=-1.0), "attackMs must be finite and >= 0"), (dict(attack_ms=nan), "attackMs must be finite and >= 0"),
                          (dict(release_ms=inf), "releaseMs must be finite and >= 0"), (dict(release_ms=-0.5), "releaseMs must be finite and >= 0"),
                          (dict(release_ms=1e30), r"releaseCoeff must lie in \(0, 1\]")):
        args = dict(good)
        args.update(change)
        with pytest.raises(na.NeuralAudioError, match="NA_CompressorParamsFromDb: " + field):
            na.compressor_params_from_db(**args)


def test_without_a_batch_the_calls_fail_loudly(na):
    """The stage lives in a batch and a batch needs a device: on the batch that does not exist every call fails with the library's
    "no HIP device" error instead of crashing."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    info, p = capi.NA_CompressorInfo(), capi.NA_CompressorParams()
    calls = [(lambda: lib.NA_BatchEnableCompressorStage(None), lambda rc: rc != 0),
             (lambda: lib.NA_BatchGetCompressorInfo(None, C.byref(info)), lambda rc: rc != 0),
             (lambda: lib.NA_BatchSetStreamCompressor(None, 0, C.byref(p), 1), lambda rc: rc != 0),
             (lambda: lib.NA_BatchSetStreamCompressor(None, 0, None, 1), lambda rc: rc != 0),
             (lambda: lib.NA_BatchGetStreamCompressor(None, 0, C.byref(p)), lambda rc: rc < 0),
             (lambda: lib.NA_BatchStreamCompressorFadeRemaining(None, 0), lambda rc: rc < 0),
             (lambda: lib.NA_BatchStreamCompressorGain(None, 0), lambda rc: rc < 0)]
    for call, failed in calls:
        assert failed(call())
        assert "no HIP device" in capi.last_error()


# ---- the accuracy of the table against the closed form (float64: the reference for this number) ----

def _sweep(lo, hi, count):
    """`count` float32 levels, geometrically spaced over [lo, hi]"""
    return np.unique(np.exp(np.linspace(math.log(lo), math.log(hi), count)).astype(np.float32))


ROUNDING = 4 * 2.0 ** -24  # relative: the two knots' own roundings, the product's and the sum's (the difference's is scaled by f * rise / t)


def test_between_knots_a_power_law_is_off_by_the_interpolation_bound_at_most():
    """Away from the knee the static curve is a power law of slope s: level^s times a constant.  Linear interpolation over a segment
    [a, a (1 + h)] is off by at most h^2 / 8 * max|f''| = h^2 / 8 * |s (s - 1)| * a^s relative to ... a^s (1 + h)^s at the least; with
    s in [-1, 0] the exact maximum for s = -1 is h^2 / (4 (1 + h)), below h^2 / 8 * |s (s - 1)| = |s (s - 1)| / 2048 at h = 1 / 16,
    the widest segment.  Asserted on a sweep of 40000 levels per curve over the stretch above the threshold (hard knee: everything
    from one segment above the corner), against the closed form in float64: bound + ROUNDING."""
    worst = {}
    for ratio in (1.5, 2.0, 4.0, 20.0, float("inf")):
        s = (0.0 if math.isinf(ratio) else 1.0 / ratio) - 1.0
        thr = -40.0
        t = K.closed_form(K.LEVELS, thr, ratio, 0.0, 0.0).astype(np.float32)
        lv = _sweep(10.0 ** (thr / 20.0) * (17.0 / 16.0) * 1.0001, 255.0, 40000)
        got = K.curve_at(t, lv).astype(np.float64)
        want = K.closed_form(lv.astype(np.float64), thr, ratio, 0.0, 0.0)
        rel = np.max(np.abs(got / want - 1.0))
        worst[ratio] = rel
        assert rel <= abs(s * (s - 1.0)) / 2048.0 + ROUNDING, (ratio, rel, abs(s * (s - 1.0)) / 2048.0)
        assert rel >= abs(s * (s - 1.0)) / 2048.0 / 4.0, "the sweep is dense enough to see the error it bounds"
    print("largest relative interpolation error per ratio:", {k: "%.3e (%.5f dB)" % (v, 20.0 * math.log10(1.0 + v)) for k, v in worst.items()})
    below = K.curve_at(K.closed_form(K.LEVELS, -40.0, 4.0, 0.0, 6.0).astype(np.float32), _sweep(2.0 ** -30, 10.0 ** (-40.0 / 20.0) * 16.0 / 17.0, 5000))
    assert np.all(below == F(10.0 ** (6.0 / 20.0))), "below the threshold the curve is the makeup gain exactly: equal knots interpolate to themselves"


def test_around_the_knee_the_deviation_stays_below_a_straddled_corner():
    """A segment that straddles a corner of slope change |s| is off by at most |s| * w / 4 dB in the dB / dB plane, w <= 20 log10(17 / 16)
    the segment's width (a chord across a corner, largest with the corner in the middle).  Measured: the largest deviation in dB over
    201 thresholds across one octave (every position of the corner inside a segment), knees 0, 1, 6 and 24 dB, ratios 2, 4 and +inf,
    8000 levels within +-(knee / 2 + 1) dB of each threshold.  The largest value, printed, is the one DESIGN.md 2.19 states
    (0.1283 dB: the limiter with a hard knee, against 0.1317 dB allowed; knee 1 dB: 0.0334 dB; a knee of 6 dB or more adds nothing to
    the power law's 0.0080 dB)."""
    w = 20.0 * math.log10(17.0 / 16.0)
    worst = {}
    for ratio in (2.0, 4.0, float("inf")):
        s = (0.0 if math.isinf(ratio) else 1.0 / ratio) - 1.0
        for knee in (0.0, 1.0, 6.0, 24.0):
            big = 0.0
            for thr in np.linspace(-26.0, -26.0 + 20.0 * math.log10(2.0), 201):
                t = K.closed_form(K.LEVELS, thr, ratio, knee, 0.0).astype(np.float32)
                lv = _sweep(10.0 ** ((thr - knee / 2.0 - 1.0) / 20.0), 10.0 ** ((thr + knee / 2.0 + 1.0) / 20.0), 8000)
                got = K.curve_at(t, lv).astype(np.float64)
                want = K.closed_form(lv.astype(np.float64), thr, ratio, knee, 0.0)
                big = max(big, float(np.max(np.abs(20.0 * np.log10(got / want)))))
            worst[(ratio, knee)] = big
            assert big <= abs(s) * w / 4.0 + 20.0 * math.log10(1.0 + ROUNDING), (ratio, knee, big, abs(s) * w / 4.0)
    print("largest deviation around the knee in dB, (ratio, knee): value:", {k: round(v, 5) for k, v in worst.items()})
    assert worst[(float("inf"), 0.0)] == max(worst.values()) and worst[(float("inf"), 0.0)] > 0.1, "the hard-knee limiter is the worst case, and the sweep finds it"


# ---- csrc/compressor_stage.h without a device ----

def _hex(v):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(np.float32(v))))[0]


def _f32(hexes):
    return np.array([int(h, 16) for h in hexes], np.uint32).view(np.float32)


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


class Program:
    """builds a script for tests/compressor_cases.cpp and parses its answers"""
    ROWS = 4

    def __init__(self, exes):
        self.exes, self.lines, self.kinds = exes, [], []

    def set(self, row, p, fade=0):
        self.lines.append("S %d %d %s %s" % (row, fade, _hex(p["attackCoeff"]), _hex(p["releaseCoeff"])))
        self.lines.append(" ".join("%08x" % v for v in _bits(p["curve"])))
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
        """one answer per command: ("E", entries, [has per row], [fade remaining per row]) or ("!", text); an X answers
        ({row: (g, y, e, last g)}, E).  Every binary -- the plain one and the sanitizer build -- must print the same text."""
        outs = [subprocess.run([str(exe)], input="\n".join(self.lines) + "\n", capture_output=True, text=True, check=True) for exe in self.exes]
        for o in outs:
            assert o.stderr == "", o.stderr[:2000]
            assert o.stdout == outs[0].stdout
        out = outs[0].stdout.splitlines()
        answers, i = [], 0
        for kind in self.kinds:
            rows = {}
            while out[i].startswith("G "):
                left, right = out[i].split(" | ")
                words, st, ys = left.split(), right.split(), out[i + 1].split()
                assert ys[0] == "Y" and ys[1] == words[1]
                rows[int(words[1])] = (_f32(words[2:]), _f32(ys[2:]), _f32(st[:1])[0], _f32(st[1:2])[0])
                i += 2
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
    """tests/compressor_cases.cpp twice: plain, and with -fsanitize=address,undefined (a plain executable: nothing is preloaded)"""
    d = tmp_path_factory.mktemp("compressor")
    base = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(O.ROOT, "neuralaudio_amd", "csrc"),
            os.path.join(O.ROOT, "tests", "compressor_cases.cpp")]
    subprocess.run(base + ["-O2", "-o", str(d / "compressor_cases")], check=True)
    subprocess.run(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(d / "compressor_cases_san")], check=True)
    return [d / "compressor_cases", d / "compressor_cases_san"]


def burst_signal(seed, total, scale=1.0):
    """silence, then noise bursts of different levels between exact silences: the follower rises through the octaves and falls back
    through the subnormals towards zero"""
    rng = np.random.default_rng(9100 + seed)
    x = np.zeros(total, np.float64)
    pos, k = 40, 0
    while pos < total:
        n = [150, 60, 260, 90][k % 4]
        x[pos:pos + n] = [0.5, 4.0, 0.02, 40.0][k % 4] * rng.standard_normal(min(n, total - pos))
        pos += n + [420, 200, 380, 150][k % 4]
        k += 1
    return (scale * x).astype(np.float32)


ROW_PARAMS = [K.params(0.3, 0.25, threshold_db=-30.0, ratio=4.0, knee_db=6.0, makeup_db=3.0),
              K.params(1.0, 0.2, threshold_db=-12.0, ratio=float("inf"), knee_db=0.0),
              K.params(0.01, 0.3, threshold_db=-50.0, ratio=2.0, knee_db=12.0, makeup_db=-1.0),
              K.params(0.7, 0.5, curve=np.linspace(2.0, 0.0, K.POINTS) ** 2)]


def _signal(total=1900):
    return np.stack([burst_signal(r, total) for r in range(Program.ROWS)])


def _check_call(rows, refs, xs, what):
    for row, ref in refs.items():
        if not ref.has:
            assert row not in rows, (what, row)
            continue
        g = ref.run(xs[row])
        got_g, got_y, e, last = rows[row]
        assert np.array_equal(_bits(got_g), _bits(g)), (what, row, int(np.flatnonzero(_bits(got_g) != _bits(g))[0]))
        with np.errstate(invalid="ignore", over="ignore"):
            assert np.array_equal(_bits(got_y), _bits((xs[row] * g).astype(np.float32))), (what, row)
        if len(g):
            assert _bits(e) == _bits(ref.levels[-1][-1]) and _bits(last) == _bits(g[-1]), (what, row)


@pytest.mark.parametrize("cut", ["one", "ragged", "tile"])
def test_the_step_and_the_book_equal_the_numpy_reference_bit_for_bit(exes, cut):
    """Four different compressors on four rows over the burst signal, in one call, in RAGGED cuts and in cuts around a tile's length:
    every gain, every sample out and the state behind every call equal the reference's bits.  First the condition on the inputs: every
    row's reference takes both branches of c, has zero and subnormal levels and levels below knot 0, crosses three octaves of knots and
    has g < 1 on a quarter of its samples."""
    x = _signal()
    refs = {row: K.CompRef() for row in range(Program.ROWS)}
    prog = Program(exes)
    for row, p in enumerate(ROW_PARAMS):
        prog.set(row, p)
        refs[row].set(p, 0)
    calls = {"one": [x.shape[1]], "ragged": H.ragged(x.shape[1]), "tile": [127, 129, 1, 128, 256, 1259]}[cut]
    assert sum(calls) == x.shape[1]
    pos = 0
    for n in calls:
        prog.call(x[:, pos:pos + n])
        pos += n
    answers = prog.run()
    assert [a[1] for a in answers[:4]] == [1, 2, 3, 4]
    pos, gains = 0, {row: [] for row in refs}
    for n, (rows, e) in zip(calls, answers[4:]):
        assert e[1] == 4 and e[2] == [1, 1, 1, 1] and e[3] == [0, 0, 0, 0]
        before = {row: len(ref.levels) for row, ref in refs.items()}
        _check_call(rows, refs, x[:, pos:pos + n], (cut, pos))
        for row in refs:
            gains[row].append(rows[row][0])
            assert len(refs[row].levels) == before[row] + 1
        pos += n
    for row, ref in refs.items():
        K.assert_inputs_reach_every_case(ref, gains[row], ("row", row))


def test_set_change_remove_fades_and_park_in_the_book(exes):
    """The entry count goes up and down with set, park and retire.  A first set call fades in from unity with e = +0; fadeSamples 0
    switches at the next sample, 1 after one sample, 100 ends inside a call, 300 spans three calls; new coefficients act on the kept e;
    a set call during a fade is refused with the samples left; a removal fades to unity and retires with the call that holds the
    fade's last sample (fadeSamples 0: at once); a set call after that starts from e = +0 again; park drops the compressor at once;
    two set calls in front of one call send both curves with one table; refused constants name their field."""
    x = _signal(1500)
    a, b, c, d = ROW_PARAMS
    # "refused": the row is in a fade then -- 172, 172, 128 and 1 samples left (the reference counts them)
    script = [("S", 0, a, 100), ("S", 1, b, 0), ("S", 2, c, 1), ("S", 3, d, 300), ("X", 0, 128), ("S", 0, b, 300), ("S", 3, a, 0, "refused"),
              ("S", 1, K.params(0.05, 0.5, curve=b["curve"]), 0), ("X", 128, 256), ("S", 0, c, 0, "refused"), ("S", 2, a, 300), ("X", 256, 300),
              ("X", 300, 428), ("R", 2, 10, "refused"), ("R", 3, 64), ("R", 1, 0), ("X", 428, 491), ("S", 3, a, 0, "refused"), ("X", 491, 492), ("S", 3, b, 20),
              ("L", 0), ("X", 492, 700), ("S", 1, a, 0), ("S", 1, c, 40), ("X", 700, 900), ("R", 1, 1), ("R", 2, 200), ("X", 900, 901), ("X", 901, 1100),
              ("bad",), ("X", 1100, 1500)]
    prog = Program(exes)
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
            bad = dict(a)
            bad["curve"] = a["curve"].copy()
            bad["curve"][77] = 65537.0
            prog.set(2, bad, 0)
    answers = prog.run()
    refs = {row: K.CompRef() for row in range(Program.ROWS)}
    refused = retired = 0
    for step, ans in zip(script, answers):
        count = sum(1 for r in refs.values() if r.has)
        if step[0] == "X":
            rows, e = ans
            had = {row for row, r in refs.items() if r.has}
            _check_call(rows, refs, x[:, step[1]:step[2]], step)
            retired += len(had - {row for row, r in refs.items() if r.has})
            assert set(rows) == had, step
            assert e[1] == sum(1 for r in refs.values() if r.has), step
            assert e[2] == [1 if (r.has and r.tB is not None) else 0 for r in refs.values()], step
            assert e[3] == [r.remaining() for r in refs.values()], step
        elif step[0] in ("S", "R"):
            ok = refs[step[1]].set(step[2] if step[0] == "S" else None, step[3] if step[0] == "S" else step[2])
            if not ok:
                refused += 1
                assert "refused" in step and ans == ("!", "fade %d" % refs[step[1]].remaining()), (step[:2], ans)
            else:
                assert "refused" not in step and ans[0] == "E" and ans[1] == sum(1 for r in refs.values() if r.has), (step[:2], ans)
                assert ans[3][step[1]] == refs[step[1]].remaining()
        elif step[0] == "L":
            refs[step[1]] = K.CompRef()
            assert ans[1] == count - 1 and ans[2][step[1]] == 0
        else:
            assert ans == ("!", "curve[77] must lie in [0, 65536]")
    assert refused == 4 and retired >= 3, (refused, retired)
    assert [r.has for r in refs.values()] == [False, False, False, True]


def test_the_known_answer(exes):
    """aA = aR = 1, samples from {0, +-0.5, +-2}, t[i] = 1 for i < 384 and 0.25 from knot 384 (level 1.0) on: y is x at |x| = 0.5 and
    exactly x / 4 at |x| = 2 -- an answer that needs no restatement.  And an all-ones curve passes any row bit for bit, NaN, infinities
    and subnormals included."""
    rng = np.random.default_rng(11)
    x = np.zeros((Program.ROWS, 400), np.float32)
    x[0] = rng.choice(np.array([0.0, 0.5, -0.5, 2.0, -2.0], np.float32), 400)
    x[1] = burst_signal(5, 400)
    x[1, 50:60] = [np.nan, np.inf, -np.inf, 1e-40, -1e-45, 300.0, -0.0, 3e38, np.nan, 1.0]
    prog = Program(exes)
    prog.set(0, dict(attackCoeff=1.0, releaseCoeff=1.0, curve=K.known_answer_curve()))
    prog.set(1, dict(attackCoeff=0.3, releaseCoeff=0.1, curve=K.unity_curve()))
    prog.call(x)
    rows, _ = prog.run()[2]
    want = np.where(np.abs(x[0]) == 2.0, x[0] / 4.0, x[0]).astype(np.float32)
    assert np.array_equal(_bits(rows[0][1]), _bits(want)) and {0.5, 2.0} <= set(np.abs(x[0]).tolist())
    assert np.array_equal(_bits(rows[1][1]), _bits(x[1])) and np.all(rows[1][0] == 1.0)
    assert K.knot_level(384) == 1.0 and K.knot_level(368) == 0.5 and K.knot_level(0) == 2.0 ** -24 and K.knot_level(512) == 256.0
