"""CPU-side tests of the mix stage (NA_BatchEnableMixStage / GetMixInfo / SetMixGroup / ClearMixGroup / GetStreamMix / MixRampRemaining,
NA_MixGainsFromPan): the binding list, the header and the export split, the contract's lines word for word, the pan helper, what the
calls do where there is no device, and csrc/mix_stage.h -- the step functions and the host book the kernels and the batch are built on
-- run without a device (tests/mix_cases.cpp) against the numpy float32 restatement (tests/mix_cases.py) for equality.  Everything that
runs on the device is in tests/test_gpu_mix.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import mix_cases as M
import na_oracle as O

STAGE = ["NA_BatchEnableMixStage", "NA_BatchGetMixInfo", "NA_BatchSetMixGroup", "NA_BatchClearMixGroup", "NA_BatchGetStreamMix",
         "NA_BatchMixRampRemaining", "NA_MixGainsFromPan"]
HOOKS = ["NA_DebugMixLaunches", "NA_DebugMixStashLaunches", "NA_DebugRunMixStage"]
F = np.float32


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    return neuralaudio_amd


def test_the_mix_stage_is_bound_declared_and_exported(na):
    """The seven calls are public: in capi.NA_SYMBOLS, declared outside the header's test-build block and exported by the library the
    tests load; the hooks are declared inside that block; Batch has the methods and the package the pan helper; the header holds the
    contract's lines word for word, the chain with the mix at its end and what is not provided, and csrc/mix_stage.h repeats the lines."""
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
    for method in ("EnableMixStage", "GetMixInfo", "SetMixGroup", "ClearMixGroup", "GetStreamMix", "MixRampRemaining"):
        assert callable(getattr(na.Batch, method))
    assert "mix_gains_from_pan" in na.__all__ and callable(na.mix_gains_from_pan)
    kernel_header = open(os.path.join(O.ROOT, "neuralaudio_amd", "csrc", "mix_stage.h")).read()
    for text in M.CONTRACT:
        assert text in public, text
        assert text in kernel_header, text
    for text in (M.NOT_ENABLED, "model -> gate -> EQ -> cabinet -> output gain -> mix", "NA_MIX_TAP_OUT", "NA_MIX_TAP_DRY", "#define NA_MIX_MAX_MEMBERS 8",
                 "reads that sample from all M sources before it writes any of the D outputs", "starts from the identity matrix", "Rows are not sanitised",
                 "comb filter", "NA_Multi*", "one-stream NeuralModel", "latency-compensated dry taps"):
        assert text in public, text
    assert [name for name, _ in capi.NA_MixInfo._fields_] == ["maxMembers", "numGroups", "drySamples", "deviceBytes"]
    assert C.sizeof(capi.NA_MixInfo) == 24
    assert (capi.NA_MIX_MAX_MEMBERS, capi.NA_MIX_TAP_OUT, capi.NA_MIX_TAP_DRY) == (M.MAX_MEMBERS, M.OUT, M.DRY)


def test_the_release_library_exports_the_calls_and_not_the_hooks():
    """make release: the public calls are in the dynamic symbol table of dist/libNeuralAudioCAPI.so, the hooks are not."""
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
    info = capi.NA_MixInfo()
    ids, taps, D = (C.c_int * 8)(0, 1), (C.c_int * 8)(), C.c_int(0)
    g = (C.c_float * 64)(1.0, 0.0, 0.0, 1.0)
    calls = [(lambda: lib.NA_BatchEnableMixStage(None), lambda rc: rc != 0),
             (lambda: lib.NA_BatchGetMixInfo(None, C.byref(info)), lambda rc: rc != 0),
             (lambda: lib.NA_BatchSetMixGroup(None, ids, None, 2, 2, g, 0), lambda rc: rc != 0),
             (lambda: lib.NA_BatchSetMixGroup(None, ids, taps, 2, 1, g, 64), lambda rc: rc != 0),
             (lambda: lib.NA_BatchClearMixGroup(None, 0), lambda rc: rc != 0),
             (lambda: lib.NA_BatchGetStreamMix(None, 0, ids, taps, 8, C.byref(D), g), lambda rc: rc < 0),
             (lambda: lib.NA_BatchMixRampRemaining(None, 0), lambda rc: rc < 0)]
    for call, failed in calls:
        assert failed(call())
        assert "no HIP device" in capi.last_error()


# ---- the pan helper ----

def test_pan_ends_are_exact_and_the_centre_is_within_an_ulp(na):
    """pan = -1: exactly (level, 0); pan = +1: exactly (0, level); pan = 0: sqrt(1/2) * level on both sides to 1 ulp of float32;
    left^2 + right^2 = level^2 across the range to float32's precision."""
    for db in (0.0, -6.0, 3.5, -40.0):
        level = 10.0 ** (db / 20.0)
        assert na.mix_gains_from_pan(db, -1.0) == (float(F(level)), 0.0)
        assert na.mix_gains_from_pan(db, 1.0) == (0.0, float(F(level)))
        left, right = na.mix_gains_from_pan(db, 0.0)
        want = math.sqrt(0.5) * level
        for got in (left, right):
            assert abs(got - want) <= float(np.spacing(F(want))), (db, got, want)
        for pan in (-0.9, -0.5, -0.25, 0.1, 0.5, 0.75):
            left, right = na.mix_gains_from_pan(db, pan)
            assert F(left) == F(level * math.cos((pan + 1.0) * math.pi / 4.0)) and F(right) == F(level * math.sin((pan + 1.0) * math.pi / 4.0))
            assert abs(left * left + right * right - level * level) <= 4e-7 * level * level
    assert na.mix_gains_from_pan(0.0, -1.0) == (1.0, 0.0)


def test_pan_refuses_what_is_not_a_pan(na):
    for db, pan, what in ((0.0, 1.0000001, "pan must lie in [-1, 1]"), (0.0, -1.5, "pan must lie in [-1, 1]"), (float("nan"), 0.0, "finite"),
                          (0.0, float("nan"), "finite"), (float("inf"), 0.0, "finite"), (0.0, float("-inf"), "finite")):
        with pytest.raises(na.NeuralAudioError, match=re.escape(what)):
            na.mix_gains_from_pan(db, pan)
    from neuralaudio_amd import capi
    assert capi.load_library().NA_MixGainsFromPan(0.0, 0.0, None, None) != 0


# ---- the restatement itself ----

def test_the_restatement_keeps_its_own_properties():
    """Identity passes bits (NaN payload, Inf, -0 included); a NaN row at gain 0 stays out; no member: +0.0; the ramp's last sample
    and everything behind it is the target; a gain sequence has no step larger than one ramp increment (+ the rounding of one sum)."""
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((4, 40)).astype(F)
    rows[1, :6] = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-42], F)
    rows[3, :] = np.nan
    ref = M.MixRef([1, 2], np.eye(2, dtype=F))
    assert M.same_bits(ref.run(rows), rows)
    ref = M.MixRef([2, 3], [[1.0, 0.0]], D=1)
    assert M.same_bits(ref.run(rows), rows)
    ref = M.MixRef([2, 0], [[0.0, -0.0]], D=1)
    out = ref.run(rows)
    assert not np.any(M.bits(out[2])) and M.same_bits(out[[0, 1, 3]], rows[[0, 1, 3]])
    g = M.gain_at(np.array([[0.25]], F), np.array([[-2.0]], F), 7, np.arange(10))[:, 0, 0]
    assert np.all(g[6:] == F(-2.0)) and g[0] == F(0.25) + F(-2.25) * F(np.float64(1) / np.float64(7))
    # (a gain carries three roundings, each within half an ulp of a value <= 2.25: two neighbours differ by the increment + 4 ulp at most)
    assert np.max(np.abs(np.diff(np.concatenate([[F(0.25)], g])))) <= 2.25 / 7 + 4 * float(np.spacing(F(2.25)))


# ---- csrc/mix_stage.h without a device ----

@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("mix") / "mix_cases"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(O.ROOT, "neuralaudio_amd", "csrc"),
                    os.path.join(O.ROOT, "tests", "mix_cases.cpp"), "-o", str(path)], check=True)
    return path


def _hex(a):
    return " ".join("%08x" % v for v in M.bits(a).ravel())


def _rows_of(lines, rows, n):
    return np.array([[int(h, 16) for h in line.split()] for line in lines], np.uint32).reshape(rows, n).view(F)


class Scenario:
    """The same scenario on the C++ book (a script for tests/mix_cases.cpp) and on the restatement."""

    def __init__(self, rows):
        self.rows, self.script, self.refs, self.dirty, self.expect = rows, ["resize %d" % rows], {}, set(), []

    def group_of(self, s):
        return next((g for g, ref in self.refs.items() if s in ref.streams), None)

    def set(self, streams, gains, D, taps=None, R=0):
        taps = [M.OUT] * len(streams) if taps is None else list(taps)
        g = np.asarray(gains, F).reshape(D, len(streams))
        self.script.append("set %d %d %d %s %s" % (len(streams), D, R, " ".join("%d %d" % st for st in zip(streams, taps)), _hex(g)))
        first = streams[0]
        ref = self.refs.get(first)
        if ref is not None and (ref.streams, ref.taps, ref.D) == (list(streams), taps, D):
            ref.set(g, R)
        else:
            assert all(self.group_of(s) is None for s in streams)
            self.refs[first] = M.MixRef(streams, g, D, taps, R)
        self.dirty.add(first)

    def drop(self, how, s):
        self.script.append("%s %d" % (how, s))
        g = self.group_of(s)
        if g is not None:
            del self.refs[g]
            self.dirty.discard(g)

    def call(self, y, x):
        n = y.shape[1]
        self.script.append("call %d" % n)
        self.script += [_hex(r) for r in y] + [_hex(r) for r in x]
        entries, sets = [], 0
        for g in sorted(self.refs):
            ref = self.refs[g]
            rows = ref.streams + [-1] * (8 - ref.M)
            mask = sum(1 << j for j, t in enumerate(ref.taps) if t == M.DRY)
            entries.append("entry %d %d %d %d %s %d %d" % (ref.M, ref.D, ref.R, ref.k, " ".join(map(str, rows)), mask, sets if g in self.dirty else -1))
            sets += g in self.dirty
        units = len(entries) + 8 * sets if entries else 0
        out = M.run_groups([self.refs[g] for g in sorted(self.refs)], y, x)
        self.dirty.clear()
        self.expect.append((entries, units, out))

    def state(self, s):
        self.script.append("state %d" % s)
        g = self.group_of(s)
        dry = any(M.DRY in ref.taps for ref in self.refs.values())
        self.expect.append("state %d %d %d %d" % (-1 if g is None else g, len(self.refs), int(dry), self.refs[g].remaining() if g is not None else 0))

    def check(self, exe):
        out = subprocess.run([str(exe)], input="\n".join(self.script) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        i = 0
        for step, want in enumerate(self.expect):
            if isinstance(want, str):
                assert out[i] == want, (step, out[i], want)
                i += 1
                continue
            entries, units, rows = want
            assert out[i:i + len(entries)] == entries, (step, out[i:i + len(entries)], entries)
            i += len(entries)
            assert out[i] == "units %d" % units, (step, out[i], units)
            got = _rows_of(out[i + 1:i + 1 + self.rows], self.rows, rows.shape[1])
            assert M.same_bits(got, rows), (step, int(np.count_nonzero(M.bits(got) != M.bits(rows))))
            i += 1 + self.rows
        assert i == len(out)


def test_book_and_step_functions_equal_the_restatement(exe):
    """mix_stage.h compiles on its own (g++, -Wall -Werror) and agrees with the restatement: entries, units and every output bit,
    through set, ramp, set during a ramp, a gain change with R = 0, clear, leave and a new group on the freed rows -- calls cut
    1 / 15 / 17 / 64 / 129, rows with NaN / Inf / -0, members in descending order, a DRY member, 8 members, gains of mixed sign."""
    rows = 12
    rng = np.random.default_rng(11)
    sc = Scenario(rows)
    cuts = [1, 15, 17, 64, 129] * 3

    def data(n):
        y, x = rng.standard_normal((rows, n)).astype(F), rng.standard_normal((rows, n)).astype(F)
        y[7, :min(n, 4)] = np.array([np.nan, np.inf, -0.0, -np.inf], F)[:min(n, 4)]
        return y, x

    sc.call(*data(5))                                                              # no group: nothing
    sc.set([5, 2], [[0.7, -0.4], [0.2, 1.5]], 2, R=100)                            # descending rows, a new group ramps from the identity
    sc.set([9, 0, 4, 9], [[0.5, -0.25, 2.0, 0.125]], 1, taps=[0, 0, 0, 1], R=0)    # interleaved, a DRY member of its own output
    sc.state(2)
    for i, n in enumerate(cuts):
        if i == 3:
            sc.set([5, 2], [[-1.0, 0.0], [0.0, 3.0]], 2, R=50)                     # during the ramp (k = 33 of 100): from the reached gains
            sc.state(5)
        if i == 4:
            sc.set([9, 0, 4, 9], [[0.0, 1.0, 0.0, -1.0]], 1, taps=[0, 0, 0, 1], R=7)
        if i == 6:
            sc.set([5, 2], np.eye(2), 2, R=0)                                      # a step to the identity: rows pass bit for bit
            sc.set([7, 6], [[1.0, 0.0]], 1, R=0)                                   # the NaN row alone at 1: passes; 6 never touched
        if i == 8:
            sc.drop("clear", 2)
            sc.drop("leave", 4)
            sc.drop("clear", 11)                                                   # in no group: nothing
            sc.state(9)
        if i == 9:
            sc.set([11, 10, 9, 8, 5, 4, 2, 0], rng.standard_normal((8, 8)), 8, R=129)
        if i == 11:
            sc.set([11, 10, 9, 8, 5, 4, 2, 0], rng.standard_normal((8, 8)), 8, R=1)
        if i == 13:
            sc.drop("leave", 8)
            sc.set([3, 1], [[0.0, 0.0]], 1, R=2)                                   # to nothing: +0.0 from the second sample on
        sc.call(*data(n))
        if i in (2, 5, 12):
            sc.state(5)
    sc.check(exe)


def test_the_cut_into_calls_never_shows_in_the_book(exe):
    """One ramp of 200 and a set call at sample 77, in one piece per stretch and cut ragged: the same bits."""
    rows, total = 4, 400
    rng = np.random.default_rng(12)
    y, x = rng.standard_normal((rows, total)).astype(F), rng.standard_normal((rows, total)).astype(F)
    outs = []
    for cuts in ([77, 323], [1, 15, 17, 44, 64, 129, 130], [77] + [1] * 23 + [300]):
        assert sum(cuts) == total and 77 in np.cumsum(cuts)
        sc = Scenario(rows)
        sc.set([3, 0, 1], [[0.5, -0.5, 0.25], [1.0, 1.0, -2.0]], 2, taps=[0, 0, 1], R=200)
        pos = 0
        for n in cuts:
            if pos == 77:
                sc.set([3, 0, 1], [[-0.75, 0.3, 0.0], [0.0, 0.1, 1.0]], 2, taps=[0, 0, 1], R=128)
            sc.call(y[:, pos:pos + n], x[:, pos:pos + n])
            pos += n
        sc.check(exe)
        outs.append(np.concatenate([e[2] for e in sc.expect], axis=1))
    assert M.same_bits(outs[0], outs[1]) and M.same_bits(outs[0], outs[2])
