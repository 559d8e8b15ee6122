"""CPU-side tests of the reverb stage (NA_BatchEnableReverbStage / GetReverbInfo / LoadReverbIR / UnloadReverbIR / SetStreamReverb /
GetStreamReverb / StreamReverbFadeRemaining): the binding list, the header, what the calls do where there is no device, and the float32
restatement the GPU tests check against (tests/reverb_cases.py) held to float64 np.convolve.  Everything that runs on the device is in
tests/test_gpu_reverb.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import na_oracle as O
import reverb_cases as R

STAGE = ["NA_BatchEnableReverbStage", "NA_BatchGetReverbInfo", "NA_BatchLoadReverbIR", "NA_BatchUnloadReverbIR", "NA_BatchSetStreamReverb",
         "NA_BatchGetStreamReverb", "NA_BatchStreamReverbFadeRemaining"]
HOOKS = ["NA_DebugRunReverbStage", "NA_DebugReverbLaunches", "NA_DebugReverbTwiddles"]
CONTRACT = ["W[q] = (cos(2 pi q / 256), -sin(2 pi q / 256))", "(a + bi)(c + di) = (a c - b d) + (a d + b c) i", "four multiplies, one subtract, one add",
            "all 256 complex bins are carried", "p = W[j * 128 / half] * u[bot], u[bot] = u[top] - p, u[top] = u[top] + p",
            "head[t] = sum over k in [0, min(K, 128)) with k <= t of h[k] * x[t - k]", "X_m = F([x block m-1, x block m])",
            "A_b = sum over j in [1, min(J - 1, b)] of H_j * X_{b-j}", "tail[128 b + i] = Re(F'(A_b))[128 + i] * 2^-8",
            "c = head + tail;  y = (dry * x) + (wet * c)", "((1 - w) * y_A) + (w * y_B)", "w = (min(k, N-1) + 1) / N", "f32 subnormals are kept",
            "never contracted into an FMA", "model -> gate -> EQ -> cabinet -> reverb -> output gain -> mix"]


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    return neuralaudio_amd


@pytest.fixture(scope="module")
def tw():
    return R.twiddles_numpy()


def test_the_reverb_stage_is_bound_declared_and_exported(na):
    """The seven calls are public: in capi.NA_SYMBOLS, declared outside the header's test-build block (so
    test_release_library_exports_the_documented_surface_and_nothing_else holds the release library to them) and exported by the
    library the tests load; the three hooks are declared inside that block; Batch has the methods; the contract's formulas are in the
    header comment, word for word."""
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
    for method in ("EnableReverbStage", "ReverbInfo", "LoadReverbIR", "UnloadReverbIR", "SetStreamReverb", "GetStreamReverb", "ReverbFadeRemaining",
                   "DebugRunReverbStage"):
        assert callable(getattr(na.Batch, method))
    assert ("typedef struct NA_ReverbInfo { int maxTaps, partitionSamples, slots, pieceSamples, numIRs; long long deviceBytes; } NA_ReverbInfo;"
            in public)
    for text in CONTRACT:
        assert text in public, text
    for text in ("non-uniform partitions", "stereo IRs", "NA_Multi*", "one-stream NeuralModel", "snapshots of the", "IR file reading or rate conversion",
                 "[1, 131072]"):
        assert text in public[public.index("the reverb stage:"):], text
    fields = [name for name, _ in capi.NA_ReverbInfo._fields_]
    assert fields == ["maxTaps", "partitionSamples", "slots", "pieceSamples", "numIRs", "deviceBytes"]
    assert C.sizeof(capi.NA_ReverbInfo) == 32
    # the kernels' header states the same order and switches contraction off in the step functions themselves
    kernel_header = open(os.path.join(O.ROOT, "neuralaudio_amd", "csrc", "reverb_stage.h")).read()
    assert kernel_header.count("#pragma clang fp contract(off)") >= 6 and "#include <hip" not in kernel_header
    makefile = open(os.path.join(O.ROOT, "neuralaudio_amd", "csrc", "Makefile")).read()
    rule = makefile[makefile.index("$(BUILD)/reverb_stage_kernels.o:"):].split("\n\n")[0]
    assert "$(REC_SLP)" in rule


def test_without_a_batch_the_calls_fail_loudly(na):
    """The stage lives in a batch and a batch needs a device: on the batch that does not exist every call fails with the library's
    "no HIP device" error instead of crashing."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    taps = np.ones(4, np.float32)
    fp = taps.ctypes.data_as(C.POINTER(C.c_float))
    info, wet, dry = capi.NA_ReverbInfo(), C.c_float(), C.c_float()
    calls = [("NA_BatchEnableReverbStage", lambda: lib.NA_BatchEnableReverbStage(None, 48000), lambda rc: rc != 0),
             ("NA_BatchGetReverbInfo", lambda: lib.NA_BatchGetReverbInfo(None, C.byref(info)), lambda rc: rc != 0),
             ("NA_BatchLoadReverbIR", lambda: lib.NA_BatchLoadReverbIR(None, fp, 4), lambda rc: rc < 0),
             ("NA_BatchUnloadReverbIR", lambda: lib.NA_BatchUnloadReverbIR(None, 0), lambda rc: rc != 0),
             ("NA_BatchSetStreamReverb", lambda: lib.NA_BatchSetStreamReverb(None, 0, 0, 0.3, 1.0, 64), lambda rc: rc != 0),
             ("NA_BatchGetStreamReverb", lambda: lib.NA_BatchGetStreamReverb(None, 0, C.byref(wet), C.byref(dry)), lambda rc: rc <= -2),
             ("NA_BatchStreamReverbFadeRemaining", lambda: lib.NA_BatchStreamReverbFadeRemaining(None, 0), lambda rc: rc < 0)]
    assert [name for name, _, _ in calls] == STAGE
    for name, call, failed in calls:
        assert failed(call()), name
        assert capi.last_error().startswith(name + ": null batch") and "no HIP device" in capi.last_error(), (name, capi.last_error())


def test_the_twiddle_table(tw):
    """128 values (cos, -sin) of 2 pi q / 256, rounded once from double: the exact points, the symmetries a rounding keeps, and -- the
    library's table is made the same way by another libm -- at most one f32 ulp from the correctly rounded value (checked against the
    library's own table in tests/test_gpu_reverb.py, and here, where the hook needs no device)."""
    assert tw.dtype == np.float32 and tw.shape == (256,)
    assert tw[0] == 1.0 and tw[1] == 0.0 and tw[2 * 64] == np.float32(np.cos(np.pi / 2)) and tw[2 * 64 + 1] == -1.0
    assert tw[2 * 32] == np.float32(np.sqrt(0.5)) and tw[2 * 32 + 1] == -np.float32(np.sqrt(0.5))
    assert np.all(tw[1::2] <= 0.0) and np.all(np.abs(tw[0::2] ** 2 + tw[1::2] ** 2 - 1.0) < 3e-7)
    lib = R.library_twiddles()
    ulp = np.spacing(np.maximum(np.abs(tw), np.abs(lib)))
    assert np.all(np.abs(lib.astype(np.float64) - tw.astype(np.float64)) <= ulp)


def test_the_transform_is_a_dft(tw):
    """F against numpy's float64 FFT, F' F = 256 * identity, and F of a real delta: the restatement is the transform the contract names."""
    rng = np.random.default_rng(3)
    re, im = rng.standard_normal((4, 256)).astype(np.float32), rng.standard_normal((4, 256)).astype(np.float32)
    fr, fi = R.transform(re, im, tw)
    ref = np.fft.fft(re.astype(np.float64) + 1j * im.astype(np.float64), axis=-1)
    assert np.max(np.abs((fr + 1j * fi) - ref)) < 2e-5 * np.max(np.abs(ref))
    br, bi = R.transform(fr, fi, tw, inverse=True)
    assert np.max(np.abs(br * np.float32(2.0 ** -8) - re)) < 2e-6 and np.max(np.abs(bi * np.float32(2.0 ** -8) - im)) < 2e-6
    d = np.zeros((1, 256), np.float32)
    d[0, 0] = 3.0
    fr, fi = R.transform(d, np.zeros_like(d), tw)
    assert np.all(fr == 3.0) and np.all(fi == 0.0)


def test_a_case_small_enough_to_follow_by_hand(tw):
    """K = 130, 260 samples: a head of 128 taps, one partition of two taps behind it, three blocks.  h = e_0 + 2 e_129: the head is x
    itself, the tail 2 x[t - 129] -- zero in block 0, and integers, so everything is exact."""
    h = np.zeros(130, np.float32)
    h[0], h[129] = 1.0, 2.0
    x = R.integers(np.random.default_rng(4), 260, 8)
    y = R.reverb_f32(h, x, tw)
    expect = x.astype(np.float64)
    expect[129:] += 2.0 * x[:131]
    err = np.abs(y - expect)
    assert np.all(y[:128] == x[:128]), "block 0: no tail yet, the head alone"
    assert np.array_equal(np.rint(y), expect) and err.max() < 1e-4, err.max()
    assert np.array_equal(R.head_f32(h, x), x)
    tail = R.tails_f32(h, x, tw)
    assert tail.shape == (384,) and not np.any(tail[:128]) and np.array_equal(np.rint(tail[:260]), expect - x)
    # wet and dry, and a later start on the same history
    y2 = R.reverb_f32(h, x, tw, wet=0.5, dry=0.25, start=200)
    assert np.allclose(y2, 0.25 * x[200:] + 0.5 * expect[200:], atol=1e-4)
    assert R.same_bits(R.reverb_f32(h, x, tw, start=131), y[131:])


@pytest.mark.parametrize("K,n,seed", [(1000, 3000, 5), (4096, 6000, 6)])
def test_the_restatement_against_float64(tw, K, n, seed):
    """Random normal input, normal taps under an exp(-k / (K/4)) decay: relative RMS error <= 1e-6 against np.convolve in float64 (a
    radix-2 sketch of the contract measured 2.1e-7 and 2.2e-7; the bound leaves a factor of about 4.5 for another butterfly order)."""
    rng = np.random.default_rng(seed)
    h, x = R.decaying(rng, K), rng.standard_normal(n).astype(np.float32)
    err = R.rel_rms(R.reverb_f32(h, x, tw), R.conv64(h, x))
    print("K=%d n=%d: relative rms error %.3g" % (K, n, err))
    assert err <= 1e-6


def test_integer_taps_and_samples(tw):
    """Integer taps in [-4, 4] and samples in [-8, 8], K = 1000, 3000 samples: np.rint(y) equals the exact integers, and the largest
    error is below 0.01 (the sketch showed 2.4e-4)."""
    rng = np.random.default_rng(7)
    h, x = R.integers(rng, 1000, 4), R.integers(rng, 3000, 8)
    y, ref = R.reverb_f32(h, x, tw), R.conv64(h, x)
    print("integers: largest error %.3g" % float(np.max(np.abs(y - ref))))
    assert np.array_equal(np.rint(y), ref) and np.max(np.abs(y - ref)) < 0.01


def test_the_contract_keeps_histories_and_fades(tw):
    """RevContract: a switch of IR continues on the history, to dry and back starts a new T0, a fade blends whole outputs with
    OutStageWeightAt in f32, and the launch count restated."""
    rng = np.random.default_rng(8)
    irs = {"a": R.decaying(rng, 300), "b": R.decaying(rng, 140)}
    x = rng.standard_normal((2, 900)).astype(np.float32)
    c = R.RevContract(2, irs, tw)
    e, exact = c.step(x[:, :100])
    assert R.same_bits(e, x[:, :100]) and list(exact) == [True, True]
    c.set(0, "a", 0.5, 1.0)
    e1, exact = c.step(x[:, 100:400])
    assert list(exact) == [False, True] and R.same_bits(e1[0], R.reverb_f32(irs["a"], x[0, 100:400], tw, 0.5, 1.0))
    c.set(0, "b", 1.0, 0.0)
    e2, _ = c.step(x[:, 400:500])
    assert R.same_bits(e2[0], R.reverb_f32(irs["b"], x[0, 100:500], tw, 1.0, 0.0)[300:])
    c.set(0, None, N=3)
    e3, _ = c.step(x[:, 500:504])
    yb = R.reverb_f32(irs["b"], x[0, 100:504], tw, 1.0, 0.0)[400:]
    w = np.float32(1) / np.float32(3)
    assert e3[0, 0] == (np.float32(1) - w) * yb[0] + w * x[0, 500] and e3[0, 2] == x[0, 502] and e3[0, 3] == x[0, 503]
    assert c.state[0] is None and c.remaining(0) == 0
    c.set(0, "a")
    e4, _ = c.step(x[:, 504:700])
    assert R.same_bits(e4[0], R.reverb_f32(irs["a"], x[0, 504:700], tw)), "a new T0"
    assert list(R.weight32(3, np.arange(5))) == [w, np.float32(2) / np.float32(3), 1.0, 1.0, 1.0]
    # 300 from T0: append, spectrum (blocks 0, 1), tail (blocks 0 .. 2), apply; 1: append, apply; 399: all four
    assert R.expected_launches(0, [300]) == 4 and R.expected_launches(0, [300, 1, 399]) == 10
    assert R.expected_launches(0, [128] * 3) == 12 and R.expected_launches(0, [1] * 128) == 2 * 128 + 2
    assert R.expected_launches(0, [2500]) == 12 and R.expected_launches(5, [10], have=False) == 3
