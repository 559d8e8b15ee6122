"""The StdMath WaveNet policy (NA_SetWaveNetMathMode(StdMath): std::tanh instead of the rational FastMath tanh) on every kernel that
implements it: the stage interpreter of the f16-split kernels (which the official tanh architectures fall back to, their specialised
chains refuse the policy), the f32 frame kernel, the 17 .. 64 and the 65 .. 128 channel kernels, and the prewarm kernel that fills the
steady state of all of them (tests/stdmath_cases.py; tests/test_stdmath_cpu.py proves without a GPU that every case lands where it says,
that the cases reach every code site and that each of them tells the two policies apart by more than 100 x its bound).

Every model is built by a loader with SetWaveNetMathMode(StdMath), every oracle is the C oracle with math_mode = MATH_STD, every stream is
prewarmed and every comparison starts at sample 0, so the prewarm kernel's own copy of the formula is in the first receptive field of
every test.  Every test asserts NA_BatchStreamKernelName and NA_BatchStreamPackFactor before it trusts a comparison.

1. every case against the StdMath oracle (the rule of the file the case came from), against a float64 evaluation with an exact tanh
   (g <= F o + 2 e + 2e-6 level: F the factor the kernel family already has, o the oracle's and e the emulated float32 formula's distance
   from float64, the 2 for the hardware's 1-ulp exp2 / rcp units against the correctly rounded emulation) and AWAY from the FastMath oracle;
2. prewarm alone: silence into a prewarmed stream;  3. block lengths;  4. batches;  5. both policies in one launch;
6. LeakyReLU models do not notice the option;  7. quiet inputs: the absolute noise floor under StdMath, measured and held.

The forced-family knobs skip this file like tests/test_gpu_split.py.

Measured on an MI355X: see profiles/stdmath_error.txt (the lines this file prints under "stdmath-error")."""
import os

import numpy as np
import pytest

import na_oracle as O
import stdmath_cases as MC

FORCED = bool(os.environ.get("NA_WN_KERNEL") or os.environ.get("NA_WN_PACK") or os.environ.get("NA_WN_SPEC") or os.environ.get("NA_SP_T")
              or os.environ.get("NA_SP_GEN") or os.environ.get("NA_WN_PAD"))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(FORCED, reason="forced kernel family")]

TOL_RMS = MC.TOL_RMS
WINDOW = 32
BLOCK = MC.BLOCK
CASES = MC.cases()
TANH_CASES = [c for c in CASES if c["tanh"]]
CONTROLS = [c for c in CASES if not c["tanh"]]
# the floor the project states for quiet inputs under FastMath (test_quiet_inputs_keep_the_absolute_noise_floor_of_the_split_arithmetic)
FLOOR_VARYING, FLOOR_CONSTANT = 5e-7, 2e-7


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


@pytest.fixture(scope="module")
def std_loader(na):
    ld = na.NeuralModelLoader()
    ld.SetWaveNetMathMode(na.EMathMode.StdMath)
    return ld


@pytest.fixture(scope="module")
def fast_loader(na):
    return na.NeuralModelLoader()


_MODELS = {}


def _model(loader, case):
    """one model per (loader, case) of this module"""
    key = (id(loader), case["name"])
    if key not in _MODELS:
        m = loader.CreateFromString(MC.text(case), ".nam", doPrewarm=False)
        assert m is not None, case["name"]
        _MODELS[key] = m
    return _MODELS[key]


def _oracle(case, math_mode=O.MATH_STD):
    return O.OracleWaveNet(case["arrays"], case["weights"], math_mode=math_mode)


def _batch(na, m, case, streams):
    b = na.Batch(0)
    assert b.AddStreams(m, streams) == 0  # (prewarmed)
    _assert_lands(b, case, 0, streams)
    return b


def _assert_lands(b, case, first, count):
    for s in (first, first + count - 1):
        assert b.StreamKernelName(s) == case["kernel"] and b.StreamPackFactor(s) == case["pack"], (case["name"], s, b.StreamKernelName(s), b.StreamPackFactor(s))


def _run(batch, x, sizes):
    """x: [streams, samples] through calls of the given sizes (the last one cut to what is left)"""
    out, a = [], 0
    for c in sizes:
        c = min(c, x.shape[1] - a)
        if c <= 0:
            break
        out.append(batch.Process(np.ascontiguousarray(x[:, a:a + c])))
        a += c
    assert a == x.shape[1], (a, x.shape)
    return np.concatenate(out, axis=1)


def _blocks(samples):
    return [BLOCK] * ((samples + BLOCK - 1) // BLOCK)


def _rule_a(case, y, yo, y64, what):
    """The rule of the file the case came from, against the StdMath oracle; returns (error, bound) over the whole signal"""
    assert y.shape == yo.shape and np.all(np.isfinite(y)), what
    level = O.rms(yo)
    assert level > 1e-5, (what, level)  # (a silent model cannot pass)
    if case["rule"] == MC.RULE_F64:
        g, o = O.rms(y - y64), O.rms(yo - y64)
        bound = MC.bound_a(case, O.rms(y64), o)
        assert g <= bound, (what, g, o, O.rms(y64))
        return g, bound
    if case["rule"] == MC.RULE_WINDOW:
        for a in range(0, y.size, WINDOW):
            err, lv = O.rms(y[a:a + WINDOW] - yo[a:a + WINDOW]), O.rms(yo[a:a + WINDOW])
            assert err < TOL_RMS * max(1.0, lv), (what, "window at", a, err, lv)
    err, bound = O.rms(y - yo), MC.bound_a(case, level)
    assert err < bound, (what, err, level)
    return err, bound


_REFS = {}


def _refs(case):
    """(x, StdMath oracle, FastMath oracle, float64 with exact tanh, float64 with the emulated formula) of a case's own signal: computed
    once, shared, never written to"""
    if case["name"] not in _REFS:
        x = MC.signal(case)
        r = (x, _oracle(case).process(x), _oracle(case, O.MATH_FAST).process(x), MC.truth(case, x), MC.emulated(case, x))
        for v in r:
            v.setflags(write=False)
        _REFS[case["name"]] = r
    return _REFS[case["name"]]


# ---------------------------------------------------------------------------------------------------------- 1. every case

@pytest.mark.parametrize("case", TANH_CASES, ids=[c["name"] for c in TANH_CASES])
def test_every_stdmath_case_matches_the_stdmath_oracle_and_float64_and_not_the_fastmath_oracle(na, std_loader, case):
    """One prewarmed stream, 1536 samples of noise in blocks of 128.  (a) the case's own rule against the StdMath oracle; (b) against a
    float64 evaluation with an exact tanh: g <= F o + 2 e + 2e-6 level; (c) more than 100 x the bound of (a) away from the FastMath oracle:
    the flag reached the kernel."""
    x, yo, yf, y64, ye = _refs(case)
    b = _batch(na, _model(std_loader, case), case, 1)
    y = _run(b, x[None, :], _blocks(x.size))[0]
    b.close()
    g, o, e, level = O.rms(y - y64), O.rms(yo - y64), O.rms(ye - y64), O.rms(y64)
    away = O.rms(y - yf)
    print("stdmath-error %-16s %-20s level %.3g  g %.3g  o %.3g  e %.3g  (gpu - oracle %.3g, gpu - fastmath oracle %.3g)" % (
        case["name"], case["kernel"], level, g, o, e, O.rms(y - yo), away))
    _, bound = _rule_a(case, y, yo, y64, (case["name"], case["site"]))
    assert g <= case["factor"] * o + 2.0 * e + TOL_RMS * level, (case["name"], g, o, e, level)
    assert away > 100.0 * bound, (case["name"], away, bound)


# ---------------------------------------------------------------------------------------------------------- 2. prewarm alone

@pytest.mark.parametrize("name", MC.SILENCE_CASES)
def test_silence_into_a_prewarmed_stdmath_stream_is_the_stdmath_steady_state(na, std_loader, name):
    """256 samples of silence: nothing but what the prewarm kernel put into the rings (its own copy of the formula) and the block kernel
    continuing it.  The output is the constant the StdMath oracle gives -- to the 2e-6 RMS of rule (a); measured: within 4e-7 peak to peak
    except Nano, whose split arithmetic wanders 1.5e-6 peak to peak around it -- and not the FastMath oracle's, 9e-5 .. 4e-4 away."""
    case = MC.by_name(name)
    z = np.zeros((1, 256), dtype=np.float32)
    b = _batch(na, _model(std_loader, case), case, 1)
    y = _run(b, z, [BLOCK, BLOCK])[0].astype(np.float64)
    b.close()
    s, f = float(_oracle(case).process(z[0])[0]), float(_oracle(case, O.MATH_FAST).process(z[0])[0])
    tol = TOL_RMS * max(1.0, abs(s))
    print("%s: silence %.9g (spread %.3g), StdMath oracle %.9g, FastMath oracle %.9g" % (name, y[0], np.ptp(y), s, f))
    assert np.all(np.isfinite(y)) and O.rms(y - y[0]) <= tol and O.rms(y - s) <= tol, (name, float(y[0]), float(np.ptp(y)), s)
    assert abs(f - s) > 10.0 * tol and np.abs(y - f).min() > tol, (name, float(y[0]), s, f)


# ---------------------------------------------------------------------------------------------------------- 3. block lengths

def _longest_ring(case):
    """an upper bound of every history ring of a case in any state format: the padded history plus a block"""
    reach = max([(k - 1) * d for a in case["arrays"] for k, d in zip(a["kernel_sizes"], a["dilations"])] +
                [(a["head_kernel_size"] - 1) * a["head_dilation"] for a in case["arrays"]])
    return (reach + 15) // 16 * 16 + BLOCK


@pytest.mark.parametrize("name", MC.BLOCK_LENGTH_CASES)
def test_stdmath_streams_compute_the_same_bits_whatever_the_block_lengths(na, std_loader, name):
    """Calls of 1 .. 128 frames (the interpreter's wave shapes: at most 2 tiles, 3 .. 4, more than 4; the frame kernel's one and two
    waves), repeated until every ring has wrapped twice (Standard: 2532 frames against rings of at most 1152), against the same stream in
    blocks of 128: bit-identical, and on the StdMath oracle."""
    case = MC.by_name(name)
    reps = -(-2 * _longest_ring(case) // sum(MC.BLOCK_LENGTHS))
    sizes = MC.BLOCK_LENGTHS * reps
    total = sum(sizes)
    assert total >= 2 * _longest_ring(case) and (name != "standard" or total >= 2 * 1024)
    x = O.signal_noise(total, seed=case["seed"] + 50)
    ys = []
    for sz in (sizes, _blocks(total)):
        b = _batch(na, _model(std_loader, case), case, 1)
        ys.append(_run(b, x[None, :], sz)[0])
        b.close()
    assert np.array_equal(ys[0], ys[1]), (name, float(np.abs(ys[0] - ys[1]).max()), int(np.flatnonzero(ys[0] != ys[1])[0]))
    _rule_a(case, ys[0], _oracle(case).process(x), None, (name, "ragged"))


# ---------------------------------------------------------------------------------------------------------- 4. batches

BATCHES = [("standard", 3), ("standard", 515), ("nano", 5), ("nano", 1031), ("feather", 3), ("two-40-20", 3), ("g-13-3", 600)]
BATCH_SIZES = [BLOCK, BLOCK, 64, BLOCK, 37, BLOCK]


def _base_rows(rows, samples, seed):
    return np.stack([O.signal_noise(samples, seed + 1000 * r) for r in range(rows)])


@pytest.mark.parametrize("name,streams", BATCHES, ids=["%s-%d" % b for b in BATCHES])
def test_stdmath_batches_compute_per_stream_what_one_stream_computes(na, std_loader, name, streams):
    """Standard x 515: two streams per workgroup of the interpreter; Nano x 5 / x 1031: a partly filled dense virtual stream, more virtual
    streams than one wave of workgroups; the frame kernel at two streams per workgroup (600).  Seven noise rows repeated: streams fed the
    same row are bit-equal, stream 0 and the last stream follow the StdMath oracle."""
    case = MC.by_name(name)
    base = _base_rows(7, sum(BATCH_SIZES), case["seed"] + 3)
    x = np.ascontiguousarray(base[np.arange(streams) % 7])
    b = _batch(na, _model(std_loader, case), case, streams)
    y = _run(b, x, BATCH_SIZES)
    b.close()
    assert np.all(np.isfinite(y))
    bad = [s for s in range(7, streams) if not np.array_equal(y[s], y[s % 7])]
    assert not bad, (name, streams, len(bad), bad[:8])
    for s in (0, streams - 1):
        _rule_a(case, y[s], _oracle(case).process(x[s]), None, (name, streams, s))


# ---------------------------------------------------------------------------------------------------------- 5. two policies in one launch

MIXED_SEQUENCES = [[128] * 6, [128, 37, 64, 100, 32, 128]]


@pytest.mark.parametrize("name,count", [("standard", 3), ("nano", 5)])
def test_fastmath_and_stdmath_groups_of_one_launch_do_not_move_each_other_by_a_bit(na, std_loader, fast_loader, name, count):
    """One batch holds `count` FastMath streams and `count` StdMath streams of the same file: one interpreter launch of two groups whose
    layers take different sides of the wave-uniform activation branch (Nano: packed groups of both policies, each with a partly filled
    virtual stream).  The FastMath streams are bit-identical to a FastMath-only batch -- which runs its chain at 128 / 64 / 32 frames:
    chain and interpreter agree bit for bit -- and the StdMath streams to a StdMath-only batch."""
    case = MC.by_name(name)
    mf, ms = _model(fast_loader, case), _model(std_loader, case)
    for sizes in MIXED_SEQUENCES:
        x = _base_rows(2 * count, sum(sizes), case["seed"] + 9)
        both = na.Batch(0)
        assert both.AddStreams(mf, count) == 0 and both.AddStreams(ms, count) == count
        assert both.StreamKernelName(0) == "WaveNetSpecKernel" and both.StreamKernelName(count) == "WaveNetSplitKernel"  # (what each group would run alone)
        assert both.StreamPackFactor(0) == both.StreamPackFactor(2 * count - 1) == case["pack"]
        y = _run(both, x, sizes)
        both.close()
        alone = []
        for m, rows in ((mf, x[:count]), (ms, x[count:])):
            b = na.Batch(0)
            assert b.AddStreams(m, count) == 0
            alone.append(_run(b, rows, sizes))
            b.close()
        assert np.array_equal(y[:count], alone[0]), (name, sizes, "FastMath streams", float(np.abs(y[:count] - alone[0]).max()))
        assert np.array_equal(y[count:], alone[1]), (name, sizes, "StdMath streams", float(np.abs(y[count:] - alone[1]).max()))
        for s, mode in ((0, O.MATH_FAST), (count - 1, O.MATH_FAST), (count, O.MATH_STD), (2 * count - 1, O.MATH_STD)):
            yo = _oracle(case, mode).process(x[s])
            assert O.rms(y[s] - yo) < TOL_RMS * max(1.0, O.rms(yo)), (name, sizes, s, O.rms(y[s] - yo))


# ---------------------------------------------------------------------------------------------------------- 6. LeakyReLU

@pytest.mark.parametrize("case", CONTROLS, ids=[c["name"] for c in CONTROLS])
def test_the_policy_does_not_touch_leakyrelu_models(na, std_loader, fast_loader, case):
    """One control per plan builder that sets the flag or the layer field: loaded both ways, the same bits."""
    x = MC.signal(case)
    ys = []
    for ld in (fast_loader, std_loader):
        b = _batch(na, _model(ld, case), case, 1)
        ys.append(_run(b, x[None, :], _blocks(x.size))[0])
        b.close()
    assert np.array_equal(ys[0], ys[1]), (case["name"], float(np.abs(ys[0] - ys[1]).max()))
    _rule_a(case, ys[1], _oracle(case).process(x), None, case["name"])


# ---------------------------------------------------------------------------------------------------------- 7. quiet inputs

QUIET = MC.quiet_cases()


def _parts(v, truth):
    e = np.asarray(v, dtype=np.float64) - truth
    return abs(float(e.mean())), O.rms(e - e.mean())


@pytest.mark.parametrize("amp", [1e-3, 1e-5])
@pytest.mark.parametrize("case", QUIET, ids=[c["name"] for c in QUIET])
def test_quiet_inputs_keep_the_absolute_noise_floor_under_stdmath(na, std_loader, case, amp):
    """test_quiet_inputs_keep_the_absolute_noise_floor_of_the_split_arithmetic under StdMath: amp (sin 0.013 t + 0.3 sin 0.31 t), the error
    against a float64 evaluation with an exact tanh split into its constant and its varying part.  The device formula cancels near zero
    (an absolute error of up to 1.8e-7 per activation where a correctly rounded tanh has 3e-8), so this is where the policy could lose
    the floor the project states for quiet passages: varying part at most 5e-7 RMS, constant part at most 2e-7."""
    x = MC.quiet_signal(amp)
    t = MC.truth(case, x)
    b = _batch(na, _model(std_loader, case), case, 1)
    y = _run(b, x[None, :], _blocks(x.size))[0]
    b.close()
    (g_dc, g_ac), (o_dc, o_ac), (e_dc, e_ac) = _parts(y, t), _parts(_oracle(case).process(x), t), _parts(MC.emulated(case, x), t)
    g, o, e, level = O.rms(y - t), O.rms(_oracle(case).process(x) - t), O.rms(MC.emulated(case, x) - t), O.rms(t)
    print("stdmath-error quiet %-9s amp %g  constant / varying: gpu %.3g / %.3g  oracle %.3g / %.3g  emulated formula %.3g / %.3g  (g %.3g  o %.3g  e %.3g)" % (
        case["name"], amp, g_dc, g_ac, o_dc, o_ac, e_dc, e_ac, g, o, e))
    assert g <= case["factor"] * o + 2.0 * e + TOL_RMS * level, (case["name"], amp, g, o, e, level)
    assert g_ac <= FLOOR_VARYING and g_dc <= FLOOR_CONSTANT, (case["name"], amp, g_dc, g_ac)
