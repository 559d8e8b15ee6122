"""Models of the tests of the StdMath WaveNet policy (NA_SetWaveNetMathMode(StdMath): std::tanh instead of the rational FastMath tanh) on
every kernel that implements it -- TEST INFRASTRUCTURE ONLY.

Shared by tests/test_gpu_stdmath.py (which runs them) and tests/test_stdmath_cpu.py (which proves without a GPU that every case loads,
is predicted on the kernel it names under both policies, that the cases reach every code site of the policy and that each of them can
tell the two policies apart).  Pure Python and numpy, seeded, never skips.

On the device the policy is the formula tanh(x) = 1 - 2 rcp(exp2(2 log2(e) x) + 1), reached through a stage flag (WN_FLAG_STD_TANH:
wavenet_plan.cpp, the f16-split plan and the frame plan) or a layer field (WnPrewarmLayer::act == 2: both builders).  The code sites, by
the name the cases carry in case["site"]:

* "split-official"  the stage interpreter (wavenet_split_kernels.hip, the activation branch of the layer stage) on the official tanh
                    architectures, which leave their specialised chains for it when the option is on (wavenet_spec_impl.h refuses a plan
                    with the flag): A1 Standard, a padded Lite 12 / 6, Feather (pack 2), Nano (pack 4, dense);
* "split-custom"    the same interpreter on runtime-shaped narrow models (tests/split_cases.py): a plain 16 / 8, the packed flavour
                    at P = 2, and at P = 4 with one channel group per stream;
* "frame"           wavenet_frame_kernels.hip StdTanh2 (tests/frame_cases.py: a K != 3 layer, or no range proof);
* "generic"         WaveNetGenericKernel (17 .. 64 channels), Activate(v, 2) of wavenet_generic_kernels.hip;
* "wide"            WaveNetWideKernel (65 .. 128 channels), the same function from the other kernel;
* "prewarm"         wavenet_prewarm_kernels.hip: the steady-state columns of every prewarmed stream -- every case (the GPU tests prewarm
                    every stream and compare from sample 0).

Every case carries the tolerance rule of the file it came from:
* RULE_RMS     2e-6 RMS over the whole signal, relative to the output level above 1 (test_gpu_parity.py, test_gpu_spec.py, test_gpu_wide.py);
* RULE_WINDOW  the same number on every 32-frame window (test_gpu_split.py, test_gpu_frame.py);
* RULE_F64     a model that is badly conditioned on purpose: at most 4 x the f32 oracle's own distance from a float64 evaluation plus 2e-6
               of the level (frame_cases.RULE_F64, test_models_without_a_range_proof_run_on_the_f32_kernel);
and the factor F its kernel family already has against float64: 8 for the 22-bit split values, 4 for the f32 frame kernel.

Head gain: the synthetic models end in a head scale of 0.02, which leaves them at a level of 0.002 .. 0.07 where the bounds above are
absolute: the two tanh policies, 3e-4 .. 2e-3 apart per activation, would then differ by less than 100 x the bound at the output and a
dropped flag could pass.  As in split_cases.HEAD_GAIN the head scale -- one f32 multiplication at the very end, in the kernel, the oracle
and the float64 reference alike -- is raised per case (GAINS) until the policies are more than 100 x the bound apart on the case's signal
(tests/test_stdmath_cpu.py asserts it).  The bounds stay what they are, so a raised gain only tightens them."""
import os

import numpy as np

import frame_cases as FC
import na_oracle as O
import ref_np
import split_cases as SC
import wide_cases as WC

SAMPLES = 1536           # 12 blocks of 128
BLOCK = 128
WORK_CAP = SC.WORK_CAP   # sum over layers of channels^2 x K x samples: oracle plus GPU stay far under a second
TOL_RMS = 2e-6
RULE_RMS, RULE_WINDOW, RULE_F64 = "2e-6 RMS over the signal", "2e-6 RMS per 32-frame window", FC.RULE_F64
SITES = ("split-official", "split-custom", "frame", "generic", "wide", "prewarm")
TWO_LOG2E = np.float32(2.885390081777927)  # 2 log2(e), the constant of the device formula


def emulated_std_tanh(z):
    """The device formula 1 - 2 rcp(exp2(2 log2(e) x) + 1) with every operation correctly rounded to float32 (the hardware's exp2 and rcp
    units are 1-ulp units: this is the plain restatement against which the device's extra error is bounded).  Returns float64; usable as
    ref_np.wavenet_forward(..., tanh=emulated_std_tanh)."""
    x = np.asarray(z, dtype=np.float64).astype(np.float32)
    one, two = np.float32(1.0), np.float32(2.0)
    with np.errstate(over="ignore"):
        p = (x * TWO_LOG2E).astype(np.float32)
        e = np.exp2(p.astype(np.float64)).astype(np.float32)      # (float64 exp2, rounded once: a correctly rounded f32 exp2)
        s = (e + one).astype(np.float32)
        r = (one / s).astype(np.float32)
        return (one - (two * r).astype(np.float32)).astype(np.float32).astype(np.float64)


def f32_rounded_tanh(z):
    """what std::tanh gives: a float64 tanh of the f32 argument, rounded to f32"""
    return np.tanh(np.asarray(z, dtype=np.float64).astype(np.float32).astype(np.float64)).astype(np.float32).astype(np.float64)


def _case(name, site, family, kernel, arrays, weights, rule, factor, seed, file=None, pack=1, gain=1.0, official=False, tanh=True):
    return dict(name=name, site=site, family=family, kernel=kernel, arrays=arrays, weights=weights, rule=rule, factor=factor, seed=seed, file=file,
                pack=pack, gain=gain, official=official, tanh=tanh, samples=SAMPLES)


def _gained(arrays, w, gain):
    return O.scale_wavenet_tensors(arrays, w, {"head_scale": gain}) if gain != 1.0 else np.asarray(w, dtype=np.float32)


def _file_case(name, file, pack, seed):
    j = O.load_json(file)
    return _case(name, "split-official", "f16-split", "WaveNetSplitKernel", O.wavenet_arrays_from_nam(j), np.asarray(j["weights"], dtype=np.float32),
                 RULE_RMS, 8.0, seed, file=file, pack=pack, official=True)


# head gains (see the module docstring): as small a power of two as leaves every case more than 100 x its bound between the policies
GAINS = {"lite": 16.0, "shift-d1-16-8": 4.0, "shift-d64-3": 4.0, "shift-d128-8-4": 8.0, "g-13-3": 64.0, "shift-k1": 64.0, "two-40-20": 64.0, "two-72-36": 64.0,
         "fixed-8-40": 64.0}  # (the split_cases models: on top of their own split_cases.HEAD_GAIN)


def cases():
    out = []

    # ---- the interpreter on the official architectures (tests/test_gpu_spec.py: _models, _lite)
    out.append(_file_case("standard", "BossWN-standard.nam", 1, 11))
    lite = O.a1_arrays(12, 6)
    out.append(_case("lite", "split-official", "f16-split", "WaveNetSplitKernel", lite, _gained(lite, O.synth_wavenet_weights(lite, seed=33), GAINS["lite"]),
                     RULE_RMS, 8.0, 12, official=True, gain=GAINS["lite"]))
    out.append(_file_case("feather", "BossWN-feather.nam", 2, 13))
    out.append(_file_case("nano", "BossWN-nano.nam", 4, 14))

    # ---- the interpreter on runtime-shaped models: compact rings only (d <= 16) on a plain 16 / 8; dilations below 128 at P = 4 with one
    # channel group per stream; dilations at and above 128 at P = 2
    named = {c["name"]: c for c in SC.named_cases()}
    for name in ("shift-d1-16-8", "shift-d64-3", "shift-d128-8-4"):
        c = named[name]
        out.append(_case(name, "split-custom", "f16-split", "WaveNetSplitKernel", c["arrays"], _gained(c["arrays"], SC.weights(c), GAINS[name]), RULE_WINDOW, 8.0, c["seed"], pack=c["pack"],
                         gain=c["gain"] * GAINS[name]))

    # ---- the f32 frame kernel: a G sweep case whose last groups are not full (13 -> 3 channels: G = 4 and G = 1), a K = 1 layer between
    # K = 2 layers, A1 Standard without the range proof
    named = {c["name"]: c for c in FC.named_cases()}
    for name in ("g-13-3", "shift-k1", "no-proof-a1"):
        c = named[name]
        gain = GAINS.get(name, 1.0)
        out.append(_case(name, "frame", "frame", "WaveNetFrameKernel", c["arrays"], _gained(c["arrays"], FC.weights(c), gain), c["rule"] if c["rule"] == RULE_F64 else RULE_WINDOW,
                         4.0, c["seed"], gain=gain))

    # ---- 17 .. 128 channels: the two-array models of tests/test_gpu_snapshot.py and a narrow array beside a wide one
    for name, site, kernel, arrays, seed in (("two-40-20", "generic", "WaveNetGenericKernel", WC.two_array(40, 20), 40),
                                             ("two-72-36", "wide", "WaveNetWideKernel", WC.two_array(72, 36), 72),
                                             ("fixed-8-40", "generic", "WaveNetGenericKernel", WC.fixed_case((8, 40), O.ACT_TANH), 48)):
        out.append(_case(name, site, "generic", kernel, arrays, _gained(arrays, O.synth_wavenet_weights(arrays, seed=seed), GAINS[name]), RULE_RMS, 8.0, seed, gain=GAINS[name]))

    # ---- controls: LeakyReLU models, one per plan builder that sets the flag or the field; the option must change nothing, bit for bit
    c = {c["name"]: c for c in SC.named_cases()}["leaky-16-8"]
    out.append(_case("control-split-leaky-16-8", "control", "f16-split", "WaveNetSplitKernel", c["arrays"], SC.weights(c), RULE_WINDOW, 8.0, c["seed"], gain=c["gain"], tanh=False))
    c = {c["name"]: c for c in FC.named_cases()}["g-5"]
    out.append(_case("control-frame-leaky-g-5", "control", "frame", "WaveNetFrameKernel", c["arrays"], FC.weights(c), RULE_WINDOW, 4.0, c["seed"], tanh=False))
    arrays = WC.two_array(24, 12, O.ACT_LEAKYRELU)
    out.append(_case("control-generic-leaky-24-12", "control", "generic", "WaveNetGenericKernel", arrays, O.synth_wavenet_weights(arrays, seed=24), RULE_RMS, 8.0, 24, tanh=False))
    return out


def by_name(name):
    return [c for c in cases() if c["name"] == name][0]


def text(case):
    """the .nam document of a case (a file's own text for the official files)"""
    if case["file"]:
        with open(os.path.join(O.MODELS_DIR, case["file"])) as f:
            return f.read()
    return O.nam_json_wavenet_generic(case["arrays"], case["weights"])


def work(case):
    return sum(a["channels"] ** 2 * k * case["samples"] for a in case["arrays"] for k in a["kernel_sizes"])


def signal(case, samples=None):
    return O.signal_noise(samples or case["samples"], seed=case["seed"])


def quiet_signal(amp, n=2048):
    """test_gpu_spec.py _quiet_errors"""
    return (amp * np.sin(0.013 * np.arange(n)) + 0.3 * amp * np.sin(0.31 * np.arange(n))).astype(np.float32)


def truth(case, x):
    """float64 evaluation with an exact tanh"""
    return ref_np.wavenet_forward(case["arrays"], case["weights"], x, tanh=np.tanh)[0]


def emulated(case, x):
    """float64 evaluation with the device formula in correctly rounded float32 operations"""
    return ref_np.wavenet_forward(case["arrays"], case["weights"], x, tanh=emulated_std_tanh)[0]


def fastmath(case, x):
    """float64 evaluation with the rational FastMath tanh"""
    return ref_np.wavenet_forward(case["arrays"], case["weights"], x, tanh=ref_np.fast_tanh)[0]


def bound_a(case, level, oracle_error=0.0):
    """the bound of a case's own rule on an RMS error at output level `level` (RULE_WINDOW: per window, so also over the whole signal)"""
    if case["rule"] == RULE_F64:
        return 4.0 * oracle_error + TOL_RMS * level
    return TOL_RMS * max(1.0, level)


# one case per copy of the formula (and both kernels that share the generic copy): the prewarm-alone test
SILENCE_CASES = ("standard", "nano", "shift-d64-3", "g-13-3", "fixed-8-40", "two-72-36")
# the block-length test: the interpreter's wave shapes (tiles <= 2, 3 .. 4, > 4) on both of its flavours, and the other kernels
BLOCK_LENGTH_CASES = ("standard", "nano", "shift-d128-8-4", "shift-k1", "two-40-20")
BLOCK_LENGTHS = [1, 16, 17, 33, 64, 65, 127, 128, 100, 128, 37, 128]


def quiet_cases():
    """Standard, Lite and Nano as tests/test_gpu_spec.py _quiet_errors loads them: the floor of the quiet-input test is an absolute number,
    so Lite keeps the head scale it has there"""
    lite = O.a1_arrays(12, 6)
    return [by_name("standard"), _case("lite-as-trained", "split-official", "f16-split", "WaveNetSplitKernel", lite, O.synth_wavenet_weights(lite, seed=33), RULE_RMS, 8.0, 12, official=True),
            by_name("nano")]
