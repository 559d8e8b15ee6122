"""The StdMath WaveNet policy without a GPU (tests/stdmath_cases.py; tests/test_gpu_stdmath.py runs the cases on the device).

* the device formula restated in correctly rounded float32 operations (stdmath_cases.emulated_std_tanh) against np.tanh, elementwise:
  the number behind the "absolute error ~1e-7" comments beside the device copies;
* every case loads under both policies, lands on the kernel family and pack factor it names whatever the policy, and only the kernel
  NAME of the official architectures moves: their specialised chains refuse a StdMath plan, so the stage interpreter runs them;
* a launch that holds a chain group and an interpreter group runs the interpreter at every block length the chains take;
* the cases reach every code site of the policy;
* every tanh case tells the two policies apart by more than 100 x the bound the GPU test applies to it."""
import numpy as np
import pytest

import na_oracle as O
import stdmath_cases as MC

CASES = MC.cases()
TANH_CASES = [c for c in CASES if c["tanh"]]
# csrc/wavenet_dev.h WnSpecArch and csrc/wavenet_launch_choice.h, as tests/test_wavenet_dispatch_cpu.py names them
SPEC_NONE, SPEC_STD, SPEC_LITE, SPEC_LITE16 = 0, 1, 2, 3
K_INTERPRETER = 3
# |emulated_std_tanh - tanh| on the grid below is 1.8e-7 at its worst (x = -1.51: 1 - 2 r cancels, and r carries the rounding of exp2, of
# the sum and of the reciprocal); one f32 ulp of 1.0 (6e-8, rounded up) for what the grid steps over
FORMULA_MAX_ABS_ERROR = 2.5e-7


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    return neuralaudio_amd


def _loaders(na):
    fast, std = na.NeuralModelLoader(), na.NeuralModelLoader()
    std.SetWaveNetMathMode(na.EMathMode.StdMath)
    return fast, std


def _grid():
    mag = np.concatenate([np.logspace(-8, np.log10(20.0), 200001), np.linspace(1e-3, 20.0, 400001)])
    return np.concatenate([mag, -mag, [100.0, -100.0, np.inf, -np.inf, 0.0]])


def test_the_device_formula_in_float32_is_within_a_quarter_of_a_millionth_of_tanh():
    x = _grid()
    y = MC.emulated_std_tanh(x)
    assert y.dtype == np.float64 and np.all(np.isfinite(y))
    x32 = x.astype(np.float32).astype(np.float64)
    err = np.abs(y - np.tanh(x32))
    worst = int(np.argmax(err))
    print("emulated formula: worst |error| %.3g at x = %.6g; f32-rounded tanh %.3g" % (err[worst], x[worst], np.abs(MC.f32_rounded_tanh(x) - np.tanh(x32)).max()))
    assert err.max() <= FORMULA_MAX_ABS_ERROR, (float(err.max()), float(x[worst]))
    assert err.max() > 1e-7  # (the cancellation is real: a correctly rounded f32 tanh is 3e-8)
    n = (x.size - 5) // 2
    assert np.abs(y[:n] + y[n:2 * n]).max() <= 2.0 * FORMULA_MAX_ABS_ERROR  # odd to within its own error
    assert np.all(np.abs(y) <= 1.0)
    for v in (20.0, 100.0, np.inf):
        assert MC.emulated_std_tanh(v) == 1.0 and MC.emulated_std_tanh(-v) == -1.0, v
    assert MC.emulated_std_tanh(0.0) == 0.0
    # near zero the formula's error is absolute: below 6e-8 it returns multiples of an ulp of 1.0 (the step the quiet-input test measures)
    tiny = MC.emulated_std_tanh(np.float32(1e-8))
    assert abs(tiny - 1e-8) <= 6e-8 and tiny in (0.0, float(np.float32(2.0) ** -23), float(np.float32(2.0) ** -24))


def test_every_case_loads_and_lands_on_its_kernel_under_both_policies(na):
    fast, std = _loaders(na)
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names) and 12 <= len(TANH_CASES) <= 14 and len(CASES) - len(TANH_CASES) >= 1
    for case in CASES:
        text = MC.text(case)
        assert MC.work(case) <= MC.WORK_CAP, (case["name"], MC.work(case))
        assert O.wavenet_num_weights(case["arrays"]) == case["weights"].size, case["name"]
        assert all(a["activation"] == (O.ACT_TANH if case["tanh"] else O.ACT_LEAKYRELU) for a in case["arrays"]), case["name"]
        mf, ms = fast.CreateFromString(text, ".nam", doPrewarm=False), std.CreateFromString(text, ".nam", doPrewarm=False)
        assert mf is not None and ms is not None, case["name"]
        assert ms.GetReceptiveFieldSize() == mf.GetReceptiveFieldSize() == O.OracleWaveNet(case["arrays"], case["weights"], prewarm=False).receptive_field
        for streams in (1, 600):
            i_f, i_s = mf.KernelInfo(1.0, streams), ms.KernelInfo(1.0, streams)
            assert (i_s["kernel"], i_s["pack"]) == (case["family"], case["pack"]), (case["name"], streams, i_s)
            assert i_s == i_f, (case["name"], streams, i_s, i_f)  # family, pack, input limit, range proof: the policy moves none of them
            k_f, k_s = na.wavenet_kernel(mf, streams), na.wavenet_kernel(ms, streams)
            assert k_s["kernel_name"] == case["kernel"], (case["name"], streams, k_s)
            assert k_s["spec_arch"] == SPEC_NONE or not case["tanh"], (case["name"], streams, k_s)  # no chain is picked for a StdMath tanh model
            if case["official"]:
                assert k_f["spec_arch"] != SPEC_NONE and k_f["kernel_name"] == "WaveNetSpecKernel", (case["name"], streams, k_f)
            else:
                assert k_f["spec_arch"] == SPEC_NONE and k_f["kernel_name"] == case["kernel"], (case["name"], streams, k_f)
            for key in ("family", "pack", "dense", "virtual", "launch_kind", "range_proven", "weights_ok", "input_limit"):
                assert k_s[key] == k_f[key], (case["name"], streams, key, k_s, k_f)
            if not case["tanh"]:
                assert k_s == k_f, (case["name"], streams)


def test_a_launch_of_a_chain_group_and_an_interpreter_group_runs_the_interpreter(na):
    """What the mixed-policy batches of tests/test_gpu_stdmath.py rely on: FastMath Standard (its chain's group) and StdMath Standard (no
    chain) in one launch, and the same for two packed Nano groups, run the interpreter at the block lengths the chains take."""
    for groups, pk in (([(SPEC_STD, 1, 2, 3, 0, 2048), (SPEC_NONE, 1, 2, 3, 0, 2048)], 0), ([(SPEC_NONE, 1, 2, 3, 0, 2048), (SPEC_STD, 1, 2, 3, 0, 2048)], 0),
                       ([(SPEC_LITE, 4, 2, 5, 1, 2048), (SPEC_NONE, 4, 2, 5, 1, 2048)], 1)):
        for n in (128, 64, 32):
            r = na.wavenet_launch(groups, n)
            assert r[0] == K_INTERPRETER and r[1] == 0 and r[6] == 2 and r[8] == 0 and r[9] == pk, (groups, n, r)
    # and the group facts assumed above are the ones the library derives for the two loads
    fast, std = _loaders(na)
    for name, arch, pack in (("standard", SPEC_STD, 1), ("nano", SPEC_LITE, 4)):
        text = MC.text(MC.by_name(name))
        k_f, k_s = na.wavenet_kernel(fast.CreateFromString(text, ".nam", doPrewarm=False), 3), na.wavenet_kernel(std.CreateFromString(text, ".nam", doPrewarm=False), 3)
        assert (k_f["spec_arch"], k_f["pack"]) == (arch, pack) and (k_s["spec_arch"], k_s["pack"]) == (SPEC_NONE, pack), (name, k_f, k_s)


def test_the_cases_reach_every_code_site_of_the_policy(na):
    """From the kernel the library predicts for the StdMath load, the channel counts and the plan facts -- not from the cases' labels."""
    _, std = _loaders(na)
    fast = na.NeuralModelLoader()
    reached = {site: [] for site in MC.SITES}
    facts = dict(packs=set(), custom_packs=set(), frame_ks=set(), frame_rules=set(), frame_partial=False, narrow_beside_wide=False, control_families=set())
    for case in CASES:
        text = MC.text(case)
        k = na.wavenet_kernel(std.CreateFromString(text, ".nam", doPrewarm=False), 1)
        official = na.wavenet_kernel(fast.CreateFromString(text, ".nam", doPrewarm=False), 1)["spec_arch"] != SPEC_NONE
        widest = max(max(a["channels"], a["head_size"], a["input_size"]) for a in case["arrays"])
        if not case["tanh"]:
            facts["control_families"].add(k["family"])
            continue
        if k["family"] == "f16-split":
            assert widest <= 16 and k["kernel_name"] == "WaveNetSplitKernel"
            site = "split-official" if official else "split-custom"
            facts["packs" if official else "custom_packs"].add(k["pack"])
        elif k["family"] == "frame":
            assert widest <= 16
            site = "frame"
            facts["frame_ks"] |= {ks for a in case["arrays"] for ks in a["kernel_sizes"]}
            facts["frame_rules"].add(case["rule"])
            facts["frame_partial"] |= any(a["channels"] % 4 for a in case["arrays"])
            assert k["range_proven"] == (case["rule"] != MC.RULE_F64) or any(ks != 3 for a in case["arrays"] for ks in a["kernel_sizes"])
        else:
            assert k["family"] == "generic" and 17 <= widest <= 128
            site = "wide" if widest > 64 else "generic"
            assert k["kernel_name"] == ("WaveNetWideKernel" if widest > 64 else "WaveNetGenericKernel")
            facts["narrow_beside_wide"] |= min(a["channels"] for a in case["arrays"]) <= 16
        assert site == case["site"], (case["name"], site)
        reached[site].append(case["name"])
        reached["prewarm"].append(case["name"])  # (every case is run prewarmed, from sample 0)
    print(reached, facts)
    assert all(reached[site] for site in MC.SITES), reached
    assert len(reached["split-official"]) == 4 and facts["packs"] == {1, 2, 4} and facts["custom_packs"] == {1, 2, 4}
    assert {1, 2, 3} <= facts["frame_ks"] and facts["frame_rules"] == {MC.RULE_WINDOW, MC.RULE_F64} and facts["frame_partial"]
    assert facts["narrow_beside_wide"] and facts["control_families"] == {"f16-split", "frame", "generic"}
    # the prewarm-alone test takes one case per copy of the formula
    assert {MC.by_name(n)["site"] for n in MC.SILENCE_CASES} >= {"split-official", "split-custom", "frame", "generic", "wide"}


@pytest.mark.parametrize("case", TANH_CASES, ids=[c["name"] for c in TANH_CASES])
def test_every_tanh_case_tells_the_two_policies_apart(case):
    """A float64 evaluation with np.tanh against one with the FastMath rational, on the case's own signal: more than 100 x the bound the
    GPU test holds the case to (a case that cannot tell the policies apart shows nothing; 3e-4 .. 8e-4 on the trained models).  The
    emulated device formula and the StdMath C oracle sit far inside that bound, so the bound of the GPU test has room for neither a
    wrong constant nor a dropped flag."""
    x = MC.signal(case)
    t = MC.truth(case, x)
    level = O.rms(t)
    o = O.rms(O.OracleWaveNet(case["arrays"], case["weights"], math_mode=O.MATH_STD).process(x) - t)
    e = O.rms(MC.emulated(case, x) - t)
    apart = O.rms(MC.fastmath(case, x) - t)
    bound = MC.bound_a(case, level, o)
    print("%s: level %.3g, policies %.3g apart = %.0f x the bound %.3g; oracle %.3g, emulated formula %.3g from float64" % (case["name"], level, apart, apart / bound, bound, o, e))
    assert level > 1e-2 and apart > 100.0 * bound, (case["name"], level, apart, bound)
    assert case["factor"] * o + 2.0 * e + MC.TOL_RMS * level < apart / 50.0, (case["name"], o, e, apart)  # the float64 bound of the GPU test, too


@pytest.mark.parametrize("name", MC.SILENCE_CASES)
def test_the_steady_states_of_the_two_policies_differ(name):
    """The prewarm-alone GPU test needs the silence output of a prewarmed stream to depend on the policy by more than its tolerance."""
    case = MC.by_name(name)
    z = np.zeros(256, dtype=np.float32)
    s, f = (O.OracleWaveNet(case["arrays"], case["weights"], math_mode=m).process(z) for m in (O.MATH_STD, O.MATH_FAST))
    assert np.ptp(s) == 0.0 and np.ptp(f) == 0.0
    assert abs(float(s[0]) - float(f[0])) > 10.0 * MC.TOL_RMS * max(1.0, abs(float(s[0]))), (name, float(s[0]), float(f[0]))
    assert abs(float(s[0]) - MC.truth(case, z)[0]) < MC.TOL_RMS
