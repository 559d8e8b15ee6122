"""The compile-time specialised WaveNet layer chains (wavenet_spec_kernels.hip) and the range / precision contract of the f16-split path.

* The specialised chains keep the stream-state format, the operand images and the order of floating-point operations of the stage
  interpreter (wavenet_split_kernels.hip), so both must agree BIT FOR BIT on the same stream -- also when a stream alternates between
  them (blocks of 128 / 64 / 32 frames run the chain, every other length the interpreter).
* Which kernel a default load of every official architecture lands on is asserted here (a silent WaveNetKernelFor regression would keep
  parity green and halve the bench).
* Quiet inputs (1e-3 .. 1e-6): the split path must be as accurate as f32 arithmetic, measured against a float64 evaluation.
* Inputs beyond the f16 range, infinities and NaNs: the contract is "clamped to +-condLimit, NaN reads as silence"; the output stays
  finite and the stream recovers after one receptive field.
"""
import os

import numpy as np
import pytest

import na_oracle as O
import ref_np

pytestmark = pytest.mark.gpu

TOL_RMS = 2e-6
FORCED = bool(os.environ.get("NA_WN_KERNEL") or os.environ.get("NA_WN_PACK") or os.environ.get("NA_WN_SPEC") or os.environ.get("NA_SP_T")
              or os.environ.get("NA_SP_GEN") or os.environ.get("NA_WN_PAD"))


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


@pytest.fixture(scope="module")
def loader(na):
    return na.NeuralModelLoader()


@pytest.fixture()
def spec_switch(na):
    from neuralaudio_amd import capi
    lib = capi.load_library()
    yield lambda on: lib.NA_DebugSetWaveNetSpec(1 if on else 0)
    lib.NA_DebugSetWaveNetSpec(1)


def _path(name):
    return os.path.join(O.MODELS_DIR, name)


def _lite(loader):
    arrays = O.a1_arrays(12, 6)
    w = O.synth_wavenet_weights(arrays, seed=33)
    return loader.CreateFromString(O.nam_json_wavenet_a1(12, 6, w), ".nam", doPrewarm=False), arrays, w


def _models(loader, which):
    if which == "standard":
        return loader.CreateFromFile(_path("BossWN-standard.nam"), doPrewarm=False), lambda: O.oracle_from_file("BossWN-standard.nam")
    if which == "lite":
        m, arrays, w = _lite(loader)
        return m, lambda: O.OracleWaveNet(arrays, w)
    name = {"feather": "BossWN-feather.nam", "nano": "BossWN-nano.nam"}[which]
    return loader.CreateFromFile(_path(name), doPrewarm=False), lambda: O.oracle_from_file(name)


def _run(batch, x, sizes):
    out, a = [], 0
    for c in sizes:
        out.append(batch.Process(np.ascontiguousarray(x[:, a:a + c])))
        a += c
    return np.concatenate(out, axis=1)


SEQUENCES = [[128] * 6, [64] * 8, [32] * 8, [128, 37, 64, 100, 32, 128, 1, 64, 128, 128]]


@pytest.mark.skipif(FORCED, reason="forced kernel family")
@pytest.mark.parametrize("which,streams", [("standard", 3), ("standard", 515), ("lite", 2), ("lite", 513), ("feather", 1030), ("nano", 1031),
                                           ("nano", 6), ("nano", 1003)])
def test_specialised_chain_is_bit_identical_to_the_interpreter(na, loader, spec_switch, which, streams):
    """(Nano x 6 / x 1003 / x 1031: partly filled last virtual stream.  Which instantiation these host-buffer calls land on is not what this
    test is about -- 512 kernel-level streams or more run as two half-batch launches, both at SPB = 1, and the default dense Nano pack
    never takes the one-tile-per-wave chain: tests/test_gpu_chain_wraps.py pins every instantiation and runs it past its ring wraps.)"""
    m, make_oracle = _models(loader, which)
    rng = np.random.default_rng(11)
    for sizes in SEQUENCES:
        total = sum(sizes)
        base = (0.3 * rng.standard_normal((min(streams, 9), total))).clip(-1, 1).astype(np.float32)
        x = base[np.arange(streams) % base.shape[0]]
        ys = []
        for on in (True, False):
            spec_switch(on)
            b = na.Batch(0)
            b.AddStreams(m, streams)
            assert b.StreamKernelName(0) == ("WaveNetSpecKernel" if on else "WaveNetSplitKernel")
            ys.append(_run(b, x, sizes))
            b.close()
        spec_switch(True)
        assert np.all(np.isfinite(ys[0]))
        assert np.array_equal(ys[0], ys[1]), (which, streams, sizes, float(np.abs(ys[0] - ys[1]).max()))
        for s in (0, streams - 1):
            assert O.rms(ys[0][s] - make_oracle().process(x[s])) < TOL_RMS, (which, s)


@pytest.mark.skipif(FORCED, reason="forced kernel family")
@pytest.mark.parametrize("streams", [5, 1030])
def test_a2_chains_are_bit_identical_to_the_interpreter_and_match_the_oracles(na, loader, spec_switch, streams):
    """Both A2 submodels (8 channels: two tiles per wave; 3 channels: four tiles per wave) in ONE launch of the A2 family: kernel sizes 6 and
    15 with their operand blocks chunked through LDS, dilations that are not tile multiples (straddling taps on many waves), the conv
    head with its own ring, LeakyReLU -- against the stage interpreter's generic flavour bit for bit, and against the oracles."""
    m = loader.CreateFromFile(_path("BossWN-a2.nam"), doPrewarm=False)
    rng = np.random.default_rng(21)
    qs = [0.0, 1.0, 0.3, 0.9]
    for sizes in ([128] * 5, [64] * 6, [128, 37, 64, 100, 128, 1, 64, 128]):
        total = sum(sizes)
        base = (0.3 * rng.standard_normal((7, total))).clip(-1, 1).astype(np.float32)
        x = base[np.arange(streams) % 7]
        ys = []
        for on in (True, False):
            spec_switch(on)
            b = na.Batch(0)
            for k in range(4):
                b.AddStreams(m, streams // 4 + (1 if k < streams % 4 else 0), quality=qs[k])
            assert b.NumStreams() == streams
            ys.append(_run(b, x, sizes))
            b.close()
        spec_switch(True)
        assert np.all(np.isfinite(ys[0]))
        assert np.array_equal(ys[0], ys[1]), (streams, sizes, float(np.abs(ys[0] - ys[1]).max()))
        first = 0
        for k in range(4):
            c = streams // 4 + (1 if k < streams % 4 else 0)
            for s_ in {first, first + c - 1}:
                if c > 0:
                    assert O.rms(ys[0][s_] - O.oracle_from_file("BossWN-a2.nam", quality=qs[k]).process(x[s_])) < TOL_RMS, (k, s_)
            first += c


@pytest.mark.skipif(FORCED, reason="forced kernel family")
def test_config3_mixed_packed_launch_is_bit_identical_to_the_interpreter(na, loader, spec_switch):
    """Lite (padded, pack 1) + Feather (pack 2) + Nano (pack 4): one launch of the packed chain, two architectures of the lite family."""
    lite, arrays, w = _lite(loader)
    feather = loader.CreateFromFile(_path("BossWN-feather.nam"), doPrewarm=False)
    nano = loader.CreateFromFile(_path("BossWN-nano.nam"), doPrewarm=False)
    counts = (1031, 1030, 1029)
    rng = np.random.default_rng(5)
    total = 128 * 3 + 64
    base = (0.3 * rng.standard_normal((7, total))).clip(-1, 1).astype(np.float32)
    x = base[np.arange(sum(counts)) % 7]
    ys = []
    for on in (True, False):
        spec_switch(on)
        b = na.Batch(0)
        for m, c in zip((lite, feather, nano), counts):
            b.AddStreams(m, c)
        assert [b.StreamPackFactor(s) for s in (0, counts[0], counts[0] + counts[1])] == [1, 2, 4]
        ys.append(_run(b, x, [128, 128, 64, 128]))
        b.close()
    spec_switch(True)
    assert np.array_equal(ys[0], ys[1]), float(np.abs(ys[0] - ys[1]).max())
    oracles = [lambda: O.OracleWaveNet(arrays, w), lambda: O.oracle_from_file("BossWN-feather.nam"), lambda: O.oracle_from_file("BossWN-nano.nam")]
    start = 0
    for k, c in enumerate(counts):
        for s in (start, start + c - 1):
            assert O.rms(ys[0][s] - oracles[k]().process(x[s])) < TOL_RMS, (k, s)
        start += c


@pytest.mark.skipif(FORCED, reason="forced kernel family")
@pytest.mark.parametrize("streams", [1, 1024, 4096])
def test_default_kernel_family_and_pack_factor_of_every_official_architecture(na, loader, streams):
    lite, _, _ = _lite(loader)
    a2 = loader.CreateFromFile(_path("BossWN-a2.nam"), doPrewarm=False)
    expect = {
        "standard": ("WaveNetSpecKernel", 1),
        "lite": ("WaveNetSpecKernel", 1),                                            # padded to 16 / 8 channels
        "feather": ("WaveNetSpecKernel", 2),                                         # narrow static models always run packed
        "nano": ("WaveNetSpecKernel", 4),
        "a2": ("WaveNetSpecKernel", 1),
        "lstm1x16": ("RecurrentDppKernel", 1),
        "lstm2x8": ("RecurrentDppKernel", 1),
    }
    models = {"standard": loader.CreateFromFile(_path("BossWN-standard.nam"), doPrewarm=False), "lite": lite,
              "feather": loader.CreateFromFile(_path("BossWN-feather.nam"), doPrewarm=False),
              "nano": loader.CreateFromFile(_path("BossWN-nano.nam"), doPrewarm=False), "a2": a2,
              "lstm1x16": loader.CreateFromFile(_path("BossLSTM-1x16.nam"), doPrewarm=False),
              "lstm2x8": loader.CreateFromFile(_path("BossLSTM-2x8.nam"), doPrewarm=False)}
    for name, m in models.items():
        b = na.Batch(0)
        b.AddStreams(m, streams, doPrewarm=False)
        got = (b.StreamKernelName(0), b.StreamPackFactor(0))
        want = expect[name]
        if name == "lstm1x16" and streams > 2048:
            want = ("RecurrentQuadKernel", 1)  # one-layer LSTMs in launches of thousands of streams: four streams per wave
        assert got == want, (name, streams, got)
        assert (b.StreamKernelName(streams - 1), b.StreamPackFactor(streams - 1)) == got
        b.close()


def _quiet_errors(na, loader, which, amp):
    """error of the GPU path and of the f32 CPU oracle against a float64 evaluation, split into its constant (DC) and varying (AC) parts"""
    m, make_oracle = _models(loader, which)
    ora = make_oracle()
    n = 2048
    x = (amp * np.sin(0.013 * np.arange(n)) + 0.3 * amp * np.sin(0.31 * np.arange(n))).astype(np.float32)
    truth, _ = ref_np.wavenet_forward(ora.arrays, ora.weights, x)
    quiet, _ = ref_np.wavenet_forward(ora.arrays, ora.weights, np.zeros(n, dtype=np.float32))
    signal = O.rms(truth - quiet)
    b = na.Batch(0)
    b.AddStreams(m, 1)
    y = _run(b, x[None, :], [128] * (n // 128))[0]
    b.close()
    yo = ora.process(x)

    def parts(v):
        e = v.astype(np.float64) - truth
        return abs(float(e.mean())), O.rms(e - e.mean())
    return parts(y), parts(yo), signal


@pytest.mark.skipif(FORCED, reason="forced kernel family")
@pytest.mark.parametrize("which", ["standard", "lite"])
@pytest.mark.parametrize("amp", [1e-3, 1e-4, 1e-5, 1e-6])
def test_quiet_inputs_keep_the_absolute_noise_floor_of_the_split_arithmetic(na, loader, which, amp):
    """A split value carries 22 mantissa bits (f32: 24) and f16 subnormals bound its ABSOLUTE precision at 3e-8, so the concern is that
    quiet passages lose relative precision.  Measured (tools/scratch/dbg_quiet.py): the error against a float64 evaluation
    does not depend on the input level at all -- A1 Standard 2.4e-7 RMS at every amplitude from 0.3 to 1e-6 (f32 frame kernel 6e-8,
    f32 CPU oracle 4e-8: the 4x of the two missing bits), Lite 2.5e-9 on all three.  Stated bound, tested here: at most 5e-7 RMS
    (46 dB inside the 1e-4 north-star tolerance) and at most 8x the f32 oracle's error plus 1e-8, constant offset at most 2e-7."""
    (g_dc, g_ac), (o_dc, o_ac), signal = _quiet_errors(na, loader, which, amp)
    assert g_ac <= 5e-7 and g_ac <= 8.0 * o_ac + 1e-8 and g_dc <= 2e-7, (which, amp, g_dc, g_ac, o_dc, o_ac, signal)


@pytest.mark.skipif(FORCED, reason="forced kernel family")
@pytest.mark.parametrize("bad", [65504.0, 1e5, 3e38, float("inf"), float("-inf"), float("nan")])
def test_out_of_range_samples_are_clamped_and_the_stream_recovers(na, loader, bad):
    """Contract of the f16-split path: samples are clamped to +-condLimit (a per-model bound <= 32752 under which no split value
    overflows), NaN reads as silence.  So the output stays finite where the reference's f32 chain stays finite, and one receptive
    field (4092 frames) after the last bad sample the stream is bit-identical to one that was fed the clamped values."""
    m = loader.CreateFromFile(_path("BossWN-standard.nam"), doPrewarm=False)
    rng = np.random.default_rng(3)
    n = 128 * 40
    x = (0.3 * rng.standard_normal(n)).clip(-1, 1).astype(np.float32)
    xb = x.copy()
    xb[100:140] = bad
    xb[300] = -bad if np.isfinite(bad) else bad
    b = na.Batch(0)
    b.AddStreams(m, 1, doPrewarm=False)
    limit = b.StreamInputLimit(0)
    b.close()
    assert 1000.0 < limit <= 32752.0, limit
    xc = np.nan_to_num(xb, nan=0.0, posinf=limit, neginf=-limit).clip(-limit, limit).astype(np.float32)
    ys = []
    for sig in (xb, xc):
        b = na.Batch(0)
        b.AddStreams(m, 1)
        ys.append(_run(b, sig[None, :], [128] * 40)[0])
        b.close()
    assert np.all(np.isfinite(ys[0])), bad
    tail = 301 + 4092
    assert np.array_equal(ys[0][tail:], ys[1][tail:])
    # and the clean part before the bad samples matches the oracle
    assert O.rms(ys[0][:100] - O.oracle_from_file("BossWN-standard.nam").process(x)[:100]) < TOL_RMS
    # inside the limit nothing is clamped: a burst just below it still matches the f32 oracle (relative to its output level)
    if bad == 65504.0:
        xh = x.copy()
        xh[100:140] = np.float32(0.95 * limit)
        b = na.Batch(0)
        b.AddStreams(m, 1)
        yh = _run(b, xh[None, :], [128] * 40)[0]
        yo = O.oracle_from_file("BossWN-standard.nam").process(xh)
        assert O.rms(yh - yo) < 2e-5 * max(1.0, O.rms(yo))  # (values of 3e4 carry 7e-3 absolute error at 22 bits, 2e-3 at 24)


@pytest.mark.skipif(FORCED, reason="forced kernel family")
def test_layout_does_not_depend_on_the_add_pattern_and_slots_are_recycled(na, loader):
    """4096 Nano streams added ONE BY ONE run packed like one bulk add (same pack factor, same kernel, same outputs, same speed class);
    streams that leave free their positions inside the virtual streams, later joins recycle ids and positions and start from a fresh
    prewarmed state while their neighbours carry on."""
    import time
    m = loader.CreateFromFile(_path("BossWN-nano.nam"), doPrewarm=False)
    S = 4096
    rng = np.random.default_rng(9)
    base = (0.3 * rng.standard_normal((5, 128 * 3))).clip(-1, 1).astype(np.float32)
    x = base[np.arange(S) % 5]
    one = na.Batch(0)
    for s in range(S):
        assert one.AddStreams(m, 1) == s
    bulk = na.Batch(0)
    bulk.AddStreams(m, S)
    assert one.StreamPackFactor(0) == one.StreamPackFactor(S - 1) == bulk.StreamPackFactor(0) == 4
    assert one.StreamKernelName(S - 1) == bulk.StreamKernelName(0) == "WaveNetSpecKernel"
    assert one.StateBytes() == bulk.StateBytes()
    ya, yb = _run(one, x, [128, 128, 128]), _run(bulk, x, [128, 128, 128])
    assert np.array_equal(ya, yb)

    def timed(b):
        xb = np.ascontiguousarray(x[:, :128])
        for _ in range(5):
            b.Process(xb)
        t0 = time.perf_counter()
        for _ in range(20):
            b.Process(xb)
        return (time.perf_counter() - t0) / 20
    ta, tb = timed(one), timed(bulk)
    assert ta < 1.25 * tb + 50e-6, (ta, tb)  # (host-buffer calls: copies dominate; the launches are the same)
    bulk.close()

    # leave / rejoin: ids 5, 6 (positions 1, 2 of virtual stream 1), a whole virtual stream (8..11), and the last id
    b = one
    fresh = O.oracle_from_file("BossWN-nano.nam")
    keep = O.oracle_from_file("BossWN-nano.nam")
    keep.process(x[4][:384])
    keep.process(x[4][:128])  # (stream 4 also went through the 25 timing buffers of x[:, :128])
    for _ in range(24):
        keep.process(x[4][:128])
    b.RemoveStreams(5, 2)
    b.RemoveStreams(8, 4)
    b.RemoveStreams(S - 1, 1)
    assert b.NumStreams() == S - 1 and b.NumLiveStreams() == S - 7
    assert b.AddStreams(m, 1) == 5 and b.AddStreams(m, 4) == 8 and b.AddStreams(m, 1) == 6 and b.AddStreams(m, 2) == S - 1
    assert b.NumStreams() == S + 1 and b.NumLiveStreams() == S + 1
    x2 = (0.3 * rng.standard_normal((S + 1, 128))).clip(-1, 1).astype(np.float32)
    y2 = b.Process(x2)
    for s in (5, 6, 8, 11, S - 1, S):
        assert O.rms(y2[s] - O.oracle_from_file("BossWN-nano.nam").process(x2[s])) < TOL_RMS, s  # recycled: fresh prewarmed state
    assert O.rms(y2[4] - keep.process(x2[4])) < TOL_RMS  # the neighbour in virtual stream 1 never noticed


def _process_blocks(batch, x, block=128):
    return np.concatenate([batch.Process(np.ascontiguousarray(x[None, a:a + block]))[0] for a in range(0, x.size, block)])


@pytest.mark.skipif(FORCED, reason="forced kernel family")
@pytest.mark.parametrize("case,factors,want", [
    ("as trained", {}, "WaveNetSpecKernel"),
    ("1x1 x 30: smaller input limit, still proven", {"1x1": 30.0}, "WaveNetSpecKernel"),
    ("1x1 x 4000: tanh layers can add more than the f16 range holds", {"1x1": 4000.0}, "WaveNetFrameKernel"),
    ("mix-in x 1e5: weights beyond the operand format", {"mixin": 1e5}, "WaveNetFrameKernel"),
    ("all weights x 1e-3: matrices below the precision floor of the split", {"rechannel": 1e-3, "conv": 1e-3, "mixin": 1e-3, "1x1": 1e-3, "head": 1e-3}, "WaveNetFrameKernel"),
    ("rechannel x 1e-6 against 1x1 x 1e3", {"rechannel": 1e-6, "1x1": 1e3}, "WaveNetFrameKernel"),
])
def test_models_without_a_range_proof_run_on_the_f32_kernel(na, loader, case, factors, want):
    """the f16-split kernels take a model only with a static proof that no value leaves the f16 range for inputs within
    the limit and that its weights fit the (hi, lo) f16 operand format.  A1 Standard with weights scaled from 1e-6 to 4000: whatever
    the proof decides, the stream follows the f32 oracle (relative to the output level), NA_BatchStreamKernelName shows the kernel, and
    the fallback has no input clamp."""
    arrays = O.a1_arrays(16, 8)
    w = O.scale_wavenet_tensors(arrays, O.synth_wavenet_weights(arrays, seed=21), factors)
    m = loader.CreateFromString(O.nam_json_wavenet_generic(arrays, w), ".nam", doPrewarm=True)
    assert m is not None
    b = na.Batch(0)
    b.AddStreams(m, 1)
    assert b.StreamKernelName(0) == want, (case, b.StreamKernelName(0))
    assert (b.StreamInputLimit(0) == float("inf")) == (want == "WaveNetFrameKernel")
    x = O.signal_noise(128 * 12, seed=8)
    y = _process_blocks(b, x)
    yo = O.OracleWaveNet(arrays, w).process(x)
    assert np.all(np.isfinite(y))
    # These models are badly conditioned on purpose (a residual stream of 1e3 .. 1e4 in front of an unsaturated tanh): the f32 oracle
    # itself is only so close to exact arithmetic, so the kernel is held to the oracle's own distance from a float64 evaluation
    # (tests/ref_np.py; the oracle is 0.1 % .. 25 % off on the scaled ones) -- at most 8 x for the 22-bit split values, 4 x for the
    # f32 kernel, whose sums run in another order
    y64, _ = ref_np.wavenet_forward(arrays, w, x)
    g, o, level = O.rms(y - y64), O.rms(yo - y64), O.rms(y64)
    assert level > 0 and g <= (8.0 if want == "WaveNetSpecKernel" else 4.0) * o + 2e-6 * level, (case, g, o, level)
    assert b.StreamRangeEvents(0) == 0
    b.close()


def _a2_style_weights(channels, conv_gain, seed):
    """A2-shaped seeded weights with every layer conv scaled by `conv_gain` and the biases scaled down, so that what the layers do to the
    signal is what the input level makes of it (measured with tests/ref_np.py at conv_gain 4: the residual stream peaks at 49 / 118
    times the input amplitude for 8 / 3 channels, the head accumulator at 137 / 325 times)."""
    arrays = O.a2_arrays(channels)
    w = O.synth_wavenet_weights(arrays, seed=seed)
    return arrays, O.scale_wavenet_tensors(arrays, w, {"conv": conv_gain, "conv_bias": 1e-6, "1x1_bias": 1e-6, "head_bias": 1e-6})


@pytest.mark.skipif(FORCED, reason="forced kernel family")
@pytest.mark.parametrize("channels", [8, 3])
def test_a2_chain_saturates_counts_the_event_and_recovers(na, loader, channels):
    """LeakyReLU chains have no static range proof (the worst case is the product of 23 layers' row sums), so the official A2 shapes run
    with saturating arithmetic: an A2-shaped model whose layers amplify (gain > 1 per layer, 50 .. 300 over the chain) follows the f32
    oracle at audio level; a passage at 3000 x full scale -- inside the input limit, which only covers the linear path of such a model --
    drives the residual stream past 65504: the values are clamped (no inf, no NaN: the rings are not poisoned),
    NA_BatchStreamRangeEvents counts it, and one receptive field after the passage the stream is back on the oracle.  Errors are judged
    against a float64 evaluation (tests/ref_np.py): the amplifying chain multiplies everybody's rounding."""
    arrays, w = _a2_style_weights(channels, 4.0, seed=40 + channels)
    m = loader.CreateFromString(O.nam_json_wavenet_generic(arrays, w), ".nam", doPrewarm=True)
    assert m is not None
    info = m.KernelInfo(1.0, 1)
    assert info["kernel"] == "f16-split" and not info["range_proven"] and info["input_limit"] > 3000.0
    ora = O.OracleWaveNet(arrays, w)
    rf = ora.receptive_field
    assert rf == 6346
    b = na.Batch(0)
    b.AddStreams(m, 1)
    assert b.StreamKernelName(0) == "WaveNetSpecKernel"
    quiet, loud, back = O.signal_noise(128 * 20, seed=3), (3000.0 * O.signal_noise(128 * 4, seed=4)).astype(np.float32), O.signal_noise(128 * 60, seed=5)
    y64, _ = ref_np.wavenet_forward(arrays, w, np.concatenate([quiet, loud, back]))
    t1, t2 = y64[:quiet.size], y64[quiet.size + loud.size:]

    def close(y, o, t):
        g, e, level = O.rms(y - t), O.rms(o - t), O.rms(t)
        return level > 0 and g <= 8.0 * e + 1e-5 * level, (g, e, level)

    y1, o1 = _process_blocks(b, quiet), ora.process(quiet)
    ok, detail = close(y1, o1, t1)
    assert ok, detail
    assert b.StreamRangeEvents(0) == 0
    y2, o2 = _process_blocks(b, loud), ora.process(loud)
    assert np.all(np.isfinite(y2)) and np.all(np.isfinite(o2))
    assert b.StreamRangeEvents(0) > 0, (float(np.abs(o2).max()),)
    y3, o3 = _process_blocks(b, back), ora.process(back)
    assert np.all(np.isfinite(y3))
    tail = ((rf + 127) // 128 + 1) * 128
    ok, detail = close(y3[tail:], o3[tail:], t2[tail:])
    assert ok, detail
    events = b.StreamRangeEvents(0)
    _process_blocks(b, back[:1280])
    assert b.StreamRangeEvents(0) == events  # nothing new once the signal is back at audio level
    # the stage interpreter (other block lengths) saturates and counts the same way
    _process_blocks(b, loud[:300], block=100)
    assert b.StreamRangeEvents(0) > events
    b.close()


@pytest.mark.skipif(FORCED, reason="forced kernel family")
def test_real_a2_model_raises_no_range_events_on_audio(na, loader):
    """The trained A2 container at full-scale input: no value comes near the f16 range (both submodels, 1024 streams)."""
    m = loader.CreateFromFile(_path("BossWN-a2.nam"), doPrewarm=True)
    b = na.Batch(0)
    b.AddStreams(m, 8, quality=0.0)
    b.AddStreams(m, 8, quality=1.0)
    x = np.stack([O.signal_noise(128 * 8, seed=60 + s) * 4.0 for s in range(16)]).clip(-1, 1).astype(np.float32)
    for a in range(0, x.shape[1], 128):
        b.Process(np.ascontiguousarray(x[:, a:a + 128]))
    assert [b.StreamRangeEvents(s) for s in range(16)] == [0] * 16
    b.close()
