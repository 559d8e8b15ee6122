"""The runtime-shaped WaveNet kernels for layer arrays of 17 .. 128 channels (wavenet_generic_kernels.hip: WaveNetGenericKernel<NB, OCC>
up to 64 channels, WaveNetWideKernel above), at the edges of their tiling and at the limits of their number format.

* a seeded architecture fuzz and a fixed list of named edges: channel counts at and just past every 16- and 64-boundary, narrow arrays
  in front of wide ones, one to three arrays, kernel sizes 1 .. 16, dilations around the block length, calls that leave the ring
  cursors off the 16-frame tile grid (tests/wide_cases.py; tests/test_host_cpu.py proves without a GPU that every seed loads);
* every compiled build of the kernels is launched: batches with more streams than the chip has CUs;
* the index-list path of non-contiguous streams, id recycling, wide models beside the other kernel families in one batch;
* the range contract of DESIGN.md 2.5, which these kernels share with the shaped f16-split ones: input clamped at the model's limit, NaN
  reads as silence, LeakyReLU chains saturate and count the event, weights outside the operand format are a load error.
"""
import os

import numpy as np
import pytest

import na_oracle as O
import ref_np
import wide_cases as WC

FORCED = bool(os.environ.get("NA_WN_KERNEL") or os.environ.get("NA_WN_PACK") or os.environ.get("NA_WN_SPEC") or os.environ.get("NA_SP_T")
              or os.environ.get("NA_SP_GEN") or os.environ.get("NA_WN_PAD"))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(FORCED, reason="forced kernel family")]

TOL_RMS = 2e-6  # the suite's WaveNet parity tolerance, relative to the output level above 1
BLOCK = 128


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


@pytest.fixture(scope="module")
def loader(na):
    return na.NeuralModelLoader()


@pytest.fixture(scope="module")
def num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _load(loader, arrays, w, prewarm=True):
    m = loader.CreateFromString(O.nam_json_wavenet_generic(arrays, w), ".nam", doPrewarm=prewarm)
    assert m is not None, arrays
    return m


def _kernel_of(arrays):
    return "WaveNetWideKernel" if WC.max_channels(arrays) > 64 else "WaveNetGenericKernel"


def _run(batch, x, sizes):
    """x: [streams, samples] through calls of the given sizes (the last one cut to what is left)"""
    out, a = [], 0
    for c in sizes:
        c = min(c, x.shape[1] - a)
        if c <= 0:
            break
        out.append(batch.Process(np.ascontiguousarray(x[:, a:a + c])))
        a += c
    assert a == x.shape[1]
    return np.concatenate(out, axis=1)


def _assert_parity(y, yo, what):
    level, err = O.rms(yo), O.rms(y - yo)
    assert np.all(np.isfinite(y)), what
    assert level > 1e-5 and err < TOL_RMS * max(1.0, level), (what, err, level)  # (a silent model cannot pass)


# ---------------------------------------------------------------------------------------------------------- (a) shapes

@pytest.mark.parametrize("seed", range(WC.NUM_FUZZ_SEEDS))
def test_random_wide_architecture_matches_oracle(na, loader, seed):
    arrays, sizes = WC.fuzz_case(seed)
    w = O.synth_wavenet_weights(arrays, seed=seed)
    m = _load(loader, arrays, w)
    ora = O.OracleWaveNet(arrays, w)
    assert m.GetReceptiveFieldSize() == ora.receptive_field
    b = na.Batch(0)
    b.AddStreams(m, 1)
    assert b.StreamKernelName(0) == _kernel_of(arrays), arrays
    x = O.signal_noise(WC.FUZZ_SAMPLES, seed=seed)
    y = _run(b, x[None, :], sizes)[0]
    b.close()
    _assert_parity(y, ora.process(x), arrays)


@pytest.mark.parametrize("channels,act", WC.FIXED_CASES, ids=["-".join(map(str, c)) for c, _ in WC.FIXED_CASES])
def test_named_edge_shapes_match_oracle_whatever_the_call_sizes(na, loader, channels, act):
    """K = [1, 4, 3], d = [128, 129, 1000] in every array (no history at all, the per-tap history path, dilations on both sides of the
    block length): once in whole blocks, once sample by sample for 300 samples and then in 37-sample calls -- the ring cursors leave the
    tile grid at once and wrap at other places -- with the same samples out, bit for bit (a frame's sums do not depend on its block)."""
    arrays = WC.fixed_case(channels, act)
    w = O.synth_wavenet_weights(arrays, seed=sum(channels))
    m = _load(loader, arrays, w)
    x = O.signal_noise(300 + 37 * 20, seed=sum(channels))
    ys = []
    for sizes in ([BLOCK] * 9, [1] * 300 + [37] * 20):
        b = na.Batch(0)
        b.AddStreams(m, 1)
        assert b.StreamKernelName(0) == _kernel_of(arrays)
        ys.append(_run(b, x[None, :], sizes)[0])
        b.close()
    _assert_parity(ys[0], O.OracleWaveNet(arrays, w).process(x), channels)
    assert np.array_equal(ys[0], ys[1]), (channels, float(np.abs(ys[0] - ys[1]).max()))


# ---------------------------------------------------------------------------------------------------------- (b) every build

def _many_streams(na, m, streams, x5, sizes):
    b = na.Batch(0)
    b.AddStreams(m, streams)
    x = x5[np.arange(streams) % x5.shape[0]]
    y = _run(b, x, sizes)
    b.close()
    return x, y


@pytest.mark.parametrize("channels", [24, 32])
def test_both_builds_of_the_32_channel_kernel_match_oracle(na, loader, num_cus, channels):
    """LaunchWaveNetGeneric runs models of 17 .. 32 channels on WaveNetGenericKernel<2, 2> (256 VGPRs) up to one stream per CU and on
    <2, 4> (128 VGPRs, two workgroups per CU) beyond: a batch on each side of the CU count, streams against their oracles, streams with
    the same input bit-identical within a batch.  (Which instantiation ran is decided by the stream count alone; the two are different
    compilations, so whether they agree bitwise is reported, not required.)"""
    arrays = WC.chain([channels], [([3, 3], [1, 64])])
    w = O.synth_wavenet_weights(arrays, seed=channels)
    m = _load(loader, arrays, w)
    x5 = np.stack([O.signal_noise(2 * BLOCK + 37, 30 + s) for s in range(5)])
    yo = [O.OracleWaveNet(arrays, w).process(x5[s]) for s in range(5)]
    small, large = 8, max(300, num_cus + 44)
    assert small <= num_cus < large  # the two branches of the launch
    outs = {}
    for streams in (small, large):
        _, y = _many_streams(na, m, streams, x5, [BLOCK, BLOCK, 37])
        outs[streams] = y
        for s in (0, streams // 3, (2 * streams) // 3, streams - 1):
            _assert_parity(y[s], yo[s % 5], (channels, streams, s))
        for s in range(5, streams):
            assert np.array_equal(y[s], y[s % 5]), (channels, streams, s)
    print("channels %d: <2,2> (%d streams) and <2,4> (%d streams) agree bitwise: %s" % (channels, small, large, np.array_equal(outs[small][:5], outs[large][:5])))


def test_a_wide_model_grid_larger_than_the_chip_matches_oracle(na, loader, num_cus):
    """65 channels: WaveNetWideKernel, one workgroup per CU -- four streams more than CUs, so the last workgroups start when others end"""
    arrays = WC.chain([65], [([2], [1])])
    w = O.synth_wavenet_weights(arrays, seed=65)
    m = _load(loader, arrays, w)
    x5 = np.stack([O.signal_noise(2 * BLOCK + 37, 40 + s) for s in range(5)])
    streams = num_cus + 4
    _, y = _many_streams(na, m, streams, x5, [BLOCK, BLOCK, 37])
    for s in (0, streams // 3, (2 * streams) // 3, streams - 1):
        _assert_parity(y[s], O.OracleWaveNet(arrays, w).process(x5[s % 5]), s)
    for s in range(5, streams):
        assert np.array_equal(y[s], y[s % 5]), s


# ---------------------------------------------------------------------------------------------------------- (c) index lists

@pytest.mark.parametrize("channels", [40, 96])
def test_wide_streams_leave_and_ids_are_recycled(na, loader, channels):
    """After RemoveStreams the live streams of a group are no longer contiguous: the kernels take slot and row from the index lists."""
    arrays = WC.two_array(channels, channels // 2)
    w = O.synth_wavenet_weights(arrays, seed=channels)
    m = _load(loader, arrays, w)
    b = na.Batch(0)
    assert b.AddStreams(m, 6) == 0
    refs = [O.OracleWaveNet(arrays, w) for _ in range(6)]

    def step(n, tag):
        x = np.stack([O.signal_noise(n, 1000 * tag + s) for s in range(len(refs))])
        y = b.Process(x)
        for s, r in enumerate(refs):
            if r is None:
                assert not np.any(y[s]), (tag, s)  # a retired row reads as silence
            else:
                _assert_parity(y[s], r.process(x[s]), (channels, tag, s))

    step(200, 1)
    b.RemoveStreams(1)
    b.RemoveStreams(3)
    refs[1] = refs[3] = None
    assert b.NumStreams() == 6 and b.NumLiveStreams() == 4 and not b.IsLive(1) and not b.IsLive(3) and b.IsLive(2)
    step(129, 2)
    assert b.AddStreams(m, 1) == 1  # the lowest retired id, with a fresh prewarmed state
    refs[1] = O.OracleWaveNet(arrays, w)
    assert b.NumStreams() == 6 and b.NumLiveStreams() == 5 and b.StreamKernelName(1) == _kernel_of(arrays)
    step(129, 3)
    step(BLOCK, 4)
    b.close()


# ---------------------------------------------------------------------------------------------------------- (d) mixed batches

@pytest.mark.parametrize("seed", range(int(os.environ.get("NA_FUZZ_WIDE_BATCH_SEEDS", "4"))))
def test_wide_models_beside_the_other_families_track_per_stream_oracles(na, loader, seed):
    """Two wide models (groups that launch on their own), A1 Standard (split launch), Nano x 5 (packed launch) and an LSTM in ONE batch;
    then a walk like test_random_batch_operations_track_per_stream_oracles: joins, leaves, re-prewarms, ragged buffers, every stream
    against its own oracle."""
    rng = np.random.default_rng(900 + seed)
    wide = {"wide40": WC.two_array(40, 20), "wide72": WC.two_array(72, 36)}
    ww = {k: O.synth_wavenet_weights(a, seed=a[0]["channels"]) for k, a in wide.items()}
    files = {"standard": "BossWN-standard.nam", "nano": "BossWN-nano.nam", "lstm": "BossLSTM-2x8.nam"}
    models = {k: _load(loader, a, ww[k], prewarm=False) for k, a in wide.items()}
    models.update({k: loader.CreateFromFile(os.path.join(O.MODELS_DIR, f), doPrewarm=False) for k, f in files.items()})

    def oracle(kind, prewarm):
        return O.OracleWaveNet(wide[kind], ww[kind], prewarm=prewarm) if kind in wide else O.oracle_from_file(files[kind], prewarm=prewarm)

    b = na.Batch(0)
    refs = []  # row -> (kind, oracle), None for a retired id

    def add(kind, count, pre):
        holes = [i for i, r in enumerate(refs) if r is None]
        runs = [h for h in holes if all((h + k) in holes for k in range(count))]
        expect = runs[0] if runs else len(refs)
        first = b.AddStreams(models[kind], count, doPrewarm=pre)
        assert first == expect, (first, expect, holes, count)
        for k in range(count):
            if first + k < len(refs):
                refs[first + k] = (kind, oracle(kind, pre))
            else:
                refs.append((kind, oracle(kind, pre)))

    for kind, count in (("wide40", 2), ("wide72", 2), ("standard", 2), ("nano", 5), ("lstm", 1)):
        add(kind, count, True)
    assert b.StreamKernelName(0) == "WaveNetGenericKernel" and b.StreamKernelName(2) == "WaveNetWideKernel"
    for step in range(12):
        live = [i for i, r in enumerate(refs) if r is not None]
        op = int(rng.integers(0, 4))
        if op == 0:
            add(str(rng.choice(list(models))), int(rng.integers(1, 3)), bool(rng.integers(0, 2)))
        elif op == 1:
            i = int(rng.choice(live))
            b.Prewarm(i)
            refs[i][1].prewarm()
        elif op == 2 and len(live) > 6:
            i = int(rng.choice(live))
            b.RemoveStreams(i, 1)
            refs[i] = None
            while refs and refs[-1] is None:
                refs.pop()
            assert b.NumStreams() == len(refs) and b.NumLiveStreams() == sum(r is not None for r in refs)
        n = int(rng.choice([1, 15, 17, 64, 128, 129, 300]))
        x = np.stack([O.signal_noise(n, 20000 * seed + 100 * step + s) for s in range(len(refs))])
        y = b.Process(x)
        for s, r in enumerate(refs):
            if r is None:
                assert not np.any(y[s]), (step, s)
                continue
            err = O.rms(y[s] - r[1].process(x[s]))
            assert err < 5e-6, (step, s, r[0], err)
    assert any(r is not None and r[0] in wide for r in refs)
    b.close()


# ---------------------------------------------------------------------------------------------------------- (e) range contract

def _range_model(loader, name):
    arrays, w = WC.range_model(name)
    return _load(loader, arrays, w), arrays, w


def _blocks(batch, x):
    return _run(batch, x[None, :], [BLOCK] * ((x.size + BLOCK - 1) // BLOCK))[0]


def _float64_bound(y, yo, y64, what):
    """The kernel is held to the f32 oracle's own distance from a float64 evaluation: at most 8 x for the 22-bit split values
    (test_models_without_a_range_proof_run_on_the_f32_kernel)."""
    g, o, level = O.rms(y - y64), O.rms(yo - y64), O.rms(y64)
    print("%s: kernel %.3g, f32 oracle %.3g from float64, level %.3g" % (what, g, o, level))
    assert np.all(np.isfinite(y)), what
    assert level > 0 and g <= 8.0 * o + 2e-6 * level, (what, g, o, level)


@pytest.mark.parametrize("amp", [30.0, 1000.0, 10000.0])
@pytest.mark.parametrize("name", ["32/8 tanh", "128/64 tanh", "24/12 leaky", "128/128 leaky"])
def test_hot_inputs_inside_the_range_follow_the_float64_reference(na, loader, name, amp):
    """Inputs far above full scale that keep every split value under half the f16 range (test_host_cpu.py proves that they do): nothing
    is clamped, nothing saturates."""
    m, arrays, w = _range_model(loader, name)
    x = (amp * O.signal_noise(1024, 5)).astype(np.float32)
    b = na.Batch(0)
    b.AddStreams(m, 1)
    assert np.abs(x).max() < b.StreamInputLimit(0)
    y = _blocks(b, x)
    y64, _ = ref_np.wavenet_forward(arrays, w, x)
    _float64_bound(y, O.OracleWaveNet(arrays, w).process(x), y64, (name, amp))
    assert b.StreamRangeEvents(0) == 0
    b.close()


@pytest.mark.parametrize("bad", [65504.0, 1e5, 3e38, float("inf"), float("-inf"), float("nan")])
@pytest.mark.parametrize("name", ["32/8 tanh", "80/72 tanh", "24/12 leaky"])
def test_out_of_range_samples_are_clamped_and_the_wide_stream_recovers(na, loader, name, bad):
    """test_out_of_range_samples_are_clamped_and_the_stream_recovers for the runtime-shaped kernels: samples are clamped to the model's
    input limit, NaN reads as silence; the output stays finite, and from one receptive field after the last bad sample (rounded up to
    the next block) the stream is bit-identical to one that was fed the clamped values.

    A LeakyReLU chain has no range proof: its limit covers the rechannel path, and the burst at 0.95 x limit drives the head accumulator
    of the 24 / 12 model to 91 492 (residual stream 56 534, activations 45 512: tests/ref_np.py).  The head mat-mul takes such a frame
    with a block exponent (wavenet_generic_kernels.hip HeadExponent), so the burst still matches the oracle; the range event is counted.
    """
    m, arrays, w = _range_model(loader, name)
    ora = O.OracleWaveNet(arrays, w)
    n = BLOCK * 12
    x = O.signal_noise(n, 3)
    xb = x.copy()
    xb[100:140] = bad
    xb[300] = -bad if np.isfinite(bad) else bad
    b = na.Batch(0)
    b.AddStreams(m, 1, doPrewarm=False)
    limit = b.StreamInputLimit(0)
    b.close()
    assert 8.0 <= limit <= 32752.0, limit  # (kSplitMinInputLimit; half the f16 range)
    assert m.KernelInfo(1.0, 1)["input_limit"] == limit
    xc = np.nan_to_num(xb, nan=0.0, posinf=limit, neginf=-limit).clip(-limit, limit).astype(np.float32)
    ys = []
    for sig in (xb, xc):
        b = na.Batch(0)
        b.AddStreams(m, 1)
        ys.append(_blocks(b, sig))
        b.close()
    assert np.all(np.isfinite(ys[0])), (name, bad)
    tail = ((301 + ora.receptive_field + BLOCK - 1) // BLOCK) * BLOCK
    assert tail + BLOCK <= n
    assert np.array_equal(ys[0][tail:], ys[1][tail:]), (name, bad)
    yo = ora.process(x)
    assert O.rms(ys[0][:100] - yo[:100]) < TOL_RMS * max(1.0, O.rms(yo[:100]))
    if bad == 65504.0:  # inside the limit nothing is clamped: a burst just below it still matches the f32 oracle
        xh = x.copy()
        xh[100:140] = np.float32(0.95 * limit)
        b = na.Batch(0)
        b.AddStreams(m, 1)
        yh = _blocks(b, xh)
        events = b.StreamRangeEvents(0)
        b.close()
        yo = O.OracleWaveNet(arrays, w).process(xh)
        print("%s: burst at 0.95 x %g: %.3g from the oracle, level %.3g, %d range events" % (name, limit, O.rms(yh - yo), O.rms(yo), events))
        assert O.rms(yh - yo) < 2e-5 * max(1.0, O.rms(yo))


@pytest.mark.parametrize("name", ["128/128 leaky", "24/12 leaky"])
def test_wide_leakyrelu_chain_saturates_counts_the_event_and_recovers(na, loader, name):
    """LeakyReLU chains have no static range proof.  A passage at 6e4 x noise -- clamped at the input limit, and still beyond 65 504
    (test_host_cpu.py: the head accumulator of both models, residual stream and activations of the 128-channel one) -- leaves the f16
    range: operands saturate, the head accumulator takes a block exponent, no inf, no NaN, the event is counted, and one receptive
    field (plus a block) after it the stream is back on the oracle."""
    m, arrays, w = _range_model(loader, name)
    ora = O.OracleWaveNet(arrays, w)
    rf = ora.receptive_field
    b = na.Batch(0)
    b.AddStreams(m, 1)
    quiet, loud, back = O.signal_noise(BLOCK * 4, 3), (6e4 * O.signal_noise(BLOCK * 4, 4)).astype(np.float32), O.signal_noise(BLOCK * 12, 5)
    y64, _ = ref_np.wavenet_forward(arrays, w, np.concatenate([quiet, loud, back]))
    t1, t2 = y64[:quiet.size], y64[quiet.size + loud.size:]

    def close(y, o, t):
        g, e, level = O.rms(y - t), O.rms(o - t), O.rms(t)
        return level > 0 and g <= 8.0 * e + 1e-5 * level, (g, e, level)

    y1, o1 = _blocks(b, quiet), ora.process(quiet)
    ok, detail = close(y1, o1, t1)
    assert ok, detail
    assert b.StreamRangeEvents(0) == 0
    y2, o2 = _blocks(b, loud), ora.process(loud)
    assert np.all(np.isfinite(y2)) and np.all(np.isfinite(o2))
    assert b.StreamRangeEvents(0) > 0, (float(np.abs(o2).max()),)
    y3, o3 = _blocks(b, back), ora.process(back)
    assert np.all(np.isfinite(y3))
    tail = ((rf + BLOCK - 1) // BLOCK + 1) * BLOCK
    assert tail + BLOCK <= back.size
    ok, detail = close(y3[tail:], o3[tail:], t2[tail:])
    assert ok, detail
    events = b.StreamRangeEvents(0)
    _blocks(b, back[:BLOCK * 4])
    assert b.StreamRangeEvents(0) == events  # nothing new once the signal is back at audio level
    b.close()


@pytest.mark.parametrize("name", ["32/8 tanh", "80/72 tanh"])
def test_wide_models_outside_the_operand_format_never_run(na, loader, name):
    """There is no f32 kernel for these widths: a model that cannot be run is a load error (test_host_cpu.py pins the messages), and
    one that loads follows the float64 reference -- never a silent NaN."""
    arrays, w = WC.range_model(name)
    x = O.signal_noise(BLOCK * 8, seed=8)
    cases = dict(WC.WEIGHT_SCALINGS)
    cases["1x1 x 30"] = {"1x1": 30.0}  # (a scaling that still loads: a smaller input limit)
    loaded = 0
    for case, factors in cases.items():
        ws = O.scale_wavenet_tensors(arrays, w, factors)
        try:
            m = loader.CreateFromString(O.nam_json_wavenet_generic(arrays, ws), ".nam")
        except na.NeuralAudioError as e:
            assert "wider than 16 channels" in str(e), (case, str(e))
            continue
        loaded += 1
        b = na.Batch(0)
        b.AddStreams(m, 1)
        y = _blocks(b, x)
        y64, _ = ref_np.wavenet_forward(arrays, ws, x)
        _float64_bound(y, O.OracleWaveNet(arrays, ws).process(x), y64, (name, case))
        assert b.StreamRangeEvents(0) == 0
        b.close()
    assert loaded >= 1


@pytest.mark.parametrize("amp", [1e-3, 1e-5, 1e-6])
@pytest.mark.parametrize("name", ["32/8 tanh", "128/64 tanh"])
def test_quiet_inputs_keep_the_noise_floor_on_wide_models(na, loader, name, amp):
    """_quiet_errors of test_gpu_spec.py on the runtime-shaped kernels: the error against a float64 evaluation, split into its constant
    and its varying part, at most 8 x the f32 oracle's own plus 1e-8, constant offset at most 2e-7 (measured figures: DESIGN.md 2.2)."""
    m, arrays, w = _range_model(loader, name)
    n = 2048
    x = (amp * np.sin(0.013 * np.arange(n)) + 0.3 * amp * np.sin(0.31 * np.arange(n))).astype(np.float32)
    truth, _ = ref_np.wavenet_forward(arrays, w, x)
    b = na.Batch(0)
    b.AddStreams(m, 1)
    y = _blocks(b, x)
    b.close()
    yo = O.OracleWaveNet(arrays, w).process(x)

    def parts(v):
        e = v.astype(np.float64) - truth
        return abs(float(e.mean())), O.rms(e - e.mean())
    (g_dc, g_ac), (o_dc, o_ac) = parts(y), parts(yo)
    print("%s amp %g: kernel AC %.3g DC %.3g, f32 oracle AC %.3g DC %.3g" % (name, amp, g_ac, g_dc, o_ac, o_dc))
    assert g_ac <= 8.0 * o_ac + 1e-8 and g_dc <= 2e-7, (name, amp, g_dc, g_ac, o_dc, o_ac)
