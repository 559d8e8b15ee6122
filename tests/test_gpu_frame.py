"""The f32 frame kernel (wavenet_frame_kernels.hip: WaveNetFrameKernel) where default loads land on it: every WaveNet of at most 16
channels with a layer kernel size other than 3, a conv head, or no f16 range proof (tests/frame_cases.py; tests/test_host_cpu.py proves
without a GPU that every case loads and is predicted to run here).

* (a) named edges and a seeded fuzz, single stream: every channel-group count with partially filled groups, tap shifts on both sides
  of 64 and 128 frames, both prefetch depths, staged weight blocks beyond the stager's fixed copy, conv heads on both sides of the reach
  that picks their kernel, ring cursors off the tile grid;
* (b) two streams per workgroup and the shadow wave of a half-filled last workgroup, which writes no row beyond the batch;
* (c) slot / row tables and id recycling;
* (d) nine different models in one batch: fused launches of eight groups plus one, with different kernel sizes and staged blocks;
* (e) the LDS limit: kernel sizes that leave room for one stream per workgroup only, and the size that is refused at load.

Every test asserts NA_BatchStreamKernelName before it trusts a comparison.  Parity: against the f32 oracle, the suite's WaveNet tolerance
(2e-6 RMS, relative to the output level above 1) on EVERY 32-frame window of the output -- one wrong frame of 1.2e-5 fails; the project
records 6e-8 RMS for this kernel on trained models (test_gpu_spec.py).  Cases that are badly conditioned on purpose (frame_cases.RULE_F64:
weights scaled until the range proof fails) are held to a float64 evaluation instead, over the whole signal: at most 4 x the f32 oracle's
own distance plus 2e-6 of the level (test_models_without_a_range_proof_run_on_the_f32_kernel).  Which rule a case uses is fixed in
frame_cases.py.  NA_FR_PF / NA_FR_SPB do not skip this file: tests/test_gpu_families.py runs it under them.

Measured on an MI355X (default knobs, against O.OracleWaveNet): the worst 32-frame window of any case is 0.0021 of the
2e-6 bound (4e-9 RMS); the model without a range proof is 0.0084 from float64 where the f32 oracle is 0.0092 (level 0.038); the bit-identities asserted below (block lengths, streams per workgroup, 511 / 512 / 513 streams) all hold."""
import os

import numpy as np
import pytest

import frame_cases as FC
import na_oracle as O
import ref_np

FORCED = bool(os.environ.get("NA_WN_KERNEL") or os.environ.get("NA_WN_PACK") or os.environ.get("NA_WN_SPEC") or os.environ.get("NA_SP_T")
              or os.environ.get("NA_SP_GEN") or os.environ.get("NA_WN_PAD"))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(FORCED, reason="forced kernel family")]

TOL_RMS = 2e-6  # the suite's WaveNet parity tolerance, relative to the output level above 1
WINDOW = 32
BLOCK = FC.BLOCK
KERNEL = "WaveNetFrameKernel"
NAMED = FC.named_cases()


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


@pytest.fixture(scope="module")
def loader(na):
    return na.NeuralModelLoader()


def _load(loader, case, prewarm=True):
    w = FC.weights(case)
    m = loader.CreateFromString(O.nam_json_wavenet_generic(case["arrays"], w), ".nam", doPrewarm=prewarm)
    assert m is not None, case["name"]
    return m, w


def _batch(na, m, streams, what):
    b = na.Batch(0)
    assert b.AddStreams(m, streams) == 0
    assert b.StreamKernelName(0) == KERNEL and b.StreamKernelName(streams - 1) == KERNEL, (what, b.StreamKernelName(0))
    return b


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


def _assert_windows(y, yo, what):
    """the parity rule: every 32-frame window (a shorter last one included) within TOL_RMS of the oracle, relative to its level above 1"""
    assert y.shape == yo.shape and np.all(np.isfinite(y)), what
    assert O.rms(yo) > 1e-5, (what, O.rms(yo))  # (a silent model cannot pass)
    worst = 0.0
    for a in range(0, y.size, WINDOW):
        err, level = O.rms(y[a:a + WINDOW] - yo[a:a + WINDOW]), O.rms(yo[a:a + WINDOW])
        worst = max(worst, err / max(1.0, level))
        assert err < TOL_RMS * max(1.0, level), (what, "window at", a, err, level)
    return worst


def _assert_float64(y, yo, y64, what):
    g, o, level = O.rms(y - y64), O.rms(yo - y64), O.rms(y64)
    print("%s: kernel %.3g, f32 oracle %.3g from float64, level %.3g" % (what, g, o, level))
    assert np.all(np.isfinite(y)) and level > 1e-5, (what, level)
    assert g <= 4.0 * o + 2e-6 * level, (what, g, o, level)


def _assert_case(case, w, x, y, yo, what):
    if case["rule"] == FC.RULE_F64:
        y64, _ = ref_np.wavenet_forward(case["arrays"], w, x)
        _assert_float64(y, yo, y64, what)
    else:
        print("%s: worst window %.3g of the bound" % (what, _assert_windows(y, yo, what) / TOL_RMS))


# ---------------------------------------------------------------------------------------------------------- (a) single stream

@pytest.mark.parametrize("case", NAMED, ids=[c["name"] for c in NAMED])
def test_named_frame_kernel_edges_match_oracle_whatever_the_call_sizes(na, loader, case):
    """Every named case of frame_cases.py twice: in whole 128-frame blocks, and as 40 .. 76 single samples followed by 37-sample calls --
    the ring cursors leave the 16-frame tile grid at once and wrap at other places.  Both runs are held to the parity rule, and they are
    bit-identical: buffers of at most 64 frames run Launch<1, 0, 1> (one wave, no prefetch) and longer ones Launch<2, 1, *> (two waves,
    history prefetched into registers), but a frame's sums are the same chain in both -- bias + mix-in, the taps in ascending order through
    the same MFMA sequence whether their operand came from the prefetch, the ring or the LDS image, then the 1x1 -- and the head conv
    (HeadConvLds / HeadConvPk) is chosen by the model's reach, not by the block."""
    m, w = _load(loader, case)
    x = O.signal_noise(case["samples"], seed=case["seed"])
    ora = O.OracleWaveNet(case["arrays"], w)
    assert m.GetReceptiveFieldSize() == ora.receptive_field
    yo = ora.process(x)
    n37 = (x.size - 40) // 37
    ys = []
    for sizes in ([BLOCK] * (x.size // BLOCK), [1] * (x.size - 37 * n37) + [37] * n37):
        b = _batch(na, m, 1, case["name"])
        ys.append(_run(b, x[None, :], sizes)[0])
        b.close()
        _assert_case(case, w, x, ys[-1], yo, (case["name"], case["path"], sizes[0]))
    assert np.array_equal(ys[0], ys[1]), (case["name"], float(np.abs(ys[0] - ys[1]).max()))


@pytest.mark.parametrize("seed", range(FC.NUM_FUZZ_SEEDS))
def test_random_frame_kernel_architecture_matches_oracle(na, loader, seed):
    """The seeded draw over the same families, through call sizes that start 1, 1, 17, mix sizes around the wave and the block length
    with sizes the host cuts, and wrap every ring at least twice."""
    case, sizes = FC.fuzz_case(seed)
    m, w = _load(loader, case)
    x = O.signal_noise(case["samples"], seed=case["seed"])
    b = _batch(na, m, 1, case["arrays"])
    y = _run(b, x[None, :], sizes)[0]
    b.close()
    _assert_case(case, w, x, y, O.OracleWaveNet(case["arrays"], w).process(x), (case["name"], case["family"], case["arrays"]))


# ---------------------------------------------------------------------------------------------------------- (b) streams per workgroup

def _base_rows(streams, samples, seed):
    base = np.stack([O.signal_noise(samples, seed + r) for r in range(7)])
    return base, base[np.arange(streams) % 7]


def test_two_streams_per_workgroup_and_the_shadow_wave_compute_what_one_stream_per_workgroup_computes(na, loader):
    """From 512 streams on a launch of more than 64 frames puts two streams into a workgroup (Launch<2, 1, 2>); 513 streams leave the
    last workgroup half filled: its surplus waves shadow the last stream -- they stage weights and meet barriers -- and must write neither
    output nor ring nor cursor.  Buffers of 128, 64, 128, 65, 128 frames alternate that launch with the one-wave launch of short buffers
    (Launch<1, 0, 1>, one stream per workgroup) on one stream state; 511 streams run one stream per workgroup throughout.  (That is the
    default; tests/test_gpu_families.py also runs this file under NA_FR_SPB=4, where both batches put four streams into a workgroup of
    the long launch and 513 leave three shadowing waves, and under NA_FR_PF=0, where every launch has one.  The assertions hold alike.)
    Rows with equal input are bit-identical within a batch and between the batches (the arithmetic does not depend on the streams per
    workgroup), first, last and a middle stream follow their oracles window by window, and after two streams left the 513-stream batch
    their rows read as silence while their neighbours carry on.  A host array has no rows beyond the batch: that the shadowing waves
    write none is the next test's, on a device array."""
    case = FC.small_k2_model()
    m, w = _load(loader, case)
    sizes = [BLOCK, 64, BLOCK, 65, BLOCK]
    base, _ = _base_rows(7, sum(sizes) + BLOCK, 50)
    yo = [O.OracleWaveNet(case["arrays"], w).process(base[r]) for r in range(7)]
    outs = {}
    for streams in (513, 511):
        x = base[np.arange(streams) % 7]
        b = _batch(na, m, streams, streams)
        y = _run(b, x[:, :sum(sizes)], sizes)
        for s in range(7, streams):
            assert np.array_equal(y[s], y[s % 7]), (streams, s)
        for s in (0, streams // 2, streams - 2, streams - 1):
            _assert_windows(y[s], yo[s % 7][:sum(sizes)], (streams, s))
        if streams == 513:
            b.RemoveStreams(100)
            b.RemoveStreams(300)
            assert b.NumStreams() == 513 and b.NumLiveStreams() == 511
            y2 = b.Process(np.ascontiguousarray(x[:, sum(sizes):]))
            assert not np.any(y2[100]) and not np.any(y2[300])
            y = np.concatenate([y, y2], axis=1)
            for s in (0, 99, 101, 299, 301, 512):
                _assert_windows(y[s], yo[s % 7], ("after two streams left", s))
        outs[streams] = y
        b.close()
    assert np.array_equal(outs[513][:511, :sum(sizes)], outs[511])


GUARD, SENTINEL = 4, 12345.0


def _build_guarded(which, batch, models):
    """-> kind: kind[s] is the model of row s, None for a retired row"""
    if which == "513":
        assert batch.AddStreams(models[0][0], 513) == 0
        kind, gone = [0] * 513, []  # (contiguous: the kernel takes row0 + index, no tables; a stream that left would drop it below 512)
    else:
        for s in range(521):
            assert batch.AddStreams(models[s % 2][0], 1) == s
        kind, gone = [s % 2 for s in range(521)], [7, 8, 300, 302, 520]  # leaves 257 and 259 streams: two odd groups
    for s in gone:
        batch.RemoveStreams(s)
        kind[s] = None
    while kind[-1] is None:
        kind.pop()  # (a retired tail row leaves the arrays)
    assert batch.NumStreams() == len(kind) and batch.NumLiveStreams() == sum(k is not None for k in kind) >= 512
    for s in (0, 1, len(kind) - 2, len(kind) - 1):
        assert batch.StreamKernelName(s) == KERNEL, (which, s, batch.StreamKernelName(s))
    return kind


@pytest.mark.parametrize("which", ["513", "521"], ids=["one-model-513", "two-models-521"])
def test_rows_outside_the_batch_and_retired_rows_of_a_device_array_are_never_written(na, loader, which):
    """What NA_BatchProcess cannot show, because its output array has exactly one row per stream: a write past the batch, which is what a
    wrong guard on the half-filled last workgroup would produce.  The batch runs on a caller's HIP stream through NA_BatchProcessDevice
    (the same ordered launches as NA_BatchProcess) into the middle of a device array whose 4 rows in front of the batch, 4 rows behind it
    and retired rows inside it hold a sentinel.  Buffers of 128, 64 and 65 frames: the launch of more than 64 frames (two streams per
    workgroup by default, four under NA_FR_SPB=4; the surplus waves of the last workgroup shadow the last stream), the one-wave launch of
    short buffers (always one stream per workgroup), and a second wave that holds one frame.  One model with 513 contiguous streams
    (rows counted from the group's first, no tables); two interleaved models (slot / row tables) with 520 rows, four retired ones inside
    and an odd number of streams in either group (257 + 259: the launcher counts live streams, and two per workgroup need 512).
    Every sentinel row still holds the sentinel in every buffer -- the device path leaves retired rows untouched, the host path reads
    them as silence -- live rows are bit-identical to NA_BatchProcess on a second batch built the same way, and first and last live
    stream of that one follow their oracles."""
    import torch
    dev = torch.device("cuda", 0)
    ts = torch.cuda.Stream(device=dev)
    host, devb = na.Batch(0), na.Batch(0, hip_stream=ts.cuda_stream)
    cases = [FC.small_k2_model()] if which == "513" else FC.table_models()
    models = [_load(loader, c, prewarm=which == "513") for c in cases]
    kind = _build_guarded(which, host, models)
    assert _build_guarded(which, devb, models) == kind
    rows = len(kind)
    sizes = [BLOCK, 64, 65]
    x = np.ascontiguousarray(_base_rows(rows, sum(sizes), 60)[1], dtype=np.float32)
    want = _run(host, x, sizes)
    xd = torch.from_numpy(x).to(dev)
    got, a = [], 0
    for n in sizes:
        xin = xd[:, a:a + n].contiguous()
        buf = torch.full((GUARD + rows + GUARD, n), SENTINEL, device=dev)
        torch.cuda.synchronize(dev)
        devb.ProcessDevice(xin.data_ptr(), buf[GUARD].data_ptr(), n)
        devb.Synchronize()
        got.append(buf.cpu().numpy())
        a += n
    host.close()
    devb.close()
    got = np.concatenate(got, axis=1)
    live = np.array([k is not None for k in kind])
    assert np.all(got[:GUARD] == SENTINEL) and np.all(got[GUARD + rows:] == SENTINEL), which  # rows in front of and behind the batch
    assert np.all(got[GUARD:GUARD + rows][~live] == SENTINEL) and not np.any(want[~live]), which  # retired rows: untouched / silent
    assert np.array_equal(got[GUARD:GUARD + rows][live], want[live]), which
    for s in (int(np.flatnonzero(live)[0]), int(np.flatnonzero(live)[-1])):
        _assert_windows(want[s], O.OracleWaveNet(cases[kind[s]]["arrays"], models[kind[s]][1]).process(x[s]), (which, s))


# ---------------------------------------------------------------------------------------------------------- (c) index tables

@pytest.mark.parametrize("streams,checked", [(40, None), (521, [0, 1, 4, 7, 8, 299, 300, 301, 302, 518, 519, 520])], ids=["40", "521"])
def test_interleaved_frame_models_leave_and_their_ids_are_recycled(na, loader, streams, checked):
    """Two frame models added alternately, one stream at a time: neither group's slots map to consecutive rows, so the kernel takes slot and
    row from the index tables.  Streams leave from the middle and the end, later joins recycle the ids (the lowest first) with a fresh
    prewarmed state; kept streams continue on their oracles, recycled ones match fresh ones, retired rows read as silence.  521 streams:
    the table path with two streams per workgroup and a half-filled last workgroup in each group (261 and 260 streams, then odd counts
    again after the leaves), a handful of streams checked."""
    cases = FC.table_models()
    models = [_load(loader, c, prewarm=False) for c in cases]
    base, x_all = _base_rows(streams, 5 * BLOCK + 65 + 64 + 37, 70)
    b = na.Batch(0)
    kind = []
    for s in range(streams):
        assert b.AddStreams(models[s % 2][0], 1) == s
        kind.append(s % 2)
    checked = list(range(streams)) if checked is None else checked
    refs = {s: O.OracleWaveNet(cases[kind[s]]["arrays"], models[kind[s]][1]) for s in checked}
    for s in (0, 1, streams - 1):
        assert b.StreamKernelName(s) == KERNEL
    pos = [0]

    def step(n, tag):
        x = x_all[:b.NumStreams(), pos[0]:pos[0] + n]
        pos[0] += n
        y = b.Process(np.ascontiguousarray(x))
        for s in range(b.NumStreams()):
            if kind[s] is None:
                assert not np.any(y[s]), (tag, s)  # a retired row reads as silence
            elif s in refs:
                _assert_windows(y[s], refs[s].process(x[s]), (streams, tag, s))

    step(BLOCK, 1)
    step(37, 2)
    step(65, 3)
    last = streams - 1
    gone = [7, 8, 20 if streams == 40 else 300, last]
    for s in gone:
        b.RemoveStreams(s)
        kind[s] = None
        refs.pop(s, None)
    kind.pop()  # (the tail id is given back)
    assert b.NumStreams() == streams - 1 and b.NumLiveStreams() == streams - 4
    step(BLOCK, 4)
    step(64, 5)
    for want in gone:  # the lowest retired id first, at last a new one at the end; each runs the other model than before
        k = (want + 1) % 2
        assert b.AddStreams(models[k][0], 1) == want
        if want == last:
            kind.append(k)
        else:
            kind[want] = k
        assert b.StreamKernelName(want) == KERNEL
        refs[want] = O.OracleWaveNet(cases[k]["arrays"], models[k][1])
    assert b.NumStreams() == streams and b.NumLiveStreams() == streams
    step(BLOCK, 6)
    step(BLOCK, 7)
    step(BLOCK, 8)
    b.close()


# ---------------------------------------------------------------------------------------------------------- (d) fused launches

def test_nine_different_frame_models_in_one_batch_track_their_oracles(na, loader):
    """Groups of the frame kernel share a launch, eight at a time: nine models make a launch of eight groups and one of one.  Inside the
    first, the largest conv kernel differs per group (3, 6 at two channels, 15 at eight: the five-tap prefetch of narrow runs beside the
    two-tap one), two groups have conv heads, and the LDS weight buffers of EVERY workgroup are sized by the 16-channel K = 7 group's block
    (524 float4) -- so all other groups run with a buffer stride that is not their own.  Ragged stream counts (1 .. 5), buffers of 128,
    64, 37, 128 and 65 frames, every stream against its own oracle by its case's rule."""
    cases = FC.fused_models()
    counts = [1, 2, 3, 4, 5, 1, 2, 3, 4]
    assert len(cases) == 9 and len({FC.layer_block_f4(k, a["channels"]) for c in cases for a in c["arrays"] for k in a["kernel_sizes"]}) > 4
    models = [_load(loader, c, prewarm=False) for c in cases]
    b = na.Batch(0)
    owner = []
    for i, (m, _) in enumerate(models):
        first = b.AddStreams(m, counts[i])
        assert first == len(owner) and b.StreamKernelName(first) == KERNEL, cases[i]["name"]
        owner += [i] * counts[i]
    sizes = [BLOCK, 64, 37, BLOCK, 65]
    x = np.stack([O.signal_noise(sum(sizes), 900 + s) for s in range(len(owner))])
    y = _run(b, x, sizes)
    b.close()
    for s, i in enumerate(owner):
        _assert_case(cases[i], models[i][1], x[s], y[s], O.OracleWaveNet(cases[i]["arrays"], models[i][1]).process(x[s]), (cases[i]["name"], s))


# ---------------------------------------------------------------------------------------------------------- (e) the LDS limit

def test_a_kernel_size_that_fits_one_stream_per_workgroup_only_runs_512_streams(na, loader):
    """16 channels, K = 63: two staged weight blocks take 131 456 of the 160 KB, which leaves room for the block images of one stream
    (147 840 bytes), not two (164 224).  From 512 streams on the launcher wants two streams per workgroup and takes the largest count
    that fits: by default 511 and 512 streams run alike (under NA_FR_SPB=4 both fall from four streams to one, under NA_FR_PF=2 the LDS
    history buffers of one stream need the same 164 224 bytes, so the register prefetch takes over), three 128-frame buffers each; first and last stream follow the
    oracle, the rows the two batches share are bit-identical.  Which instantiation ran is not visible through the API: the test shows
    that the 512-stream call succeeds and computes the same, frame_lds_cases.cpp that only one stream fits.  (Before the limit was
    decided in frame_lds.h the 512-stream Process call failed with hipErrorInvalidValue.)"""
    case = FC.lds_model(63)
    m, w = _load(loader, case)
    base, _ = _base_rows(7, 3 * BLOCK, 90)
    yo = [O.OracleWaveNet(case["arrays"], w).process(base[r]) for r in range(7)]
    outs = {}
    for streams in (511, 512):
        b = _batch(na, m, streams, streams)
        y = _run(b, base[np.arange(streams) % 7], [BLOCK] * 3)
        b.close()
        for s in (0, streams - 1):
            _assert_windows(y[s], yo[s % 7], (streams, s))
        for s in range(7, streams):
            assert np.array_equal(y[s], y[s % 7]), (streams, s)
        outs[streams] = y
    assert np.array_equal(outs[512][:511], outs[511])


def test_the_largest_kernel_size_runs_short_and_long_buffers_and_the_next_is_refused_at_load(na, loader):
    """16 channels, K = 70: 162 176 bytes with 128-frame blocks, the largest that loads; a 64-frame and a 128-frame buffer both run.
    K = 71 would run the first and fail at the second (164 224 bytes): it is refused at load, with the layer and its kernel size named."""
    case = FC.lds_model(70)
    m, w = _load(loader, case)
    x = O.signal_noise(64 + BLOCK, seed=case["seed"])
    b = _batch(na, m, 1, case["name"])
    y = _run(b, x[None, :], [64, BLOCK])[0]
    b.close()
    _assert_windows(y, O.OracleWaveNet(case["arrays"], w).process(x), case["name"])
    case = FC.lds_model(71)
    with pytest.raises(na.NeuralAudioError, match="layer 0: kernel size 71 at 16 channels"):
        loader.CreateFromString(O.nam_json_wavenet_generic(case["arrays"], FC.weights(case)), ".nam", doPrewarm=False)
