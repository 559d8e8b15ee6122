"""The stage interpreter of the f16-split kernels (wavenet_split_kernels.hip: WaveNetSplitKernel<T, SPB, WPS, GEN, PK>) on models that are
not one of the official architectures -- their production kernel at every block length: every WaveNet of at most 16 channels with K = 3
layers, 1x1 heads and a proven f16 range, in its plain, padded or packed layout (tests/split_cases.py; tests/test_host_cpu.py proves
without a GPU that every case loads, is predicted here with the pack factor it claims, and is well conditioned).

* (a) named edges and a seeded fuzz, 7 streams with their own noise (a partly filled last virtual stream at P = 2 and P = 4) and 1 stream,
  in whole blocks and in ragged calls, with and without prewarm;
* (b) neighbours inside a packed virtual stream of a custom model: members leave, join fresh or prewarmed, are prewarmed again;
* (c) launches of 512 and more kernel-level streams: two streams per workgroup, a half-filled last workgroup, the half-batch chains;
* (d) launches a custom group shares with official ones, which then run on the interpreter too;
* (e) the range contract: samples beyond the input limit, infinities and NaN, for the stream itself and for its neighbours in a pack.

Every test asserts NA_BatchStreamKernelName and NA_BatchStreamPackFactor before it trusts a comparison.  Parity: against the f32 oracle,
the suite's WaveNet tolerance (2e-6 RMS, relative to the output level above 1) on EVERY 32-frame window of the output -- one wrong frame
of 1.2e-5 fails; the model must not be silent.  (Official models in (d) are held to the rule of tests/test_gpu_spec.py, the same number
over the whole signal.)  The forced-family knobs skip this file like tests/test_gpu_frame.py.

The cases' head scale is raised (split_cases.HEAD_GAIN) so that the bound, absolute below a level of 1, bites: with the lo x hi product of
one 1x1 or of two conv taps taken out of the interpreter, 67 and 26 of the 106 tests here fail.

Measured on an MI355X (default knobs, against O.OracleWaveNet): the worst 32-frame window of any case is 0.059 of the 2e-6 bound
(packed4-2-4; rings-63 0.055, the worst plain case 0.031); every bit-identity asserted below (call sizes, 1 / 7 / 513 .. 2052 streams,
ordered and half-batch launches, shared and own launches, neighbours of a pack) holds.  Instantiations launched: T = 2 with
SPB x WPS = {1, 2} x {1, 2, 4} at GEN = false, plain and packed (PK), and GEN = true at SPB = 1, WPS = 1, 2, 4."""
import os

import numpy as np
import pytest

import na_oracle as O
import split_cases as SC

FORCED = bool(os.environ.get("NA_WN_KERNEL") or os.environ.get("NA_WN_PACK") or os.environ.get("NA_WN_SPEC") or os.environ.get("NA_SP_T")
              or os.environ.get("NA_SP_GEN") or os.environ.get("NA_WN_PAD"))
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(FORCED, reason="forced kernel family")]

TOL_RMS = 2e-6  # the suite's WaveNet parity tolerance, relative to the output level above 1
WINDOW = 32
BLOCK = SC.BLOCK
KERNEL = "WaveNetSplitKernel"
NAMED = SC.named_cases()
STREAMS = 7  # P = 2: three full virtual streams and one member; P = 4: one full virtual stream and three members


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


@pytest.fixture(scope="module")
def loader(na):
    return na.NeuralModelLoader()


def _load(loader, case):
    w = SC.weights(case)
    m = loader.CreateFromString(O.nam_json_wavenet_generic(case["arrays"], w), ".nam", doPrewarm=False)
    assert m is not None, case["name"]
    return m, w


def _official(loader, name):
    return loader.CreateFromFile(os.path.join(O.MODELS_DIR, name), doPrewarm=False)


def _assert_lands(batch, case, first, count):
    for s in (first, first + count - 1):
        assert batch.StreamKernelName(s) == KERNEL and batch.StreamPackFactor(s) == case["pack"], \
            (case["name"], s, batch.StreamKernelName(s), batch.StreamPackFactor(s))


def _batch(na, m, case, streams, prewarm=True):
    b = na.Batch(0)
    assert b.AddStreams(m, streams, doPrewarm=prewarm) == 0
    _assert_lands(b, case, 0, streams)
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


def _worst_window(y, yo, what):
    """the parity rule: every 32-frame window (a shorter last one included) within TOL_RMS of the oracle, relative to its level above 1;
    returns the worst window as a fraction of the bound"""
    assert y.shape == yo.shape and np.all(np.isfinite(y)), what
    assert O.rms(yo) > 1e-5, (what, O.rms(yo))  # (a silent model cannot pass)
    worst = 0.0
    for a in range(0, y.size, WINDOW):
        err, level = O.rms(y[a:a + WINDOW] - yo[a:a + WINDOW]), O.rms(yo[a:a + WINDOW])
        worst = max(worst, err / (TOL_RMS * max(1.0, level)))
        assert err < TOL_RMS * max(1.0, level), (what, "window at", a, err, level)
    return worst


def _noise(rows, samples, seed):
    return np.stack([O.signal_noise(samples, seed + 1000 * r) for r in range(rows)])


def _oracles(case, w, x, prewarm=True):
    return [O.OracleWaveNet(case["arrays"], w, prewarm=prewarm).process(row) for row in x]


def _ragged(total):
    n37 = (total - 40) // 37
    return [1] * (total - 37 * n37) + [37] * n37


# ---------------------------------------------------------------------------------------------------------- (a) edges and fuzz

def _edges(na, loader, case, ragged):
    """Four runs of one case.  Prewarmed: 7 streams in whole 128-frame blocks and 7 streams in the ragged calls -- bit-identical, the
    kernels are chunk-invariant -- every stream against its own prewarmed oracle.  Fresh (zero history): 1 stream in whole blocks and 7
    streams in the ragged calls, against fresh oracles; the single stream is bit-identical to row 0 of the 7."""
    m, w = _load(loader, case)
    x = _noise(STREAMS, case["samples"], case["seed"])
    assert m.GetReceptiveFieldSize() == SC.receptive_field(case["arrays"])
    blocks = [BLOCK] * (x.shape[1] // BLOCK)
    worst = 0.0
    for prewarm in (True, False):
        yo = _oracles(case, w, x, prewarm)
        ys = []
        for streams, sizes in ((STREAMS if prewarm else 1, blocks), (STREAMS, ragged)):
            b = _batch(na, m, case, streams, prewarm)
            ys.append(_run(b, x[:streams], sizes))
            b.close()
            for s in range(streams):
                worst = max(worst, _worst_window(ys[-1][s], yo[s], (case["name"], case["path"], "prewarm" if prewarm else "fresh", streams, sizes[0], s)))
        rows = ys[0].shape[0]
        assert np.array_equal(ys[0], ys[1][:rows]), (case["name"], prewarm, float(np.abs(ys[0] - ys[1][:rows]).max()))
    print("%s [%s, P = %d]: worst window %.3g of the bound" % (case["name"], case["layout"], case["pack"], worst))


@pytest.mark.parametrize("case", NAMED, ids=[c["name"] for c in NAMED])
def test_named_split_interpreter_edges_match_oracle_whatever_the_call_sizes(na, loader, case):
    """Every named case of split_cases.py: whole 128-frame blocks (four waves per stream) against 56 single samples followed by 37-sample
    calls (one wave, then two; the ring cursors leave the 16-frame tile grid at once and wrap at other places; models with compact rings
    are cut to 32 + 5)."""
    _edges(na, loader, case, _ragged(case["samples"]))


@pytest.mark.parametrize("seed", range(SC.NUM_FUZZ_SEEDS))
def test_random_split_interpreter_architecture_matches_oracle(na, loader, seed):
    """The seeded draw over the same space, through call sizes that start 1, 1, 17, mix sizes around the wave and the block length with
    sizes the host cuts, and wrap every ring at least twice."""
    case, sizes = SC.fuzz_case(seed)
    _edges(na, loader, case, sizes)


# ---------------------------------------------------------------------------------------------------------- (b) neighbours in a pack

PACKED = [SC.packed2_custom(), SC.packed4_custom(), SC.dense_custom()]


@pytest.mark.parametrize("join_prewarmed", [False, True], ids=["fresh-join", "prewarmed-join"])
@pytest.mark.parametrize("case", PACKED, ids=[c["name"] for c in PACKED])
def test_members_of_a_custom_pack_leave_join_and_are_prewarmed_again_without_touching_their_neighbours(na, loader, case, join_prewarmed):
    """7 streams of a packed custom model, twice: a quiet batch in which nothing happens, and one in which member 1 of virtual stream 0
    leaves, the batch runs a buffer without it, another stream joins into the freed position (fresh -- its channel groups zeroed -- or
    prewarmed: the ring fill of one member of a running virtual stream, in the dense and the padded layout) and stream 5 is prewarmed
    again while it runs.  Streams that kept running are bit-identical to the quiet batch; the joiner and the re-prewarmed stream follow
    fresh oracles from then on; the retired row reads as silence."""
    m, w = _load(loader, case)
    sizes = [BLOCK, 37, 64, BLOCK, 65, 31, BLOCK, BLOCK]
    x = _noise(STREAMS, sum(sizes), case["seed"] + 7)
    quiet, busy = _batch(na, m, case, STREAMS), _batch(na, m, case, STREAMS)
    want = _run(quiet, x, sizes)
    quiet.close()
    got = [_run(busy, x[:, :165], sizes[:2])]
    busy.RemoveStreams(1)
    assert busy.NumStreams() == STREAMS and busy.NumLiveStreams() == STREAMS - 1
    got.append(_run(busy, x[:, 165:229], [64]))
    assert not np.any(got[-1][1])
    assert busy.AddStreams(m, 1, doPrewarm=join_prewarmed) == 1
    busy.Prewarm(5)
    _assert_lands(busy, case, 0, STREAMS)
    got.append(_run(busy, x[:, 229:], sizes[3:]))
    busy.close()
    got = np.concatenate(got, axis=1)
    for s in (0, 2, 3, 4, 6):
        assert np.array_equal(got[s], want[s]), (case["name"], s, float(np.abs(got[s] - want[s]).max()))
    assert np.array_equal(got[[1, 5], :165], want[[1, 5], :165]) and np.array_equal(got[5, :229], want[5, :229])
    _worst_window(got[1, 229:], O.OracleWaveNet(case["arrays"], w, prewarm=join_prewarmed).process(x[1, 229:]), (case["name"], "joiner"))
    _worst_window(got[5, 229:], O.OracleWaveNet(case["arrays"], w).process(x[5, 229:]), (case["name"], "prewarmed again"))
    _worst_window(want[0], O.OracleWaveNet(case["arrays"], w).process(x[0]), (case["name"], "quiet"))


# ---------------------------------------------------------------------------------------------------------- (c) 512 and more kernel-level streams

BIG = [(SC.plain_custom(), 513), (SC.plain_custom(), 1030), (SC.packed2_custom(), 1030), (SC.packed4_custom(), 2052), (SC.dense_custom(), 2052)]
HALVES_KNOBS = ("NA_HOST_HALVES", "NA_RESIDENT", "NA_SP_SPB", "NA_HOST_CHAINS")


@pytest.mark.parametrize("case,streams", BIG, ids=["%s-%d" % (c["name"], s) for c, s in BIG])
def test_large_custom_batches_compute_what_a_batch_of_seven_streams_computes(na, loader, case, streams):
    """From 512 kernel-level streams on a launch puts two streams into a workgroup (SPB = 2); a batch on its own HIP stream runs such a
    buffer as two free-running half-batch launches instead (gpu_batch_chains.cpp PrepareHalves: one split launch of at least 512
    kernel-level streams).  513 plain streams: ordered, 256 full workgroups and a half-filled one; in halves, 257 + 256 streams at one per
    workgroup.  1030 plain, 1030 at P = 2 (515 virtual streams, the last one half filled) and 2052 at P = 4 (513 virtual streams): two per
    workgroup either way.  Each size runs on a caller's HIP stream (ordered launches) and on the batch's own (half launches, asserted),
    seven distinct noise rows repeated, buffers of 128, 128, 64, 128, 37 and 128 frames; every row is bit-identical to the same row of a
    7-stream batch, and rows 0, one in the middle and the last follow their oracles."""
    import torch
    dev = torch.device("cuda", 0)
    m, w = _load(loader, case)
    sizes = [BLOCK, BLOCK, 64, BLOCK, 37, BLOCK]
    base = _noise(STREAMS, sum(sizes), case["seed"] + 3)
    small = _batch(na, m, case, STREAMS)
    want = _run(small, base, sizes)
    small.close()
    x = np.ascontiguousarray(base[np.arange(streams) % STREAMS])
    xd = torch.from_numpy(x).to(dev)
    ts = torch.cuda.Stream(device=dev)
    for own in (False, True):
        b = na.Batch(0) if own else na.Batch(0, hip_stream=ts.cuda_stream)
        assert b.AddStreams(m, streams) == 0
        _assert_lands(b, case, 0, streams)
        outs, a = [], 0
        for n in sizes:
            xin = xd[:, a:a + n].contiguous()
            yd = torch.zeros(streams, n, device=dev)
            torch.cuda.synchronize(dev)
            b.ProcessDevice(xin.data_ptr(), yd.data_ptr(), n)
            b.WaitOutputs()
            b.Synchronize()
            if not any(os.environ.get(k) for k in HALVES_KNOBS):
                assert b.UsesHalfLaunches() == own, (case["name"], streams, own, n)
            outs.append(yd.cpu().numpy())
            a += n
        b.close()
        y = np.concatenate(outs, axis=1)
        bad = [s for s in range(streams) if not np.array_equal(y[s], want[s % STREAMS])]
        assert not bad, (case["name"], streams, "own stream" if own else "caller's stream", len(bad), bad[:8])
    for s in (0, streams // 2, streams - 1):
        _worst_window(y[s], O.OracleWaveNet(case["arrays"], w).process(x[s]), (case["name"], streams, s))


# ---------------------------------------------------------------------------------------------------------- (d) shared launches

def _shared(na, loader, members, sizes, seed):
    """members: (model, count, quality, oracle factory, case or None).  One batch of all of them against one batch per member alone,
    bit for bit, and every stream against its oracle: a custom case window by window, an official model over the whole signal."""
    total = sum(c for _, c, _, _, _ in members)
    x = _noise(total, sum(sizes), seed)
    b = na.Batch(0)
    first = []
    for m, count, q, _, case in members:
        first.append(b.AddStreams(m, count, quality=q))
        if case is not None:
            _assert_lands(b, case, first[-1], count)
    assert b.NumStreams() == total
    y = _run(b, x, sizes)
    b.close()
    for (m, count, q, oracle, case), f in zip(members, first):
        alone = na.Batch(0)
        assert alone.AddStreams(m, count, quality=q) == 0
        ya = _run(alone, x[f:f + count], sizes)
        alone.close()
        assert np.array_equal(y[f:f + count], ya), (f, count, float(np.abs(y[f:f + count] - ya).max()))
        for s in range(f, f + count):
            yo = oracle().process(x[s])
            if case is not None:
                _worst_window(y[s], yo, (case["name"], s))
            else:
                assert np.all(np.isfinite(y[s])) and O.rms(yo) > 1e-5 and O.rms(y[s] - yo) < TOL_RMS * max(1.0, O.rms(yo)), (s, O.rms(y[s] - yo))


def _custom(loader, case, count):
    m, w = _load(loader, case)
    return (m, count, 1.0, lambda: O.OracleWaveNet(case["arrays"], w), case)


def _file(loader, name, count, quality=1.0):
    return (_official(loader, name), count, quality, lambda: O.oracle_from_file(name, quality=quality), None)


SHARED_SIZES = [BLOCK, 64, 37, BLOCK, 32, 65]


def test_a_plain_custom_model_beside_a1_standard_moves_neither_by_a_bit(na, loader):
    """One custom 16 / 8 group in a launch takes the specialised chain away from the A1 Standard streams beside it (LaunchWaveNetSpecFused
    refuses a launch that is not one official architecture): both run on the interpreter's fast instantiation.  Standard alone runs its
    chain, and chain and interpreter are bit-identical."""
    _shared(na, loader, [_file(loader, "BossWN-standard.nam", 3), _custom(loader, SC.plain_custom(), 3), _file(loader, "BossWN-standard.nam", 2)], SHARED_SIZES, 11)


def test_packed_customs_beside_feather_and_nano_in_one_packed_launch(na, loader):
    """P = 2 and P = 4 customs (padded and dense packs) beside the official packed models: one launch of the packed flavour (PK), ragged
    member counts in every group's last virtual stream."""
    _shared(na, loader, [_file(loader, "BossWN-feather.nam", 3), _custom(loader, SC.packed2_custom(), 3), _file(loader, "BossWN-nano.nam", 5),
                         _custom(loader, SC.packed4_custom(), 5), _custom(loader, SC.dense_custom(), 6)], SHARED_SIZES, 12)


def test_a_plain_fast_custom_rides_in_the_packed_launch(na, loader):
    """LaunchKind::SplitJoinsPacked: a batch that has a packed group runs its plain fast groups in the packed launch, as packs of one."""
    padded = [c for c in NAMED if c["name"] == "padded-12-6"][0]
    _shared(na, loader, [_custom(loader, SC.plain_custom(), 3), _custom(loader, SC.packed2_custom(), 3), _custom(loader, padded, 2)], SHARED_SIZES, 13)


def test_a_fast_custom_beside_a2_streams_runs_the_generic_instantiation(na, loader):
    """The A2 submodels' plans are not fast ones (kernel sizes 6 and 15, a conv head): a launch they share with a custom fast model runs
    GEN = true over the custom's fast plan."""
    _shared(na, loader, [_file(loader, "BossWN-a2.nam", 2, 1.0), _custom(loader, SC.plain_custom(), 3), _file(loader, "BossWN-a2.nam", 2, 0.0)], SHARED_SIZES, 14)


# ---------------------------------------------------------------------------------------------------------- (e) the range contract

BAD = [1e5, float("inf"), float("-inf"), float("nan")]
RANGE = [SC.plain_custom(), SC.packed2_custom(), SC.packed4_custom()]


def _range_contract(na, m, streams, bad, check_lands, rf, seed):
    """Row 1 of a `streams`-stream batch is fed bad samples (a burst of 40 and a single one of the other sign); -> (the limit, outputs with the
    bad samples, with the clamped ones, with silence in row 1, the inputs, the first frame at which row 1 has forgotten the bad ones)"""
    n = 12 * BLOCK
    x = _noise(streams, n, seed)
    xb = x.copy()
    xb[1, 100:140] = bad
    xb[1, 300] = -bad if np.isfinite(bad) else bad
    outs = []
    for k in range(3):
        b = na.Batch(0)
        assert b.AddStreams(m, streams) == 0
        check_lands(b)
        limit = b.StreamInputLimit(1)
        assert 1.0 < limit <= 32752.0, limit
        xk = xb.copy()
        if k == 1:
            xk[1] = np.nan_to_num(xb[1], nan=0.0, posinf=limit, neginf=-limit).clip(-limit, limit)
        if k == 2:
            xk[1] = 0.0
        outs.append(_run(b, xk.astype(np.float32), [BLOCK] * 12))
        b.close()
    assert 301 + rf < n - BLOCK
    return limit, outs, x, 301 + rf


@pytest.mark.parametrize("bad", BAD)
@pytest.mark.parametrize("case", RANGE, ids=[c["name"] for c in RANGE])
def test_out_of_range_samples_of_a_custom_model_are_clamped_and_no_neighbour_notices(na, loader, case, bad):
    """The contract of the f16-split path on custom models: a sample beyond NA_BatchStreamInputLimit is clamped to it, +-inf to +-limit,
    NaN reads as silence; one receptive field after the last bad sample the stream is bit-identical to one that was fed the clamped
    values.  The other streams of the batch -- at P = 2 and 4 the members of the same virtual stream, whose block-diagonal operands
    multiply the bad member's value by their zeros -- are bit-identical to a run in which the bad member was fed silence."""
    m, w = _load(loader, case)
    limit, (yb, yc, y0), x, tail = _range_contract(na, m, STREAMS, bad, lambda b: _assert_lands(b, case, 0, STREAMS), SC.receptive_field(case["arrays"]), case["seed"] + 20)
    assert np.all(np.isfinite(yb)), (case["name"], bad)
    assert np.array_equal(yb[1, tail:], yc[1, tail:]), (case["name"], bad, float(np.abs(yb[1, tail:] - yc[1, tail:]).max()))
    others = [s for s in range(STREAMS) if s != 1]
    assert np.array_equal(yb[others], y0[others]) and np.array_equal(yc[others], y0[others]), (case["name"], bad)
    oracle = O.OracleWaveNet(case["arrays"], w)
    _worst_window(yb[1, :96], oracle.process(x[1])[:96], (case["name"], "before the bad samples"))
    _worst_window(yb[0], O.OracleWaveNet(case["arrays"], w).process(x[0]), (case["name"], "neighbour"))


@pytest.mark.parametrize("bad", BAD)
def test_out_of_range_samples_of_one_nano_stream_do_not_reach_the_other_members_of_its_pack(na, loader, bad):
    """The same neighbour check on the official packed chain: Nano x 5 (P = 4: streams 0, 2 and 3 share a virtual stream with the bad one)."""
    m = _official(loader, "BossWN-nano.nam")

    def lands(b):
        assert b.StreamPackFactor(1) == 4

    limit, (yb, yc, y0), x, _ = _range_contract(na, m, 5, bad, lands, 0, 77)
    assert np.all(np.isfinite(yb)), bad
    others = [0, 2, 3, 4]
    assert np.array_equal(yb[others], y0[others]) and np.array_equal(yc[others], y0[others]), bad
    yo = O.oracle_from_file("BossWN-nano.nam").process(x[0])
    assert O.rms(yb[0] - yo) < TOL_RMS * max(1.0, O.rms(yo))
