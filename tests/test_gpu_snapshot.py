"""GPU tests of the stream snapshots (NA_BatchSaveStreams / NA_BatchLoadStreams, csrc/stream_snapshot.h).

Every case drives clipped noise (na_oracle.signal_noise), so the state matters, and most compare an interrupted run -- process, save,
load somewhere else, continue -- with an uninterrupted one bit for bit: the same kernel runs both, and a snapshot keeps the state's own
number format.  Where the two sides run different kernel families (f32 frame kernel <-> f16-split chain) the comparison is the suite's
WaveNet tolerance against the live oracle.  Every comparison has a sensitivity control: a fresh prewarmed stream that skips the load
must be far off (CONTROL_RMS = 100 x the tolerance: a control within two orders of magnitude of the bound it guards shows nothing)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import na_oracle as O
import wide_cases as WC

pytestmark = pytest.mark.gpu

TOL_RMS = 2e-6               # the suite's WaveNet tolerance (tests/test_gpu_offline.py, test_gpu_parity.py)
CONTROL_RMS = 100 * TOL_RMS
N1 = 128 * 37 + 100          # ragged: the last buffer is cut 64 + 32 + 4 for compact rings
CHUNK = 8192
CONV_TAIL_STACK = "synthetic_stack_gru12_conv16k4d64elu_dense5softmax_dense1.json"
KNOBS = ("NA_WN_KERNEL", "NA_WN_SPEC", "NA_WN_PACK", "NA_WN_DENSE", "NA_WN_PAD", "NA_HOST_HALVES", "NA_HOST_DIRECT", "NA_SP_T", "NA_SP_GEN", "NA_RESIDENT")


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


def _model(na, name, quality=1.0, on_demand=False):
    loader = na.NeuralModelLoader()
    loader.SetDefaultQualityScaleFactor(quality)
    if on_demand:
        loader.SetCompositeModelLoadMode(na.ECompositeModelLoadMode.OnDemand)
    if name == "lite":  # (no A1 Lite capture among the sample models: a synthetic one, as tests/test_gpu_offline.py builds it)
        arrays = O.a1_arrays(12, 6)
        m = loader.CreateFromString(O.nam_json_wavenet_a1(12, 6, O.synth_wavenet_weights(arrays, seed=41)), ".nam", doPrewarm=False)
    elif name in WIDE:  # layer arrays wider than 16 channels: the runtime-shaped kernels (WaveNetGenericKernel / WaveNetWideKernel)
        arrays = WC.two_array(*WIDE[name])
        m = loader.CreateFromString(O.nam_json_wavenet_generic(arrays, O.synth_wavenet_weights(arrays, seed=WIDE[name][0])), ".nam", doPrewarm=False)
    else:
        m = loader.CreateFromFile(os.path.join(O.MODELS_DIR, name), doPrewarm=False)
    assert m is not None
    m._loader = loader
    return m


def _run(batch, x):
    """x [streams, n] through the batch in host buffers of at most CHUNK samples"""
    x = np.atleast_2d(x)
    return np.concatenate([batch.Process(x[:, i:i + CHUNK]) for i in range(0, x.shape[1], CHUNK)], axis=1)


def _window(m):
    rf = m.GetReceptiveFieldSize()
    return rf if rf > 0 else 512  # recurrent models: the first 512 samples stand for "the first receptive field"


def _control_bound(y):
    """What a stream that skipped the load must be off by (RMS over the window `y` of the uninterrupted run): CONTROL_RMS, an absolute
    figure like the tolerance it guards -- except for a model whose output hardly moves at all.  The softmax stack among the sample
    models is one: its output over clipped noise is -0.17 with 7.8e-5 RMS of variation around it (measured on the model alone, before
    any snapshot code ran), so NO input-dependent difference can reach 2e-4 there.  For such a model the bound is a quarter of the
    output's own variation: a stream with unrelated state is off by about as much as the signal itself moves (measured: 0.5 of it
    for the LSTM 1x16 sample model)."""
    y = np.asarray(y, np.float64)
    return min(CONTROL_RMS, 0.25 * float(np.sqrt(np.mean((y - y.mean()) ** 2))))


# ---------------------------------------------------------------------------------------------------------------- 1

WIDE = {"wide-40/20": (40, 20), "wide-72/36": (72, 36)}
CASES = [("BossWN-standard.nam", 1.0), ("lite", 1.0), ("wide-40/20", 1.0), ("wide-72/36", 1.0), ("BossWN-feather.nam", 1.0), ("BossWN-nano.nam", 1.0), ("BossWN-a2.nam", 0.0),
         ("BossWN-a2.nam", 1.0), ("BossLSTM-1x16.nam", 1.0), ("BossLSTM-2x8.nam", 1.0), ("synthetic_gru_1x16.json", 1.0), (CONV_TAIL_STACK, 1.0)]


@pytest.mark.parametrize("name,quality", CASES)
def test_interrupted_run_equals_the_uninterrupted_one(na, name, quality):
    """A processes N1 + N2.  B processes N1, is saved and removed; a fresh C (no prewarm, another batch) is loaded and processes N2.
    C's output is A's second part bit for bit; a prewarmed stream that skips the load is far off over the first receptive field."""
    m = _model(na, name, quality)
    rf = m.GetReceptiveFieldSize()
    n2 = max(2 * rf, 8192)
    x = O.signal_noise(N1 + n2, seed=21)
    bA = na.Batch(0)
    bA.AddStreams(m, 1, quality=quality)
    yA = np.concatenate([_run(bA, x[:N1]), _run(bA, x[N1:])], axis=1)[0]

    bB = na.Batch(0)
    bB.AddStreams(m, 1, quality=quality)
    yB = _run(bB, x[:N1])[0]
    assert np.array_equal(yB, yA[:N1])
    assert bB.StreamSnapshotBytes(0) == na.snapshot_bytes(m)
    blob = bB.SaveStreams([0])
    assert len(blob) == na.snapshot_bytes(m)
    kernel_b = bB.StreamKernelName(0)
    bB.RemoveStreams(0)
    bB.close()

    bC = na.Batch(0)
    bC.AddStreams(m, 1, quality=quality, doPrewarm=False)
    bC.LoadStreams([0], blob)
    assert bC.StreamKernelName(0) == kernel_b == bA.StreamKernelName(0)
    yC = _run(bC, x[N1:])[0]

    bD = na.Batch(0)
    bD.AddStreams(m, 1, quality=quality)  # prewarmed, no load
    yD = _run(bD, x[N1:])[0]
    w = _window(m)
    control = O.rms(yD[:w] - yA[N1:N1 + w])
    diff = int(np.count_nonzero(yC != yA[N1:]))
    print("%s q=%g on %s: %d bytes, %d of %d samples differ, control rms %.3g over %d samples (bound %.3g)"
          % (name, quality, kernel_b, len(blob), diff, n2, control, w, _control_bound(yA[N1:N1 + w])))
    assert control > _control_bound(yA[N1:N1 + w]), "the input does not make the state matter"
    assert np.array_equal(yC, yA[N1:]), (name, quality, int(np.argmax(yC != yA[N1:])), O.rms(yC - yA[N1:]))
    for b in (bA, bC, bD):
        b.close()


# ---------------------------------------------------------------------------------------------------------------- 2

@pytest.mark.parametrize("name,pack,x_count,save_ids,y_count,y_ids", [
    # X: two dense virtual streams, positions 0-3 and 0-2; the streams at positions 1 (id 1) and 2 (id 6) go to positions 3 (id 3) and 0 (id 4) of Y
    ("BossWN-nano.nam", 4, 7, (1, 6), 8, (3, 4)),
    # pack of 2: position 1 (id 1) -> position 0 (id 2), position 0 (id 2) -> position 1 (id 1)
    ("BossWN-feather.nam", 2, 3, (1, 2), 4, (2, 1))])
def test_packed_positions(na, name, pack, x_count, save_ids, y_count, y_ids):
    """Streams inside packed virtual streams move to other positions of virtual streams whose neighbours keep running (and whose
    shared cursors stand elsewhere): the moved streams continue like their unmoved twins, the neighbours like a run without the load."""
    m = _model(na, name)
    rf = m.GetReceptiveFieldSize()
    n2 = 2 * rf
    n_other = 128 * 11 + 37  # what Y's streams have processed: another cursor position than X's N1
    xs = np.stack([O.signal_noise(N1 + n2, seed=100 + s) for s in range(x_count)])
    ys_in = np.stack([O.signal_noise(n_other + n2, seed=200 + s) for s in range(y_count)])

    bX = na.Batch(0)
    bX.AddStreams(m, x_count)
    assert all(bX.StreamPackFactor(s) == pack for s in range(x_count))
    _run(bX, xs[:, :N1])
    blob = bX.SaveStreams(list(save_ids))
    twins = _run(bX, xs[:, N1:])  # (a save is read-only: X's own streams are the unmoved twins)

    def build_y(load):
        b = na.Batch(0)
        b.AddStreams(m, y_count)
        _run(b, ys_in[:, :n_other])
        lo, hi = min(y_ids), max(y_ids)
        assert hi == lo + 1
        b.RemoveStreams(lo, 2)
        assert b.AddStreams(m, 2, doPrewarm=False) == lo  # the two fresh streams recycle the ids -- and the positions inside the packs
        assert all(b.StreamPackFactor(s) == pack for s in range(y_count))
        if load:
            b.LoadStreams(list(y_ids), blob)
        x2 = ys_in[:, n_other:].copy()
        for src, dst in zip(save_ids, y_ids):
            x2[dst] = xs[src, N1:]
        out = _run(b, x2)
        name_y = b.StreamKernelName(y_ids[0])
        b.close()
        return out, name_y

    got, kernel_y = build_y(True)
    plain, _ = build_y(False)
    assert kernel_y == bX.StreamKernelName(save_ids[0])
    for src, dst in zip(save_ids, y_ids):
        control = O.rms(plain[dst][:rf] - twins[src][:rf])
        print("%s: stream %d -> %d, control rms %.3g" % (name, src, dst, control))
        assert control > CONTROL_RMS
        assert np.array_equal(got[dst], twins[src]), (src, dst, int(np.argmax(got[dst] != twins[src])))
    for s in range(y_count):
        if s not in y_ids:
            assert np.array_equal(got[s], plain[s]), ("neighbour", s)
    bX.close()


# ---------------------------------------------------------------------------------------------------------------- 3

@pytest.mark.watchdog(300)
def test_three_hundred_streams_in_one_call(na):
    from neuralaudio_amd import capi
    lib = capi.load_library()
    m = _model(na, "BossWN-standard.nam")
    rf = m.GetReceptiveFieldSize()
    S, K, n2 = 1024, 300, 2 * rf
    rng = np.random.default_rng(3)
    x = np.clip(0.25 * rng.standard_normal((S, N1 + n2)), -1.0, 1.0).astype(np.float32)
    b1 = na.Batch(0)
    b1.AddStreams(m, S)
    _run(b1, x[:, :N1])
    ids = 7 + 3 * np.arange(K)  # strided
    launches = lib.NA_DebugSnapshotLaunches()
    blob = b1.SaveStreams(ids)
    assert lib.NA_DebugSnapshotLaunches() == launches + 1  # one model group: one export launch for 300 streams
    assert len(blob) == K * na.snapshot_bytes(m)
    b2 = na.Batch(0)
    b2.AddStreams(m, K, doPrewarm=False)
    perm = rng.permutation(K)
    launches = lib.NA_DebugSnapshotLaunches()
    b2.LoadStreams(perm, blob)  # blob i (stream ids[i] of b1) -> stream perm[i] of b2
    assert lib.NA_DebugSnapshotLaunches() == launches + 1
    x2 = np.empty((K, n2), np.float32)
    x2[perm] = x[ids, N1:]
    want = _run(b1, x[:, N1:])[ids]
    got = _run(b2, x2)[perm]
    assert b1.StreamKernelName(int(ids[0])) == b2.StreamKernelName(0)
    bad = [int(i) for i in range(K) if not np.array_equal(got[i], want[i])]
    assert not bad, bad[:10]
    b3 = na.Batch(0)
    b3.AddStreams(m, 1)
    assert O.rms(_run(b3, x[7:8, N1:])[0][:rf] - want[0][:rf]) > CONTROL_RMS
    for b in (b1, b2, b3):
        b.close()


# ---------------------------------------------------------------------------------------------------------------- 4

def test_slimmable_container_keeps_quality_bits_and_both_submodels(na):
    src_m = _model(na, "BossWN-a2.nam", 0.0, on_demand=True)
    dst_m = _model(na, "BossWN-a2.nam", 1.0)  # LoadAll
    x = O.signal_noise(3 * 3000 + 2 * 20000, seed=31)
    src = na.Batch(0)
    src.AddStreams(src_m, 1, quality=0.0)
    first = src.GetActiveSubModel(0)
    # the other submodel never had its prewarm: a snapshot taken now says so, and the LoadAll destination answers like the source
    assert not src.IsQualityChangeRealtimeSafe(0, 1.0)
    early = src.SaveStreams([0])
    dst0 = na.Batch(0)
    dst0.AddStreams(dst_m, 1, quality=1.0)
    assert dst0.IsQualityChangeRealtimeSafe(0, 0.0) and dst0.GetActiveSubModel(0) != first
    dst0.LoadStreams([0], early)
    assert dst0.GetActiveSubModel(0) == first
    assert not dst0.IsQualityChangeRealtimeSafe(0, 1.0) and dst0.IsQualityChangeRealtimeSafe(0, 0.0)
    dst0.close()

    _run(src, x[:3000])
    src.SetQuality(0, 1.0)  # first use of the other submodel: prewarmed now
    assert src.GetActiveSubModel(0) != first
    _run(src, x[3000:6000])
    src.SetQuality(0, 0.0)
    _run(src, x[6000:9000])
    blob = src.SaveStreams([0])

    dst = na.Batch(0)
    dst.AddStreams(dst_m, 1, quality=1.0)
    dst.LoadStreams([0], blob)
    assert dst.GetActiveSubModel(0) == src.GetActiveSubModel(0) == first
    for q in (0.0, 1.0):
        assert dst.IsQualityChangeRealtimeSafe(0, q) == src.IsQualityChangeRealtimeSafe(0, q)
    fresh = na.Batch(0)
    fresh.AddStreams(dst_m, 1, quality=0.0)
    # both submodels continue like the source's: the active one, then -- after a switch -- the frozen one
    a, b, f = _run(src, x[9000:29000])[0], _run(dst, x[9000:29000])[0], _run(fresh, x[9000:29000])[0]
    assert O.rms(f[:4096] - a[:4096]) > CONTROL_RMS
    assert np.array_equal(a, b), int(np.argmax(a != b))
    for bb in (src, dst, fresh):
        bb.SetQuality(0, 1.0)
    a, b, f = _run(src, x[29000:])[0], _run(dst, x[29000:])[0], _run(fresh, x[29000:])[0]
    assert O.rms(f[:4096] - a[:4096]) > CONTROL_RMS
    assert np.array_equal(a, b), int(np.argmax(a != b))
    for bb in (src, dst, fresh):
        bb.close()


# ---------------------------------------------------------------------------------------------------------------- 5

CHILD = """
import os, sys
sys.path[:0] = [%(root)r, %(tests)r]
import numpy as np
import neuralaudio_amd as na
import na_oracle as O
mode, blob_path, out_path, n1, n2 = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5])
x = O.signal_noise(n1 + n2, seed=51)
m = na.NeuralModelLoader().CreateFromFile(os.path.join(O.MODELS_DIR, "BossWN-standard.nam"), doPrewarm=False)
b = na.Batch(0)
if mode == "save":
    b.AddStreams(m, 1)
    for i in range(0, n1, 8192):
        b.Process(x[None, i:min(i + 8192, n1)])
    open(blob_path, "wb").write(b.SaveStreams([0]))
else:
    b.AddStreams(m, 1, doPrewarm=False)
    b.LoadStreams([0], open(blob_path, "rb").read())
    y = np.concatenate([b.Process(x[None, i:min(i + 8192, n1 + n2)]) for i in range(n1, n1 + n2, 8192)], axis=1)[0]
    np.save(out_path, y)
print("KERNEL " + b.StreamKernelName(0))
"""


def _child(tmp_path, env, mode, blob_path, out_path, n1, n2):
    script = tmp_path / "snapshot_child.py"
    script.write_text(CHILD % dict(root=O.ROOT, tests=os.path.join(O.ROOT, "tests")))
    e = dict({k: v for k, v in os.environ.items() if k not in KNOBS}, **env)
    try:
        r = subprocess.run([sys.executable, str(script), mode, str(blob_path), str(out_path), str(n1), str(n2)], env=e, capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired as ex:
        pytest.fail("the %s child did not finish in 240 s: %s" % (mode, (ex.stdout or b"")[-2000:]))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [l for l in r.stdout.splitlines() if l.startswith("KERNEL ")][-1].split()[1]


@pytest.mark.watchdog(260)
@pytest.mark.parametrize("direction", ["f32_to_split", "split_to_f32"])
def test_across_state_formats_and_processes(na, tmp_path, direction):
    """A1 Standard saved on the f32 frame kernel and loaded on the f16-split chain (another process: NA_WN_KERNEL is read once per
    process), and the other way round.  Different arithmetic on the two sides, so the measure is the oracle: RMS error of the
    continuation against the live oracle over the whole signal, over the first receptive field after the restore, <= TOL_RMS."""
    m = _model(na, "BossWN-standard.nam")
    rf = m.GetReceptiveFieldSize()
    n2 = 2 * rf
    x = O.signal_noise(N1 + n2, seed=51)
    yo = O.oracle_from_file("BossWN-standard.nam").process(x)
    blob_path, out_path = tmp_path / "blob.bin", tmp_path / "out.npy"
    if direction == "f32_to_split":
        k_src = _child(tmp_path, {"NA_WN_KERNEL": "frame"}, "save", blob_path, out_path, N1, n2)
        b = na.Batch(0)
        b.AddStreams(m, 1, doPrewarm=False)
        b.LoadStreams([0], blob_path.read_bytes())
        k_dst = b.StreamKernelName(0)
        y = _run(b, x[N1:])[0]
        b.close()
    else:
        b = na.Batch(0)
        b.AddStreams(m, 1)
        _run(b, x[:N1])
        blob_path.write_bytes(b.SaveStreams([0]))
        k_src = b.StreamKernelName(0)
        b.close()
        k_dst = _child(tmp_path, {"NA_WN_KERNEL": "frame"}, "load", blob_path, out_path, N1, n2)
        y = np.load(out_path)
    frame, split = (k_src, k_dst) if direction == "f32_to_split" else (k_dst, k_src)
    assert frame == "WaveNetFrameKernel" and split in ("WaveNetSpecKernel", "WaveNetSplitKernel"), (k_src, k_dst)
    enc = int(np.frombuffer(blob_path.read_bytes(), "<u4", count=1, offset=48 + 4)[0])
    assert enc == (0 if direction == "f32_to_split" else 1)  # F32 / SPLIT section
    fresh = na.Batch(0)
    fresh.AddStreams(m, 1)
    control = O.rms(_run(fresh, x[N1:])[0][:rf] - yo[N1:N1 + rf])
    fresh.close()
    err = O.rms(y[:rf] - yo[N1:N1 + rf])
    print("%s: %s -> %s, rms error vs oracle over the first %d samples %.3g (whole continuation %.3g), control %.3g"
          % (direction, k_src, k_dst, rf, err, O.rms(y - yo[N1:]), control))
    assert control > CONTROL_RMS
    assert err <= TOL_RMS, err


# ---------------------------------------------------------------------------------------------------------------- 6

def test_legacy_one_stream_model(na):
    def make(name):
        loader = na.NeuralModelLoader()
        m = loader.CreateFromFile(os.path.join(O.MODELS_DIR, name))
        m._loader = loader
        return m
    for name in ("BossWN-standard.nam", "BossLSTM-1x16.nam"):
        x = O.signal_noise(N1 + 8192, seed=61)
        a, b, fresh = make(name), make(name), make(name)
        a.Process(x[:N1])
        blob = a.SaveState()
        assert len(blob) == a.SnapshotBytes()
        b.LoadState(blob)
        want, got, plain = a.Process(x[N1:]), b.Process(x[N1:]), fresh.Process(x[N1:])
        assert O.rms(plain[:512] - want[:512]) > CONTROL_RMS
        assert np.array_equal(want, got), name
        other = make("BossWN-nano.nam")
        with pytest.raises(na.NeuralAudioError, match="fingerprint"):
            other.LoadState(blob)


# ---------------------------------------------------------------------------------------------------------------- 7

def test_refusals_leave_every_stream_alone(na):
    from neuralaudio_amd import capi
    lib = capi.load_library()
    m = _model(na, "BossWN-standard.nam")
    x = np.stack([O.signal_noise(3000 + 8192, seed=70 + s) for s in range(5)])
    src = na.Batch(0)
    src.AddStreams(m, 5)
    _run(src, x[::-1, :3000])  # (other states than the destination's)
    good = src.SaveStreams([0, 1, 2, 3, 4])
    one = len(good) // 5
    assert one == na.snapshot_bytes(m)
    b, twin = na.Batch(0), na.Batch(0)
    for bb in (b, twin):
        bb.AddStreams(m, 5)
        _run(bb, x[:, :3000])

    def corrupt(offset, fmt, value, index=0):
        raw = bytearray(good)
        raw[index * one + offset:index * one + offset + np.dtype(fmt).itemsize] = np.asarray([value], fmt).tobytes()
        return bytes(raw)

    arrays = O.a1_arrays(16, 8)
    loader = na.NeuralModelLoader()
    synth = loader.CreateFromString(O.nam_json_wavenet_a1(16, 8, O.synth_wavenet_weights(arrays, seed=9)), ".nam", doPrewarm=False)
    sb = na.Batch(0)
    sb.AddStreams(synth, 5)
    foreign = sb.SaveStreams([0, 1, 2, 3, 4])  # same architecture and size, other weights
    sb.close()
    cases = [("truncated", good[:-10], "truncated"), ("truncated header", good[:4 * one + 20], "truncated"),
             ("magic", corrupt(0, "<u4", 0x5353414F), "magic"), ("version", corrupt(4, "<u4", 2), "version"),
             ("fingerprint", foreign, "fingerprint"), ("fingerprint bit", corrupt(16, "<u8", 1), "fingerprint"),
             ("third of five", corrupt(0, "<u4", 0, index=2), "snapshot 2"), ("submodel count", corrupt(24, "<u4", 2, index=4), "submodel count")]
    ids = (C.c_int * 5)(0, 1, 2, 3, 4)
    for what, blob, reason in cases:
        assert lib.NA_BatchLoadStreams(b._h, ids, 5, blob, len(blob)) != 0, what
        assert reason in capi.last_error(), (what, capi.last_error())
        with pytest.raises(na.NeuralAudioError):
            b.LoadStreams([0, 1, 2, 3, 4], blob)
    with pytest.raises(na.NeuralAudioError, match="twice"):
        b.LoadStreams([0, 1, 1, 3, 4], good)
    with pytest.raises(na.NeuralAudioError, match="not a live stream"):
        b.LoadStreams([0, 1, 2, 3, 5], good)
    # a save into a short buffer reports the size it needs and writes nothing
    buf = C.create_string_buffer(b"\x55" * 100, 100)
    need = C.c_size_t(0)
    assert lib.NA_BatchSaveStreams(b._h, ids, 5, buf, 100, C.byref(need)) != 0
    assert need.value == 5 * one and "too small" in capi.last_error() and buf.raw == b"\x55" * 100
    assert np.array_equal(_run(b, x[:, 3000:]), _run(twin, x[:, 3000:]))
    # ... and the good blob does load
    b.LoadStreams([0, 1, 2, 3, 4], good)
    for bb in (src, b, twin):
        bb.close()


# ---------------------------------------------------------------------------------------------------------------- 8

@pytest.mark.parametrize("resident", [False, True], ids=["half-batch chains", "resident launch"])
def test_a_save_beside_the_fast_paths_is_read_only(na, resident):
    import torch
    m = _model(na, "BossWN-standard.nam")
    S, n, steps = 1024, 128, 8
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(8)
    x = torch.clamp(0.25 * torch.randn(steps, S, n, generator=g), -1.0, 1.0).to(dev)
    want, got = torch.zeros(steps, S, n, device=dev), torch.zeros(steps, S, n, device=dev)
    ref, b = na.Batch(0), na.Batch(0)
    for bb in (ref, b):
        bb.AddStreams(m, S)
        if resident:
            bb.SetResidentLaunch(True)
    torch.cuda.synchronize(dev)
    for k in range(steps):
        ref.ProcessDevice(x[k].data_ptr(), want[k].data_ptr(), n)
    ref.Synchronize()
    blobs = []
    for k in range(steps):
        b.ProcessDevice(x[k].data_ptr(), got[k].data_ptr(), n)
        if not any(os.environ.get(kn) for kn in KNOBS):
            assert b.UsesResidentLaunch() == resident and (resident or b.UsesHalfLaunches())
        if k in (2, 5):  # mid-run: buffers are in flight on the chains / posted to the resident launch
            blobs.append(b.SaveStreams(np.arange(0, S, 97)))
    b.Synchronize()
    assert torch.equal(got, want)
    assert len(blobs[0]) == len(blobs[1]) and blobs[0] != blobs[1]
    # the blob taken after step 5 is the state after step 5: restored into a fresh batch it continues with steps 6, 7
    ids = np.arange(0, S, 97)
    c = na.Batch(0)
    c.AddStreams(m, ids.size, doPrewarm=False)
    c.LoadStreams(np.arange(ids.size), blobs[1])
    tail = np.concatenate([c.Process(x[k][ids].cpu().numpy()) for k in (6, 7)], axis=1)
    if c.StreamKernelName(0) == b.StreamKernelName(0):
        assert np.array_equal(tail, torch.cat([want[6][ids], want[7][ids]], dim=1).cpu().numpy())
    for bb in (ref, b, c):
        bb.close()
