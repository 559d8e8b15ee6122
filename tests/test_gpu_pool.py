"""GPU tests of the stream pool (NA_BatchReserveStreams / NA_BatchActivateStream / NA_BatchParkStream, csrc/gpu_batch.h):
join and leave for a batch that never stops.

ReserveStreams creates parked, ARMED streams on the set-up side; Activate / Park are host bookkeeping, and the processing call that
follows enqueues the list upload and one re-arm launch per model group.  What is checked here:
  1. an activated stream computes what a stream freshly added with AddStreams computes -- bit for bit against a twin batch, and within the
     suite's 2e-6 RMS of the CPU oracle's fresh model (the check that does not rest on the library alone);
  2. a parked stream carries nothing over, whatever it ran before;
  3. streams that did not join or leave never notice, also inside packed virtual streams;
  4. activate / park and the processing call behind them neither allocate nor wait for the device (a stalled device shows it);
  5. every entry point and launch schedule;
  6. the rules of the interface.
Every case drives clipped noise, so the state matters."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import na_oracle as O
import wide_cases as WC

pytestmark = pytest.mark.gpu

TOL_RMS = 2e-6  # the suite's WaveNet tolerance (tests/test_gpu_snapshot.py, test_gpu_offline.py, test_gpu_parity.py)
CONV_TAIL_STACK = "synthetic_stack_gru12_conv16k4d64elu_dense5softmax_dense1.json"
CALLS = (128, 1, 17, 300)


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


def _noise(n, seed, gain=0.25):
    rng = np.random.default_rng(seed)
    return np.clip(gain * rng.standard_normal(n), -1.0, 1.0).astype(np.float32)


# ---- the model families: name -> (model, oracle(quality, prewarm) -> object with .process(x)) ---------------------------------------

class _NumpyStack:
    """tests/ref_np.keras_stack_forward as an oracle object (one call: it starts from the model's fresh state)"""
    def __init__(self, mj, prewarm):
        self.mj, self.prewarm = mj, prewarm

    def process(self, x):
        import ref_np as R
        return R.keras_stack_forward(self.mj, x, prewarm=2048 if self.prewarm else 0).astype(np.float32)


def _wavenet_from_arrays(loader, arrays, seed, a1=None):
    w = O.synth_wavenet_weights(arrays, seed=seed)
    text = O.nam_json_wavenet_a1(a1[0], a1[1], w) if a1 else O.nam_json_wavenet_generic(arrays, w)
    return loader.CreateFromString(text, ".nam", doPrewarm=False), (lambda q, pw: O.OracleWaveNet(arrays, w, prewarm=pw))


def _lstm(loader, layers, hidden, seed):
    w = O.synth_lstm_weights(layers, hidden, seed)
    return (loader.CreateFromString(O.nam_json_lstm(layers, hidden, w), ".nam", doPrewarm=False),
            (lambda q, pw: O.OracleLSTM.from_nam(layers, hidden, w, prewarm=pw)))


def _family(na, name):
    loader = na.NeuralModelLoader()
    if name.endswith(".nam") or name.endswith(".json"):
        m = loader.CreateFromFile(os.path.join(O.MODELS_DIR, name), doPrewarm=False)
        if name == CONV_TAIL_STACK:
            mj = O.load_json(name)
            make = lambda q, pw: _NumpyStack(mj, pw)
        else:
            make = lambda q, pw: O.oracle_from_file(name, quality=q, prewarm=pw)
    elif name == "lite":
        m, make = _wavenet_from_arrays(loader, O.a1_arrays(12, 6), 41, a1=(12, 6))
    elif name.startswith("wide-"):
        c, h = (int(v) for v in name[5:].split("/"))
        m, make = _wavenet_from_arrays(loader, WC.two_array(c, h), c)
    elif name == "head-24":  # one array of 24 channels whose head is a convolution over time (a conv-head ring in the state)
        m, make = _wavenet_from_arrays(loader, WC.chain([24], [([3, 3, 2, 3], [1, 7, 64, 200])], head_kernel=4), 24)
    elif name.startswith("lstm-"):
        layers, hidden = (int(v) for v in name[5:].split("x"))
        m, make = _lstm(loader, layers, hidden, 7 + hidden)
    else:
        raise KeyError(name)
    assert m is not None, name
    m._loader = loader
    return m, make


FAMILIES = [("BossWN-standard.nam", 1.0), ("lite", 1.0), ("wide-20/10", 1.0), ("wide-80/40", 1.0), ("head-24", 1.0),
            ("BossLSTM-1x16.nam", 1.0), ("lstm-2x16", 1.0), ("synthetic_gru_1x16.json", 1.0), ("lstm-1x40", 1.0), (CONV_TAIL_STACK, 1.0),
            ("BossWN-a2.nam", 0.0), ("BossWN-a2.nam", 1.0)]


def _run_calls(batch, x, calls=CALLS):
    """x [rows, sum(calls)] through NA_BatchProcess in calls of those lengths"""
    out, pos = [], 0
    for n in calls:
        out.append(batch.Process(np.ascontiguousarray(x[:, pos:pos + n])))
        pos += n
    assert pos == x.shape[1]
    return np.concatenate(out, axis=1)


def _bit_equal(got, want, what):
    assert np.array_equal(got, want), (what, int(np.argmax(got != want)), int(np.count_nonzero(got != want)), O.rms(got - want))


# ---------------------------------------------------------------------------------------------------------------- 1

@pytest.mark.parametrize("prewarm", [True, False], ids=["prewarmed", "fresh"])
@pytest.mark.parametrize("name,quality", FAMILIES)
def test_an_activated_stream_equals_a_freshly_added_one(na, name, quality, prewarm):
    """Reserve 6, run 300 samples with everybody parked, activate ids 4 and 1, run calls of 128, 1, 17 and 300 samples: the two rows are
    the rows of a twin batch built with AddStreams bit for bit, and the CPU oracle's fresh model to 2e-6 RMS."""
    m, make = _family(na, name)
    rows, total = 6, sum(CALLS)
    x = np.stack([_noise(total, 300 + r) for r in range(rows)])
    pool = na.Batch(0)
    assert pool.ReserveStreams(m, rows, doPrewarm=prewarm) == 0
    assert pool.NumStreams() == rows and pool.NumParked() == rows and pool.NumLiveStreams() == 0
    idle = pool.Process(np.stack([_noise(300, 900 + r) for r in range(rows)]))
    assert not np.any(idle), "parked rows give silence"
    pool.ActivateStream(4, quality)
    pool.ActivateStream(1, quality)
    y = _run_calls(pool, x)
    twin = na.Batch(0)
    twin.AddStreams(m, rows, quality=quality, doPrewarm=prewarm)
    assert pool.StreamKernelName(4) == twin.StreamKernelName(4) != ""
    yt = _run_calls(twin, x)
    for r in range(rows):
        if r in (4, 1):
            err = O.rms(y[r] - make(quality, prewarm).process(x[r]))
            print("%s q=%g %s row %d on %s: %d samples differ from the twin, rms vs oracle %.3g"
                  % (name, quality, "prewarmed" if prewarm else "fresh", r, pool.StreamKernelName(r), int(np.count_nonzero(y[r] != yt[r])), err))
            _bit_equal(y[r], yt[r], (name, r))
            assert err < TOL_RMS, (name, r, err)
        else:
            assert not np.any(y[r]), r
    pool.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------- 2

@pytest.mark.parametrize("name,quality", FAMILIES)
def test_a_parked_stream_carries_nothing_over(na, name, quality):
    """A stream runs loud noise for two receptive fields (recurrent models: 5000 samples), is parked over two buffers and activated: it is
    a freshly added stream again, bit for bit.  So it is after park -> activate with no processing call in between, and a stream that
    was activated and parked again without a processing call in between never ran and is still armed."""
    m, make = _family(na, name)
    rf = m.GetReceptiveFieldSize()
    loud_n = 2 * rf if rf > 0 else 5000
    calls = (128, 17, 300)
    xf = _noise(sum(calls), 77)
    twin = na.Batch(0)
    twin.AddStreams(m, 1, quality=quality)
    fresh = _run_calls(twin, xf[None, :], calls)[0]
    twin.close()

    b = na.Batch(0)
    b.ReserveStreams(m, 3)
    b.ActivateStream(0, quality)  # (a neighbour that keeps running)
    b.ActivateStream(1, quality)

    def run(active_row, n=None):
        blk = np.stack([_noise(sum(calls), 500 + r) for r in range(3)])
        if active_row is not None:
            blk[active_row] = xf
        if n is not None:
            return _run_calls(b, blk[:, :n], (n,))
        return _run_calls(b, blk, calls)

    loud = np.stack([_noise(loud_n, 40 + r, gain=0.6) for r in range(3)])
    for i in range(0, loud_n, 2048):
        b.Process(np.ascontiguousarray(loud[:, i:i + 2048]))
    b.ParkStream(1)
    for _ in range(2):
        y = run(None, 128)
        assert not np.any(y[1]) and not np.any(y[2]) and np.any(y[0])
    b.ActivateStream(1, quality)
    y = run(1)
    print("%s q=%g: after loud noise + park: %d samples differ from a fresh stream" % (name, quality, int(np.count_nonzero(y[1] != fresh))))
    _bit_equal(y[1], fresh, (name, "park, two buffers, activate"))
    # park -> activate with no processing call in between
    b.ParkStream(1)
    b.ActivateStream(1, quality)
    _bit_equal(run(1)[1], fresh, (name, "park, activate"))
    # activate -> park with none in between: the stream never ran
    b.ActivateStream(2, quality)
    b.ParkStream(2)
    y = run(None, 128)
    assert not np.any(y[2])
    b.ActivateStream(2, quality)
    _bit_equal(run(2)[2], fresh, (name, "activate, park, buffer, activate"))
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 3

def test_live_streams_never_notice_the_pool(na):
    """Four live A1 Standard streams and two pooled ones that join and leave on a fixed schedule over 20 buffers: the four are
    bit-identical to a batch without a pool, and each pooled stream starts every visit like a fresh one."""
    m, _ = _family(na, "BossWN-standard.nam")
    n, buffers = 128, 20
    x = np.stack([_noise(n * buffers, 60 + r) for r in range(6)])
    ref = na.Batch(0)
    ref.AddStreams(m, 4)
    want = _run_calls(ref, x[:4], (n,) * buffers)
    b = na.Batch(0)
    assert b.AddStreams(m, 4) == 0 and b.ReserveStreams(m, 2) == 4
    # buffer -> operations in front of it
    schedule = {2: [("a", 4)], 3: [("a", 5)], 6: [("p", 4)], 7: [("a", 4), ("p", 5)], 11: [("p", 4), ("a", 5)], 12: [("a", 4)], 17: [("p", 4), ("p", 5)], 18: [("a", 5)]}
    twins, got = {}, []  # a pooled stream's twin: a batch with one stream added when it joined
    for k in range(buffers):
        for op, s in schedule.get(k, []):
            if op == "a":
                b.ActivateStream(s, 1.0)
                twins[s] = na.Batch(0)
                twins[s].AddStreams(m, 1)
            else:
                b.ParkStream(s)
                twins.pop(s).close()
        y = b.Process(np.ascontiguousarray(x[:, k * n:(k + 1) * n]))
        got.append(y[:4])
        for s in (4, 5):
            if s in twins:
                _bit_equal(y[s], twins[s].Process(np.ascontiguousarray(x[s:s + 1, k * n:(k + 1) * n]))[0], ("pooled stream", s, "buffer", k))
            else:
                assert not np.any(y[s]), (k, s)
    _bit_equal(np.concatenate(got, axis=1), want, "the four live streams")
    b.close()
    ref.close()


@pytest.mark.parametrize("name,pack", [("BossWN-nano.nam", 4), ("BossWN-feather.nam", 2)])
def test_neighbours_inside_a_packed_virtual_stream_never_notice(na, name, pack):
    """1028 parked streams of a narrow model cost nothing (parked streams do not run).  Members 0, 1, 5 and 1027 join; member 1 is parked
    and activated again while member 0 -- its neighbour in the same virtual stream -- runs.  Every row is the unpacked computation to the
    usual tolerance (the CPU oracle's fresh model: every in-process batch of this model packs), row 0 is bit-identical to a run in
    which member 1 never moved."""
    m, make = _family(na, name)
    S, n = 1028, 128
    ids = (0, 1, 5, 1027)
    phases = (3, 2, 4)  # buffers: all four, without member 1, with it again
    x = {s: _noise(n * sum(phases), 700 + s) for s in ids}

    def run(move):
        b = na.Batch(0)
        assert b.ReserveStreams(m, S) == 0
        assert b.StreamPackFactor(0) == pack
        for s in ids:
            b.ActivateStream(s, 1.0)
        assert all(b.StreamPackFactor(s) == pack for s in ids)
        out = {s: [] for s in ids}
        blk = np.zeros((S, n), np.float32)
        k = 0
        for phase, count in enumerate(phases):
            if move and phase == 1:
                b.ParkStream(1)
            if move and phase == 2:
                b.ActivateStream(1, 1.0)
            for _ in range(count):
                for s in ids:
                    blk[s] = x[s][k * n:(k + 1) * n]
                y = b.Process(blk)
                assert not np.any(y[2]) and not np.any(y[1026])
                for s in ids:
                    out[s].append(y[s].copy())
                k += 1
        b.close()
        return {s: np.concatenate(v) for s, v in out.items()}

    moved, still = run(True), run(False)
    _bit_equal(moved[0], still[0], "member 0 while member 1 left and came back")
    for s in (5, 1027):
        _bit_equal(moved[s], still[s], ("member", s))
    for s in ids:
        err = O.rms(still[s] - make(1.0, True).process(x[s]))
        print("%s member %d: rms vs the unpacked oracle %.3g" % (name, s, err))
        assert err < TOL_RMS, (s, err)
    a, c = phases[0] * n, (phases[0] + phases[1]) * n
    assert not np.any(moved[1][a:c])
    _bit_equal(moved[1][:a], still[1][:a], "member 1 before it left")
    err = O.rms(moved[1][c:] - make(1.0, True).process(x[1][c:]))
    print("%s member 1 after it came back: rms vs a fresh oracle %.3g" % (name, err))
    assert err < TOL_RMS, err


# ---------------------------------------------------------------------------------------------------------------- 4

STALL_MS = 400.0


def test_activate_park_and_the_next_buffer_neither_allocate_nor_wait(na):
    """A batch on a caller's stream, 8 A1 Standard + 8 LSTM 1x16 reserved, a few active.  Behind NA_DebugStallDevice(400) the sequence
    Park, Activate, Activate, ProcessDevice -- two re-arm launches and two list uploads among its device work -- returns in under half
    the stall (one synchronise or one hipFree in it would cost the rest of the stall), a Synchronize issued afterwards returns no
    earlier than the stall's end, NA_DebugDeviceResourceCalls has not moved, and the outputs are the twin's."""
    import torch
    from neuralaudio_amd import capi
    lib = capi.load_library()
    dev = torch.device("cuda", 0)
    std, _ = _family(na, "BossWN-standard.nam")
    lstm, _ = _family(na, "BossLSTM-1x16.nam")
    n, rows, buffers = 128, 16, 6
    stream = torch.cuda.Stream(dev)
    b = na.Batch(0, hip_stream=stream.cuda_stream)
    assert b.GetWaitLimitMs() == 2000.0
    assert b.ReserveStreams(std, 8) == 0 and b.ReserveStreams(lstm, 8) == 8
    xs = [np.stack([_noise(n, 1000 * k + r) for r in range(rows)]) for k in range(buffers)]
    dx = [torch.from_numpy(v).to(dev) for v in xs]
    dy = [torch.zeros(rows, n, device=dev) for _ in xs]
    torch.cuda.synchronize(dev)

    def step(k):
        b.ProcessDevice(dx[k].data_ptr(), dy[k].data_ptr(), n, n, n)

    for s in (0, 2, 1, 8, 9, 10):
        b.ActivateStream(s, 1.0)
    step(0)
    # the warm-up cycle: streams 1 (WaveNet) and 10 (LSTM) leave, come back -- the first re-arm launches -- and leave again
    b.ParkStream(1)
    b.ParkStream(10)
    step(1)
    b.ActivateStream(1, 1.0)
    b.ActivateStream(10, 1.0)
    step(2)
    b.ParkStream(1)
    b.ParkStream(10)
    step(3)
    b.Synchronize()
    calls = lib.NA_DebugDeviceResourceCalls()
    b.DebugStallDevice(STALL_MS)
    t0 = time.monotonic()
    b.ParkStream(2)
    b.ActivateStream(1, 1.0)
    b.ActivateStream(10, 1.0)
    step(4)
    dt = time.monotonic() - t0
    b.Synchronize()
    total = time.monotonic() - t0
    moved = lib.NA_DebugDeviceResourceCalls() - calls
    print("park + 2 activates + ProcessDevice behind a %.0f ms stall: %.2f ms; synchronised after %.0f ms; resource calls %d" % (STALL_MS, dt * 1e3, total * 1e3, moved))
    assert dt < 0.5 * STALL_MS / 1000.0, dt
    assert total >= 0.95 * STALL_MS / 1000.0, total  # (the device really was stalled while the calls returned)
    assert moved == 0
    assert not b.IsBroken()
    step(5)
    b.Synchronize()
    got = [v.cpu().numpy() for v in dy]

    def twin_rows(ks):
        t = na.Batch(0)
        t.AddStreams(std, 8)
        t.AddStreams(lstm, 8)
        out = {k: t.Process(xs[k]) for k in ks}
        t.close()
        return out

    whole, visit2, visit3 = twin_rows(range(buffers)), twin_rows([2]), twin_rows([4, 5])
    for k in range(buffers):
        for r in (0, 8, 9):
            _bit_equal(got[k][r], whole[k][r], ("live row", r, "buffer", k))
        if k < 4:
            _bit_equal(got[k][2], whole[k][2], ("row 2 before it left", k))
    for r in (1, 10):
        _bit_equal(got[0][r], whole[0][r], ("row", r, "first visit"))
        _bit_equal(got[2][r], visit2[2][r], ("row", r, "second visit"))
        for k in (4, 5):
            _bit_equal(got[k][r], visit3[k][r], ("row", r, "third visit, buffer", k))
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 5

def test_a_join_between_two_tickets_and_through_host_blocks(na):
    """Submit / Collect with a join between two tickets in flight, then NA_BatchProcess on a pageable and on a registered block."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    m, _ = _family(na, "BossWN-standard.nam")
    n, rows = 128, 5
    x = np.stack([_noise(n * 6, 80 + r) for r in range(rows)])
    blk = lambda k: np.ascontiguousarray(x[:, k * n:(k + 1) * n])
    b = na.Batch(0)
    assert b.AddStreams(m, 2) == 0 and b.ReserveStreams(m, 3) == 2
    twin = na.Batch(0)
    twin.AddStreams(m, 2)
    late = na.Batch(0)  # rows 3 (joins before buffer 1) and 2 (joins before buffer 4) as fresh streams
    late.AddStreams(m, 1)
    late2 = na.Batch(0)
    late2.AddStreams(m, 1)
    t0 = b.Submit(blk(0))
    b.ActivateStream(3, 1.0)  # ticket 0 is in flight
    t1 = b.Submit(blk(1))
    y0, y1 = b.Collect(t0), b.Collect(t1)
    assert not np.any(y0[2:]) and not np.any(y1[2]) and not np.any(y1[4])
    y2 = b.Collect(b.Submit(blk(2)))
    y3 = b.Process(blk(3))  # pageable
    b.ActivateStream(2, 1.0)
    reg = np.zeros((2, rows, n), np.float32)
    assert lib.NA_RegisterHostBuffer(reg.ctypes.data_as(C.c_void_p), reg.nbytes) == 0
    try:
        ys = [y0, y1, y2, y3]
        for k in (4, 5):
            reg[0] = blk(k)
            assert lib.NA_BatchProcess(b._h, reg[0].ctypes.data_as(C.POINTER(C.c_float)), reg[1].ctypes.data_as(C.POINTER(C.c_float)), n) == 0, capi.last_error()
            ys.append(reg[1].copy())
    finally:
        assert lib.NA_UnregisterHostBuffer(reg.ctypes.data_as(C.c_void_p)) == 0
    for k in range(6):
        yt = twin.Process(blk(k)[:2])
        _bit_equal(ys[k][:2], yt, ("rows 0-1, buffer", k))
        if k >= 1:
            _bit_equal(ys[k][3], late.Process(blk(k)[3:4])[0], ("row 3, buffer", k))
        if k >= 4:
            _bit_equal(ys[k][2], late2.Process(blk(k)[2:3])[0], ("row 2, buffer", k))
        assert not np.any(ys[k][4])
    for bt in (b, twin, late, late2):
        bt.close()


def test_a_join_or_leave_that_changes_the_launch_units_creates_nothing_in_submit(na):
    """Submit / Collect on a pooled WaveNet + LSTM batch whose streams of ONE family run.  The first LSTM stream joins (one launch unit
    becomes two: another schedule of streams and events inside Submit), leaves again (back to one), then the batch goes over to the
    LSTM alone.  Once every pipeline slot has been used NA_DebugDeviceResourceCalls does not move: what either schedule needs was
    created by ReserveStreams.  The rows equal their twins bit for bit."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    std, _ = _family(na, "BossWN-standard.nam")
    lstm, _ = _family(na, "BossLSTM-1x16.nam")
    n, rows, buffers = 128, 6, 12
    x = np.stack([_noise(n * buffers, 300 + r) for r in range(rows)])
    blk = lambda k: np.ascontiguousarray(x[:, k * n:(k + 1) * n])
    b = na.Batch(0)
    assert b.ReserveStreams(std, 3) == 0 and b.ReserveStreams(lstm, 3) == 3
    b.ActivateStream(0, 1.0)
    b.ActivateStream(1, 1.0)
    # buffer -> operations in front of it; rows 0, 1 run buffers 0-9, row 3 buffers 4-5 and, as a new stream, 8-11
    schedule = {4: [("a", 3)], 6: [("p", 3)], 8: [("a", 3)], 10: [("p", 0), ("p", 1)]}
    ys, moved = [], []
    pending = b.Submit(blk(0))
    calls = None
    for k in range(1, buffers + 1):
        if k == 4:  # (every slot has carried a buffer: its pinned blocks exist)
            calls = lib.NA_DebugDeviceResourceCalls()
        for op, s in schedule.get(k, []):
            (b.ActivateStream(s, 1.0) if op == "a" else b.ParkStream(s))
        nxt = b.Submit(blk(k)) if k < buffers else None  # (two tickets in flight)
        ys.append(b.Collect(pending))
        pending = nxt
        if calls is not None:
            moved.append(lib.NA_DebugDeviceResourceCalls() - calls)
    print("device resource calls since buffer 4, per buffer:", moved)
    assert moved[-1] == 0, moved
    twin = na.Batch(0)
    twin.AddStreams(std, 2)
    for k in range(10):
        _bit_equal(ys[k][:2], twin.Process(blk(k)[:2]), ("rows 0-1, buffer", k))
    for visit in ((4, 5), (8, 9, 10, 11)):
        t = na.Batch(0)
        t.AddStreams(lstm, 1)
        for k in visit:
            _bit_equal(ys[k][3], t.Process(blk(k)[3:4])[0], ("row 3, buffer", k))
        t.close()
    for k in range(buffers):
        live = {0, 1} if k < 10 else set()
        live |= {3} if k in (4, 5, 8, 9, 10, 11) else set()
        for r in set(range(rows)) - live:
            assert not np.any(ys[k][r]), (r, k)
    twin.close()
    b.close()


def test_the_same_through_the_copy_engines():
    """The host-buffer entry points run kernels on the pinned blocks by default; NA_HOST_DIRECT=0 (read once per process) sends the blocks
    through the copy engines instead: per-slot streams while a buffer is one launch, two copy streams when it is several.  That is
    where a change of the number of launch units changes which streams Submit needs, so the test above runs once in such a process."""
    import subprocess
    import sys
    if os.environ.get("NA_HOST_DIRECT"):
        pytest.skip("already inside a forced run")
    me = os.path.abspath(__file__) + "::test_a_join_or_leave_that_changes_the_launch_units_creates_nothing_in_submit"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-m", "gpu", "-p", "no:cacheprovider", me],
                       env=dict(os.environ, NA_HOST_DIRECT="0", NA_TEST_NO_WARM="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1500:]


def test_a_mixed_batch_recaptures_its_launch_graph(na):
    """WaveNet + LSTM streams: several launch units per buffer (fork / join, a captured hipGraph where the runtime is trusted with one).
    Joins and leaves change the lists the captured launches hold and, when a group gains its first or loses its last stream, the units."""
    std, _ = _family(na, "BossWN-standard.nam")
    lstm, _ = _family(na, "BossLSTM-1x16.nam")
    n, rows, buffers = 128, 6, 8
    x = np.stack([_noise(n * buffers, 90 + r) for r in range(rows)])
    b = na.Batch(0)
    assert b.ReserveStreams(std, 3) == 0 and b.ReserveStreams(lstm, 3) == 3
    # buffer -> operations in front of it
    schedule = {0: [("a", 0)], 1: [("a", 3)], 2: [("a", 1), ("a", 4)], 4: [("p", 3), ("p", 4)], 5: [("a", 5)], 6: [("p", 0), ("p", 1)], 7: [("a", 2)]}
    since = {}
    twins = {}
    for k in range(buffers):
        for op, s in schedule.get(k, []):
            if op == "a":
                b.ActivateStream(s, 1.0)
                twins[s] = na.Batch(0)
                twins[s].AddStreams(std if s < 3 else lstm, 1)
            else:
                b.ParkStream(s)
                twins.pop(s).close()
        y = b.Process(np.ascontiguousarray(x[:, k * n:(k + 1) * n]))
        for s in range(rows):
            if s in twins:
                _bit_equal(y[s], twins[s].Process(np.ascontiguousarray(x[s:s + 1, k * n:(k + 1) * n]))[0], ("row", s, "buffer", k))
            else:
                assert not np.any(y[s]), (s, k)
    b.close()


def test_half_batch_chains_survive_a_park_and_an_activate(na):
    """An own-stream batch of 516 reserved / 512 active A1 Standard streams runs its device-pointer buffers as half-batch launches,
    before and after a park + activate (which drain the chains: the one host-side wait of the contract)."""
    import torch
    dev = torch.device("cuda", 0)
    m, _ = _family(na, "BossWN-standard.nam")
    S, act, n = 516, 512, 128
    b = na.Batch(0)
    assert b.ReserveStreams(m, S) == 0
    for s in range(act):
        b.ActivateStream(s, 1.0)
    twin = na.Batch(0)
    twin.AddStreams(m, S)
    base = np.stack([_noise(n * 4, 10 + r) for r in range(7)])
    x = base[np.arange(S) % 7]
    dx = torch.from_numpy(x).to(dev)
    dy = torch.zeros(S, n * 4, device=dev)
    torch.cuda.synchronize(dev)
    knobs = any(os.environ.get(k) for k in ("NA_WN_KERNEL", "NA_WN_SPEC", "NA_HOST_HALVES", "NA_SP_T", "NA_SP_GEN", "NA_RESIDENT"))

    def step(k):
        b.ProcessDevice(dx.data_ptr() + 4 * k * n, dy.data_ptr() + 4 * k * n, n, 4 * n, 4 * n)

    step(0)
    step(1)
    b.WaitOutputs()
    assert knobs or b.UsesHalfLaunches()
    b.ParkStream(7)
    b.ActivateStream(514, 1.0)
    step(2)
    b.ActivateStream(7, 1.0)  # (it ran: a re-arm, behind the chains)
    step(3)
    b.Synchronize()
    assert knobs or b.UsesHalfLaunches()
    got = dy.cpu().numpy()
    want = np.concatenate([twin.Process(np.ascontiguousarray(x[:, k * n:(k + 1) * n])) for k in range(4)], axis=1)
    for r in (0, 6, 8, 255, 256, 511):
        _bit_equal(got[r], want[r], ("row", r))
    _bit_equal(got[7, :2 * n], want[7, :2 * n], "row 7 before it left")
    fresh = na.Batch(0)
    fresh.AddStreams(m, 1)
    yf = np.concatenate([fresh.Process(np.ascontiguousarray(x[514:515, k * n:(k + 1) * n])) for k in (2, 3)], axis=1)
    _bit_equal(got[514, 2 * n:], yf[0], "row 514 from its first buffer")
    again = na.Batch(0)
    again.AddStreams(m, 1)
    _bit_equal(got[7, 3 * n:], again.Process(np.ascontiguousarray(x[7:8, 3 * n:]))[0], "row 7 after it came back")
    again.close()
    for bt in (b, twin, fresh):
        bt.close()


def test_a_resampling_batch_starts_the_joiner_at_the_batch_phase(na):
    """44.1 -> 48 kHz, default quantum: the activated row equals row 0 of a fresh resampling batch that was fed the same number of
    external samples first (the phase is the batch's; a joining stream starts from zero filter histories at it)."""
    m, _ = _family(na, "BossWN-standard.nam")
    calls = (441, 100, 441, 37)
    lead = (441, 300)
    x = np.stack([_noise(sum(lead) + sum(calls), 120 + r) for r in range(3)])
    b = na.Batch(0)
    b.SetResampling(44100)
    assert b.ReserveStreams(m, 3) == 0
    b.ActivateStream(0, 1.0)
    head = _run_calls(b, x[:, :sum(lead)], lead)
    assert not np.any(head[1:])
    b.ActivateStream(2, 1.0)
    y = _run_calls(b, x[:, sum(lead):], calls)
    twin = na.Batch(0)
    twin.SetResampling(44100)
    # the same number of external samples first: the phase is the batch's; then a fresh stream joins it
    twin.AddStreams(m, 1)
    _run_calls(twin, x[:1, :sum(lead)], lead)
    assert twin.AddStreams(m, 1) == 1
    yt = _run_calls(twin, x[[0, 2], sum(lead):], calls)
    _bit_equal(y[2], yt[1], "the activated row")
    _bit_equal(y[0], yt[0], "the row that was there")
    assert not np.any(y[1])
    b.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------- 6

def test_the_rules(na):
    std, _ = _family(na, "BossWN-standard.nam")
    lstm, _ = _family(na, "BossLSTM-1x16.nam")
    a2, _ = _family(na, "BossWN-a2.nam")
    b = na.Batch(0)
    assert b.AddStreams(std, 2) == 0
    assert b.ReserveStreams(lstm, 2) == 2 and b.ReserveStreams(std, 3) == 4 and b.ReserveStreams(a2, 1) == 7
    assert (b.NumStreams(), b.NumLiveStreams(), b.NumParked()) == (8, 2, 6)
    assert b.FindParked(std) == 4 and b.FindParked(lstm) == 2 and b.FindParked(a2) == 7
    assert b.IsParked(4) and not b.IsLive(4) and not b.IsParked(0) and b.IsLive(0) and not b.IsParked(99) and not b.IsParked(-1)
    for bad in (0, 99, -1):  # live, out of range
        with pytest.raises(na.NeuralAudioError, match="not a parked stream"):
            b.ActivateStream(bad, 1.0)
    with pytest.raises(na.NeuralAudioError, match="did not come from ReserveStreams"):
        b.ParkStream(1)
    with pytest.raises(na.NeuralAudioError, match="parked"):
        b.ParkStream(4)
    for call in (lambda: b.SetQuality(7, 0.0), lambda: b.Prewarm(4), lambda: b.SaveStreams([0, 4]), lambda: b.LoadStreams([4], b"")):
        with pytest.raises(na.NeuralAudioError, match="parked"):
            call()
    b.Prewarm(-1)  # skips the parked ones
    b.ActivateStream(4, 1.0)
    assert (b.NumStreams(), b.NumLiveStreams(), b.NumParked()) == (8, 3, 5)
    assert b.FindParked(std) == 5 and b.IsLive(4)
    with pytest.raises(na.NeuralAudioError, match="not a parked stream"):
        b.ActivateStream(4, 1.0)
    b.ActivateStream(7, 0.0)
    assert b.GetActiveSubModel(7) == O.quality_to_submodel(O.load_json("BossWN-a2.nam"), 0.0) and b.FindParked(a2) == -1
    b.ParkStream(7)
    b.ActivateStream(7, 1.0)
    assert b.GetActiveSubModel(7) == O.quality_to_submodel(O.load_json("BossWN-a2.nam"), 1.0)
    # RemoveStreams frees a parked stream like any other; its id is recycled
    b.RemoveStreams(5)
    assert (b.NumStreams(), b.NumLiveStreams(), b.NumParked()) == (8, 4, 3)
    with pytest.raises(na.NeuralAudioError, match="not a parked stream"):
        b.ActivateStream(5, 1.0)  # removed
    assert b.ReserveStreams(lstm, 1) == 5 and b.IsParked(5) and b.FindParked(lstm) == 2
    b.ParkStream(4)
    assert b.FindParked(std) == 4
    y = b.Process(np.stack([_noise(128, r) for r in range(8)]))
    assert np.any(y[0]) and np.any(y[7]) and not np.any(y[2:7])
    b.close()


def test_a_snapshot_of_an_activated_stream_continues_in_an_added_one(na):
    m, _ = _family(na, "BossWN-standard.nam")
    n1, n2 = 128 * 5 + 17, 128 * 3
    x = _noise(n1 + n2, 5)
    b = na.Batch(0)
    b.ReserveStreams(m, 3)
    b.ActivateStream(1, 1.0)
    blk = np.zeros((3, n1), np.float32)
    blk[1] = x[:n1]
    y1 = b.Process(blk)[1]
    blob = b.SaveStreams([1])
    blk2 = np.zeros((3, n2), np.float32)
    blk2[1] = x[n1:]
    want = b.Process(blk2)[1]
    c = na.Batch(0)
    c.AddStreams(m, 1, doPrewarm=False)
    c.LoadStreams([0], blob)
    _bit_equal(c.Process(x[None, n1:])[0], want, "the loaded stream")
    whole = na.Batch(0)
    whole.AddStreams(m, 1)
    _bit_equal(np.concatenate([y1, want]), whole.Process(x[None, :])[0], "the activated stream against an added one")
    for bt in (b, c, whole):
        bt.close()
