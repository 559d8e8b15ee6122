"""Which route a processing call takes (neuralaudio_amd/csrc/host_route.h, NA_DebugLastHostRoute) on the smallest batches that reach
each one, and that the route does not change what is computed: every case drives one batch beside a twin with ONE entry point -- a batch
on a caller's stream through ProcessDevice, which always runs ordered -- and asserts the route, bit-equal rows for every live stream
and zero rows for parked ones.  The rule itself is checked on the CPU over all of its facts (test_host_route_cpu.py); here the entry
points gather the facts."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import na_oracle as O

pytestmark = pytest.mark.gpu
N = 32
# NA_HOST_DIRECT=0 (read once per process) sends host rows through the copy engines: test_the_small_batches_through_the_copy_engines
DIRECT = os.environ.get("NA_HOST_DIRECT", "1") != "0"
# the knobs that take a 512-stream batch off the chains (tests/test_gpu_pool.py): the rows are still compared, the routes are not
KNOBS = any(os.environ.get(k) for k in ("NA_WN_KERNEL", "NA_WN_SPEC", "NA_HOST_HALVES", "NA_SP_T", "NA_SP_GEN", "NA_RESIDENT")) or not DIRECT


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


@pytest.fixture(scope="module")
def models(na):
    loader = na.NeuralModelLoader()
    return {name: loader.CreateFromFile(os.path.join(O.MODELS_DIR, name), doPrewarm=False) for name in ("BossWN-standard.nam", "BossLSTM-1x16.nam")}


def _buffers(rows, count, seed):
    rng = np.random.default_rng(seed)
    base = np.clip(0.25 * rng.standard_normal((min(rows, 7), count * N)), -1.0, 1.0).astype(np.float32)
    x = base[np.arange(rows) % len(base)]
    return [np.ascontiguousarray(x[:, k * N:(k + 1) * N]) for k in range(count)]


def _route(na, batch):
    return na.HOST_ROUTES[batch.DebugLastHostRoute()]


class _Pair:
    """The batch under test and its twin, filled alike: `layout` = [(model, active, parked)], rows in that order."""

    def __init__(self, na, layout):
        import torch
        self.na, self.torch, self.dev = na, torch, torch.device("cuda", 0)
        self.ts = torch.cuda.Stream(device=self.dev)
        self.batch, self.twin = na.Batch(0), na.Batch(0, hip_stream=self.ts.cuda_stream)
        self.live = []
        for b in (self.batch, self.twin):
            for model, active, parked in layout:
                first = b.ReserveStreams(model, active + parked) if parked else b.AddStreams(model, active)
                for s in range(first, first + active):
                    if parked:
                        b.ActivateStream(s, 1.0)
                    if b is self.batch:
                        self.live.append(s)
        self.rows = self.batch.NumStreams()
        self.parked = [s for s in range(self.rows) if s not in self.live]

    def both(self, call):
        for b in (self.batch, self.twin):
            call(b)

    def device_rows(self, batch, x):
        """x through ProcessDevice of `batch`; the output rows start as zeros (a parked row is left alone)."""
        torch = self.torch
        dx = torch.from_numpy(x).to(self.dev)
        dy = torch.zeros_like(dx)
        torch.cuda.synchronize(self.dev)
        with torch.cuda.stream(self.ts):
            batch.ProcessDevice(dx.data_ptr(), dy.data_ptr(), N)
            batch.Synchronize()
        torch.cuda.synchronize(self.dev)
        return dy.cpu().numpy()

    def check(self, x, got, route, what, routes_hold=True):
        """`got`: the rows the batch under test produced for x by the route it reports; the twin runs x now."""
        taken = _route(self.na, self.batch)
        assert not routes_hold or taken == route, (what, taken)
        want = self.device_rows(self.twin, x)
        assert _route(self.na, self.twin) == "DeviceOrdered", what
        for s in self.live:
            assert np.array_equal(got[s], want[s]), (what, taken, "row", s, int(np.count_nonzero(got[s] != want[s])))
        for s in self.parked:
            assert not np.any(got[s]), (what, taken, "parked row", s)
        assert O.rms(got[self.live[0]]) > 1e-5 and O.rms(got[self.live[-1]]) > 1e-5, what  # (the streams ran: not silence)

    def close(self):
        self.batch.close()
        self.twin.close()


def _small_batches(na, models):
    std, lstm = models["BossWN-standard.nam"], models["BossLSTM-1x16.nam"]
    four = _Pair(na, [(std, 4, 1)])
    mixed = _Pair(na, [(std, 3, 1), (lstm, 3, 0)])
    return four, mixed


def test_every_route_of_a_small_batch(na, models):
    """4 x A1 Standard (and a parked fifth), 32 samples: the blocking call, registered blocks, a lone Submit, the same with a gain entry,
    ProcessDevice on the batch's own stream; 3 x Standard + 3 x LSTM 1x16 with a gain entry: several launch units on the copy streams."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    four, mixed = _small_batches(na, models)
    assert four.batch.DebugLastHostRoute() == -1
    xs = iter(_buffers(four.rows, 8, 31))
    x = next(xs)
    four.check(x, four.batch.Process(x), "StagedInPlace" if DIRECT else "StagedCopies", "blocking call")
    # blocks the caller registered: [in | out] back to back, the call gets pointers inside
    block = np.zeros((2, four.rows, N), dtype=np.float32)
    assert lib.NA_RegisterHostBuffer(block.ctypes.data_as(C.c_void_p), block.nbytes) == 0
    try:
        block[0], block[1] = next(xs), 7.0
        assert lib.NA_BatchProcess(four.batch._h, block[0].ctypes.data_as(C.POINTER(C.c_float)), block[1].ctypes.data_as(C.POINTER(C.c_float)), N) == 0
        four.check(block[0].copy(), block[1].copy(), "RegisteredInPlace" if DIRECT else "StagedCopies", "registered blocks")
    finally:
        assert lib.NA_UnregisterHostBuffer(block.ctypes.data_as(C.c_void_p)) == 0
    x = next(xs)
    ticket = four.batch.Submit(x)
    four.check(x, four.batch.Collect(ticket), "SubmitInPlace" if DIRECT else "SubmitOwnStream", "a lone Submit")
    x = next(xs)
    got = four.device_rows(four.batch, x)
    four.check(x, got, "DeviceOrdered", "ProcessDevice on the batch's own stream")
    # a stage with an entry: no read-modify-write over the bus, whatever the knob says
    four.both(lambda b: (b.EnableOutputStage(), b.SetStreamGain(1, 0.5)))
    x = next(xs)
    ticket = four.batch.Submit(x)
    four.check(x, four.batch.Collect(ticket), "SubmitOwnStream", "Submit with a gain entry")
    x = next(xs)
    four.check(x, four.batch.Process(x), "StagedCopies", "blocking call with a gain entry")
    four.close()

    xs = iter(_buffers(mixed.rows, 4, 32))
    x = next(xs)
    ticket = mixed.batch.Submit(x)
    mixed.check(x, mixed.batch.Collect(ticket), "SubmitInPlace" if DIRECT else "SubmitCopyStreams", "mixed batch, Submit")
    mixed.both(lambda b: (b.EnableOutputStage(), b.SetStreamGain(4, 0.5)))
    for k in range(2):  # (the second replays what the first captured, where the batch runs its units as a graph)
        x = next(xs)
        ticket = mixed.batch.Submit(x)
        mixed.check(x, mixed.batch.Collect(ticket), "SubmitCopyStreams", ("mixed batch with a gain entry, Submit", k))
    mixed.close()


def test_the_small_batches_through_the_copy_engines():
    """The case above once in a process with NA_HOST_DIRECT=0: the 4-stream batch's Submit rides on its slot's own stream, the mixed
    batch's on the copy streams, the blocking call goes through the copy engines."""
    if os.environ.get("NA_HOST_DIRECT"):
        pytest.skip("already inside a forced run")
    me = os.path.abspath(__file__) + "::test_every_route_of_a_small_batch"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", "-m", "gpu", "-p", "no:cacheprovider", me],
                       env=dict(os.environ, NA_HOST_DIRECT="0", NA_TEST_NO_WARM="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1500:]


def test_host_rows_to_device_rows_of_a_multi_gpu_shard(na, models):
    """ProcessHostToDevice has one caller: a shard of the multi-GPU host under RCCL fan-in (here two ranks on the loopback table)."""
    std = models["BossWN-standard.nam"]
    na.debug_set_rccl_api(1)
    try:
        multi = na.MultiBatch([0, 0])
        multi.SetFanIn("rccl")
        multi.AddStreams(std, 4)
        multi.Commit()
        pair = _Pair(na, [(std, 4, 0)])
        for k, x in enumerate(_buffers(4, 2, 33)):
            got = multi.Process(x)
            assert len(multi.ShardRanges()) == 2
            for shard in (0, 1):
                assert na.HOST_ROUTES[multi.DebugLastHostRoute(shard)] == ("ToDeviceInPlace" if DIRECT else "ToDeviceCopies")
            want = pair.device_rows(pair.twin, x)
            assert np.array_equal(got, want) and O.rms(got[0]) > 1e-5, k
        multi.close()
        pair.close()
    finally:
        na.debug_set_rccl_api(0)


def test_every_route_of_a_batch_that_fills_the_chains(na, models):
    """512 x A1 Standard, 32 samples -- 512 kernel-level streams is where PrepareHalves starts: the second of two tickets in flight
    rides the chains, the blocking call is staged in halves, ProcessDevice on the batch's own stream takes the chains; a gain entry then
    moves the next Submit to its slot's own stream, and the rows stay what the twin computes across the change."""
    pair = _Pair(na, [(models["BossWN-standard.nam"], 512, 0)])
    b, hold = pair.batch, not KNOBS
    pair.both(lambda bb: bb.EnableOutputStage())  # (no entry yet: nothing changes)
    xs = _buffers(512, 6, 34)
    tickets, routes = [], []
    for x in xs[:2]:
        b.NextInput(N)[:] = x
        tickets.append(b.SubmitInput(N))
        routes.append(_route(na, b))
    assert not hold or routes == ["SubmitInPlace", "SubmitHalves"], routes
    for x, ticket, route in zip(xs[:2], tickets, routes):
        pair.check(x, b.CollectView(ticket).copy(), route, ("two tickets in flight", route), routes_hold=False)
    pair.check(xs[2], b.Process(xs[2]), "StagedHalves", "blocking call", hold)
    got = pair.device_rows(b, xs[3])
    pair.check(xs[3], got, "DeviceHalves", "ProcessDevice on the batch's own stream", hold)
    b.NextInput(N)[:] = xs[4]
    ticket = b.SubmitInput(N)  # (a lone ticket, and the synchronisation above has drained the chains)
    pair.check(xs[4], b.CollectView(ticket).copy(), "SubmitInPlace", "a lone Submit behind drained chains", hold)
    pair.both(lambda bb: bb.SetStreamGain(300, 0.5))
    b.NextInput(N)[:] = xs[5]
    ticket = b.SubmitInput(N)
    pair.check(xs[5], b.CollectView(ticket).copy(), "SubmitOwnStream", "Submit with a gain entry")
    pair.close()
