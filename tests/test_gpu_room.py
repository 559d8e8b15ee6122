"""GPU tests of the room stage (csrc/room_stage.h).  The contract states every f32 operation and its order, so the expected
value is the numpy float32 restatement of tests/room_cases.py and every comparison is on the bits.  The first tests drive the stage through
its hook (NA_DebugRunRoomStage) on rows that stand in for model outputs; the others run a batch of the smallest committed model."""
import numpy as np
import pytest

import handover_cases as H
import room_cases as K
from mod_cases import signal

pytestmark = pytest.mark.gpu
F = np.float32
ROWS = 6


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    if neuralaudio_amd.device_count() < 1:
        pytest.fail("no HIP device visible: the product path has no CPU fallback")
    return neuralaudio_amd


@pytest.fixture(scope="module")
def nano(na):
    loader = na.NeuralModelLoader()
    return loader, loader.CreateFromFile(H.os.path.join(H.O.MODELS_DIR, H.NANO), doPrewarm=False)


launches = lambda: __import__("neuralaudio_amd").capi.load_library().NA_DebugRoomLaunches()
bits = lambda a: np.ascontiguousarray(a, F).view(np.uint32)
noise_rows = lambda total, seed: np.stack([signal(seed + r, total) for r in range(ROWS)])


def assert_same(y, e, what=()):
    for row in range(y.shape[0]):
        diff = np.flatnonzero(bits(y[row]) != bits(e[row]))
        assert len(diff) == 0, what + ("row", row, "first at", int(diff[0]), float(y[row][diff[0]]), float(e[row][diff[0]]), "of", len(diff))


def make(na, nano, max_line):
    b = na.Batch(0)
    assert b.AddStreams(nano[1], ROWS, doPrewarm=False) == 0
    if max_line:
        b.EnableRoomStage(max_line)
    return b


def hook_run(b, ops, x, calls):
    """the stage alone over x[ROWS, total] cut into `calls`, rows an odd stride apart; ops as room_cases.run_cuts takes them"""
    out, pos = [], 0
    for c, n in enumerate(calls):
        for row, p, fade in ops.get(c, ()):
            b.SetStreamRoom(row, p, fade)
        block = np.full((ROWS, n + 3), F(7.0))
        block[:, :n] = x[:, pos:pos + n]
        b.DebugRunRoomStage(block, n)
        assert np.all(block[:, n:] == F(7.0)), "the stage wrote past the end of a row"
        out.append(block[:, :n].copy())
        pos += n
    return np.concatenate(out, axis=1)


@pytest.mark.parametrize("edge", sorted(K.EDGES))
def test_lengths_at_the_edges(na, nano, edge):
    """The three length sets of room_cases.EDGES: four settings on four rows (feedback at its bound with damp 0.5, a fade in, wet alone)
    over calls around the piece's length, and a live change on row 0 -- lengths (every read head cross-fades), feedback, damp and wet
    fade over 900 samples across three calls.  Rows 4 and 5 have no entry and keep their bits, NaN included."""
    max_line, lines = K.EDGES[edge]
    calls = [333, 128, 1, 129, 700, 127, 682]
    x = noise_rows(sum(calls), 10)
    ops = {0: [(0, K.params(lines, 0.3, 0.25, 0.5, 0.75), 0), (1, K.params(lines[::-1], K.MAX_FEEDBACK, 0.5, 1.0, 0.5), 0), (2, K.params(lines, 0.35, 0.1), 200)],
           2: [(3, K.params(lines[4:] + lines[:4], [0.05 * i for i in range(8)], 0.0, 1.0, 0.0), 0)], 3: [(0, K.params(lines[::-1], K.MAX_FEEDBACK, 0.5, 1.0, 0.5), 900)]}
    b = make(na, nano, max_line)
    info = b.GetRoomInfo()
    assert (info["maxLineSamples"], info["ringSamples"], info["pieceSamples"], info["numRooms"]) == (max_line, 2 * max_line, 128, 0)
    assert info["deviceBytes"] >= 16 * 8 * 2 * max_line * 4
    before = launches()
    y = hook_run(b, ops, x, calls)
    assert launches() - before == len(calls), "one launch per call, whatever its length"
    assert b.GetRoomInfo()["numRooms"] == 4 and b.GetStreamRoom(0) == ops[3][0][1] and b.GetStreamRoom(4) is None and b.StreamRoomFadeRemaining(0) == 0
    b.close()
    assert_same(y, K.run_cuts(ops, x, calls)[0], (edge,))
    assert np.array_equal(bits(y[4:]), bits(x[4:])) and np.isnan(x[4]).any() and not np.array_equal(bits(y[0]), bits(x[0]))


def test_the_known_answer(na, nano):
    """damp 0, feedback 0.25, every line 128, wet 1, dry 0: H8 of equal values is 8 e_0 and H8 of e_0 is all ones, so an impulse comes
    back as 2^(2 - m) at t = 256 m and +0 elsewhere -- exact, down through the subnormals to 2^-148, after which fl(0.25 * 2^-148)
    ties to +0.  A build that flushes to zero ends at 2^-126; one that contracts or reorders leaves residues beside the powers."""
    n = 256 * 152
    x = np.zeros((ROWS, n), F)
    x[0, 0] = x[1, 5] = 1.0
    p = K.params([128] * 8, 0.25, 0.0, 1.0, 0.0)
    b = make(na, nano, 256)
    y = hook_run(b, {0: [(0, p, 0), (1, p, 0)]}, x, [n])
    b.close()
    want = np.zeros(n, F)
    m = np.arange(1, 151)
    want[256 * m] = np.ldexp(1.0, 2 - m).astype(F)
    assert want[256 * 150] == 2.0 ** -148 and 0 < want[256 * 130] < np.finfo(F).tiny and np.count_nonzero(want) == 150
    assert_same(y[:2], np.stack([want, np.roll(want, 5)]))
    assert not y[2:].any()


def test_neighbours_removal_and_recycling(na, nano):
    """Rows with and without entries in one batch; NULL fades row 0 out over 300 samples, the call in which the fade ends leaves the rest
    of its row untouched and the row then passes bit for bit without a launch; row 1 runs a loud line, its stream is removed and its id
    recycled: the new entry reads +0 by position, not what the rings hold."""
    lines = K.EDGES["at-max"][1]
    calls = [400, 200, 250, 150, 300]
    x = noise_rows(sum(calls), 20)
    with np.errstate(over="ignore"):
        x[1, :600] *= F(1e6)
    loud, soft = K.params(lines, K.MAX_FEEDBACK, 0.0, 1.0, 1.0), K.params(lines, 0.3, 0.2, 1.0, 0.0)
    first = {0: [(0, soft, 0), (1, loud, 0)], 1: [(0, None, 300)]}
    b = make(na, nano, 256)
    y0 = hook_run(b, first, x[:, :600], calls[:2])
    assert b.GetStreamRoom(0) is None and b.StreamRoomFadeRemaining(0) == 100 and b.GetRoomInfo()["numRooms"] == 2
    b.RemoveStreams(1, 1)
    assert b.GetRoomInfo()["numRooms"] == 1 and b.AddStreams(nano[1], 1, doPrewarm=False) == 1 and b.GetStreamRoom(1) is None
    y1 = hook_run(b, {0: [(1, soft, 0)]}, x[:, 600:1000], calls[2:4])
    assert b.GetRoomInfo()["numRooms"] == 1 and b.StreamRoomFadeRemaining(0) == 0
    b.SetStreamRoom(1, None, 0)
    before = launches()
    y2 = hook_run(b, {}, x[:, 1000:], calls[4:])
    assert launches() == before and b.GetRoomInfo()["numRooms"] == 0
    b.close()
    e = K.run_cuts(first, x[:, :1000], calls[:4])[0]
    e[1, 600:] = K.run_cuts({0: [(1, soft, 0)]}, x[:, 600:1000], calls[2:4])[0][1]
    assert_same(np.concatenate([y0, y1, y2], axis=1), np.concatenate([e, x[:, 1000:]], axis=1))
    assert np.array_equal(bits(y1[0, 100:]), bits(x[0, 700:1000])) and np.max(np.abs(y1[1])) < 100.0, "nothing of the loud line leaks"


def batch_run(na, nano, x, calls, ops, path="process", max_line=256):
    """ROWS nano streams through "process" (host rows), "strided" (device rows an odd stride apart), "in-place" (device rows, output over input) or "plain" (host rows, no stage)"""
    import torch
    dev = torch.device("cuda", 0)
    b = make(na, nano, 0 if path == "plain" else max_line)
    out, pos = [], 0
    for c, n in enumerate(calls):
        for row, p, fade in ops.get(c, ()):
            b.SetStreamRoom(row, p, fade)
        block = np.ascontiguousarray(x[:, pos:pos + n])
        pos += n
        if path in ("process", "plain"):
            out.append(b.Process(block))
            continue
        stride = n + 3 if path == "strided" else n
        dx = torch.from_numpy(block).to(dev)
        dy = dx if path == "in-place" else torch.full((ROWS, stride), 7.0, device=dev)
        torch.cuda.synchronize(dev)
        b.ProcessDevice(dx.data_ptr(), dy.data_ptr(), n, n, stride)
        b.Synchronize()
        rows = dy.cpu().numpy()
        assert np.all(rows[:, n:] == F(7.0)), "the stage wrote past the end of a row"
        out.append(rows[:, :n].copy())
    b.close()
    return np.concatenate(out, axis=1)


@pytest.mark.parametrize("cut", [1000] + K.CUTS)
def test_the_cut_into_calls_never_shows(na, nano, cut):
    """One call and calls of 1, 127, 128, 129 and 333 samples, from host rows, from device rows an odd stride apart and in place: equal
    to the restatement applied to the rows the same batch produces with the stage idle.  Idle, the stage launches nothing and the rows
    are those of a batch without it; the bits do not depend on maxLineSamples (rings of 512 and of 32768 floats)."""
    calls = K.cuts_of(1000, [cut])
    x = np.stack([H.noise(1000, 700 + r) for r in range(ROWS)])
    lines = K.EDGES["at-max"][1]
    ops = {0: [(0, K.params([128] * 8, 0.3, 0.25), 0), (1, K.params(lines, K.MAX_FEEDBACK, 0.5, 1.0, 0.5), 0), (2, K.params(lines[::-1], 0.2, 0.0, 0.7, 0.7), 500),
               (3, K.params(lines, 0.35, 0.4, 1.0, 0.0), 0)]}
    before = launches()
    idle = batch_run(na, nano, x, calls, {})
    assert launches() == before, "enabled without an entry: nothing of the stage is launched"
    e = K.run_cuts(ops, idle, calls)[0]
    for path in ("process", "strided", "in-place"):
        before = launches()
        assert_same(batch_run(na, nano, x, calls, ops, path), e, (cut, path))
        assert launches() - before == len(calls)
    assert np.array_equal(bits(e[4:]), bits(idle[4:])) and not np.array_equal(e[0], idle[0]) and np.any(idle[0])
    if cut == 333:
        assert np.array_equal(bits(idle), bits(batch_run(na, nano, x, calls, {}, "plain")))
        assert_same(batch_run(na, nano, x, calls, ops, max_line=16384), e, ("maxLineSamples 16384",))


def test_rules(na, nano):
    """Every call says "room stage not enabled" before the enable call; each refusal names its field; Get returns the target from the
    set call on and a set call during a fade is refused with the samples left; a larger maximum is refused while a stream has a room."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    b = make(na, nano, 0)
    p = K.params(K.EDGES["primes"][1], 0.3, 0.2)
    for call in (lambda: b.SetStreamRoom(0, p), lambda: b.SetStreamRoom(0, None), lambda: b.GetStreamRoom(0), lambda: b.StreamRoomFadeRemaining(0),
                 lambda: b.GetRoomInfo(), lambda: b.DebugRunRoomStage(np.zeros((ROWS, 8), F))):
        with pytest.raises(na.NeuralAudioError, match=r"room stage not enabled \(NA_BatchEnableRoomStage\)"):
            call()
    assert lib.NA_BatchGetStreamRoom(b._h, 0, None) < 0 and lib.NA_BatchStreamRoomFadeRemaining(b._h, 0) < 0
    for bad in (128, 255, 768, 32768, -1):
        with pytest.raises(na.NeuralAudioError, match=r"EnableRoomStage: maxLineSamples must be a power of two in \[256, 16384\]"):
            b.EnableRoomStage(bad)
    b.EnableRoomStage(1024)
    b.EnableRoomStage(256)  # idempotent for an equal or smaller maximum
    assert b.GetRoomInfo()["maxLineSamples"] == 1024 and b.GetRoomInfo()["ringSamples"] == 2048
    nan, above = float("nan"), float(np.nextafter(F(K.MAX_FEEDBACK), F(1.0)))
    one = lambda field, i, v: dict(p, **{field: [v if k == i else old for k, old in enumerate(p[field])]})
    for change, text in ((one("lineSamples", 0, 127), r"lineSamples\[0\] must lie in \[128, maxLineSamples\] \(maxLineSamples = 1024\)"), (one("lineSamples", 7, 1025), r"lineSamples\[7\] must lie in"),
                         (one("feedback", 3, above), r"feedback\[3\] must lie in \[0, 1 / sqrt 8\]"), (one("feedback", 5, -1e-9), r"feedback\[5\] must lie in"), (one("feedback", 0, nan), r"feedback\[0\] must lie in"),
                         (dict(p, damp=0.51), r"damp must lie in \[0, 0.5\]"), (dict(p, damp=nan), r"damp must lie in \[0, 0.5\]"), (dict(p, damp=-0.1), r"damp must lie in \[0, 0.5\]"),
                         (dict(p, wet=float("inf")), "wet must be finite and at most 1e6 in magnitude"), (dict(p, dry=nan), "dry must be finite and at most 1e6 in magnitude")):
        with pytest.raises(na.NeuralAudioError, match="SetStreamRoom: " + text):
            b.SetStreamRoom(0, change)
    with pytest.raises(na.NeuralAudioError, match=r"SetStreamRoom: fadeSamples must lie in \[0, 1 << 20\]"):
        b.SetStreamRoom(0, p, (1 << 20) + 1)
    at_bound = one("feedback", 1, K.MAX_FEEDBACK)
    b.SetStreamRoom(2, at_bound, 1 << 20)
    assert b.StreamRoomFadeRemaining(2) == 1 << 20 and b.GetStreamRoom(2) == at_bound and b.GetRoomInfo()["numRooms"] == 1
    with pytest.raises(na.NeuralAudioError, match=r"SetStreamRoom: a room fade of stream 2 is running \(1048576 samples left\)"):
        b.SetStreamRoom(2, None, 10)
    with pytest.raises(na.NeuralAudioError, match="a larger maxLineSamples is refused while a stream has a room"):
        b.EnableRoomStage(2048)
    b.RemoveStreams(2, 1)
    b.EnableRoomStage(2048)
    assert b.GetRoomInfo()["ringSamples"] == 4096 and b.GetRoomInfo()["numRooms"] == 0
    b.close()
