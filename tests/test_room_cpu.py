"""CPU-side tests of the room stage: NA_RoomParamsFromSeconds's arithmetic, the struct layouts, and the numpy restatement
of the contract (tests/room_cases.py) on its own -- the cut into calls does not show in its bits, and the loop is stable at the bounds
of a setting.  Everything that runs on the device is in tests/test_gpu_room.py."""
import ctypes as C
import math

import numpy as np
import pytest

import room_cases as K
from mod_cases import signal

F = np.float32
INF = float("inf")


@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    return neuralaudio_amd


@pytest.mark.parametrize("rate,size_ms,decay,damp,wet_db,dry_db", [(48000, 40.0, 1.5, 0.2, -12.0, 0.0), (44100, 11.0, 0.4, 0.0, 0.0, -INF), (96000, 180.0, 6.0, 0.5, -INF, -3.0),
                                                                   (48000, 1.0, 0.05, 0.1, 20.0, 0.0)])
def test_room_params_from_seconds_matches_double_arithmetic(na, rate, size_ms, decay, damp, wet_db, dry_db):
    """Every field equals the double formula rounded once; a line is the smallest prime not below its target unless clamped (1 ms:
    every line 128; 180 ms at 96 kHz: line 0 at 16384, which is no prime); every result is a setting SetStreamRoom takes."""
    got = na.room_params_from_seconds(rate, size_ms, decay, damp, wet_db, dry_db)
    assert got == K.from_seconds(rate, size_ms, decay, damp, wet_db, dry_db)
    for i, n in enumerate(got["lineSamples"]):
        want = rate * size_ms / 1000.0 * 2.0 ** (-i / 8.0)
        assert n in (K.MIN_LINE, K.MAX_LINE) or (n >= want and K.prime_from(math.ceil(want)) == n)
        assert 0.0 < got["feedback"][i] <= K.MAX_FEEDBACK
    assert got["lineSamples"][0] == {40.0: 1931, 11.0: 487, 180.0: 16384, 1.0: 128}[size_ms] and got["lineSamples"][7] >= K.MIN_LINE
    if size_ms == 40.0:
        assert got["feedback"][0] == float(F(10.0 ** (-3.0 * 1931 / (1.5 * 48000)) / math.sqrt(8.0)))


def test_the_structs_are_the_headers(na):
    """NA_RoomParams is nineteen words, NA_RoomInfo four ints and a long long; the feedback bound is fl(1 / sqrt 8), below 1 / sqrt 8;
    without a device the batch calls fail loudly; NA_RoomParamsFromSeconds refuses by name."""
    from neuralaudio_amd import capi
    P, I = capi.NA_RoomParams, capi.NA_RoomInfo
    assert [name for name, _ in P._fields_] == ["lineSamples", "feedback", "damp", "wet", "dry"]
    assert (C.sizeof(P), P.lineSamples.offset, P.feedback.offset, P.damp.offset, P.wet.offset, P.dry.offset) == (76, 0, 32, 64, 68, 72)
    assert [name for name, _ in I._fields_] == ["maxLineSamples", "ringSamples", "pieceSamples", "numRooms", "deviceBytes"]
    assert (C.sizeof(I), I.deviceBytes.offset) == (24, 16)
    assert (capi.NA_ROOM_LINES, capi.NA_ROOM_MIN_LINE_SAMPLES, capi.NA_ROOM_MAX_LINE_SAMPLES) == (K.LINES, K.MIN_LINE, K.MAX_LINE)
    assert K.MAX_FEEDBACK == float(F(0.35355338)) and K.MAX_FEEDBACK < 1.0 / math.sqrt(8.0)
    assert capi.load_library().NA_BatchEnableRoomStage(None, 256) != 0 and "no HIP device" in capi.last_error()
    for change, text in ((dict(sample_rate=0), "sampleRate must be >= 1"), (dict(size_ms=float("nan")), "sizeMs must be finite and at least 0"), (dict(decay_seconds=0.0), "decaySeconds must be finite and above 0"),
                         (dict(damp=0.51), r"damp must lie in \[0, 0.5\]"), (dict(wet_db=121.0), "wet must be finite and at most 1e6 in magnitude"), (dict(dry_db=INF), "dry must be finite and at most 1e6 in magnitude")):
        with pytest.raises(na.NeuralAudioError, match="NA_RoomParamsFromSeconds: " + text):
            na.room_params_from_seconds(**dict(dict(sample_rate=48000, size_ms=40.0, decay_seconds=1.5, damp=0.2, wet_db=-12.0, dry_db=0.0), **change))


@pytest.mark.parametrize("edge", sorted(K.EDGES))
def test_the_restatement_does_not_show_the_cut(edge):
    """Calls of 1, 127, 128, 129 and 333 samples in turn against three calls, with a set call that changes lengths, feedback, damp and
    wet fading across many calls and a removal behind it: the same bits, NaN, infinities and subnormals of the input included."""
    lines, total = K.EDGES[edge][1], 2600
    x = np.stack([signal(40 + r, total) for r in range(2)])
    a, b = K.params(lines, 0.3, 0.25, 0.5, 0.75), K.params(lines[::-1], K.MAX_FEEDBACK, 0.5, 1.0, 0.5)
    calls = K.cuts_of(total, K.CUTS)
    at = [0, len(calls) // 3, 2 * len(calls) // 3]
    starts = [sum(calls[:c]) for c in at] + [total]
    sets = [[(0, a, 0), (1, a, 300)], [(0, b, 700)], [(1, None, 200)]]
    y, refs = K.run_cuts(dict(zip(at, sets)), x, calls)
    y3, _ = K.run_cuts(dict(enumerate(sets)), x, list(np.diff(starts)))
    assert np.array_equal(y.view(np.uint32), y3.view(np.uint32))
    assert refs[0].B == b and not refs[1].has and not np.array_equal(y[0], x[0])


@pytest.mark.parametrize("damp", [0.0, 0.5])
def test_the_loop_is_stable_at_the_bounds(damp):
    """feedback = fl(1 / sqrt 8), damp 0 and 0.5: the energy the loop holds (RoomRef.energy) does not grow over 20 circulations of the longest line.
    The bound is rounding alone: a line's sample comes from seven rounded operations, at most 16 * 2^-24 on its square, once per pass of >= 128 samples."""
    lines = K.EDGES["at-max"][1]
    ref = K.RoomRef()
    ref.set(K.params(lines, K.MAX_FEEDBACK, damp, 1.0, 0.0), 0)
    ref.run(signal(50, 600)[64:])
    start = ref.energy()
    ref.run(np.zeros(20 * max(lines), F))
    print("energy after / before: %.9f" % (ref.energy() / start))
    assert 0.0 < ref.energy() <= start * (1.0 + 20 * max(lines) / K.MIN_LINE * 16 * 2.0 ** -24)
