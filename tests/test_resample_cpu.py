"""Host arithmetic of batch resampling (include/neuralaudio_amd.h "batch resampling", csrc/resample.cpp); no device.

The expectations are this file's own restatement of the contract: Fc = lcm(Fe, Fm), te = Fc / Fe, tm = Fc / Fm, K = 48 * max(te, tm)
+ 1, J(E) = floor((E - 1) * te / tm) + 1, P(E) = floor(J(E) / q) * q, S = (q - 1) * tm + pad, latency = (48 * max(te, tm) + S) / te."""
import math

import numpy as np
import pytest

import neuralaudio_amd as na

PAIRS = [(44100, 48000), (88200, 48000), (48000, 44100), (32000, 48000), (22050, 48000)]
T = 48


def _terms(fe, fm):
    g = math.gcd(fe, fm)
    return fm // g, fe // g  # te, tm


def _shift(te, tm, q):
    base = T * max(te, tm) + (q - 1) * tm
    pad = (-base) % te
    return (q - 1) * tm + pad, (base + pad) // te


def _J(E, te, tm):
    return 0 if E <= 0 else ((E - 1) * te) // tm + 1


@pytest.mark.parametrize("fe,fm", PAIRS)
@pytest.mark.parametrize("q", [1, 32, 64, 128])
def test_the_plan_of_a_rate_pair_equals_the_formulas(fe, fm, q):
    te, tm = _terms(fe, fm)
    p = na.resample_plan(fe, fm, q)
    K = T * max(te, tm) + 1
    S, latency = _shift(te, tm, q)
    assert S - (q - 1) * tm < te
    assert (p["external_rate"], p["model_rate"], p["te"], p["tm"], p["quantum"]) == (fe, fm, te, tm, q)
    assert p["prototype_length"] == K
    assert p["taps_up"] == (K - 1) // te + 1 and p["taps_down"] == (K - 1) // tm + 1
    assert p["latency_samples"] == latency


def test_the_latencies_at_44100_hz_and_the_default_quantum():
    assert [na.resample_plan(44100, 48000, q)["latency_samples"] for q in (1, 32, 128)] == [48, 77, 165]
    p = na.resample_plan(44100, 48000)
    assert (p["te"], p["tm"], p["taps_up"], p["taps_down"], p["prototype_length"]) == (160, 147, 49, 53, 7681)
    assert na.resample_plan(44100, 48000, 0) == na.resample_plan(44100, 48000, p["quantum"])
    assert p["quantum"] in (1, 32)  # (the default: whichever the step measurement in DESIGN.md 2.8 decided)


def test_equal_rates_mean_no_resampling():
    p = na.resample_plan(48000, 48000)
    assert p["latency_samples"] == 0 and p["te"] == 1 and p["tm"] == 1
    assert na.resample_model_frames(48000, 48000, 0, 12345) == 12345


@pytest.mark.parametrize("args,words", [((0, 48000, 0), ["positive"]), ((44100, -1, 0), ["positive"]), ((44100, 48000, 3), ["quantum", "3"]),
                                        ((44101, 48000, 0), ["44101", "48000", "640"])])
def test_refusals_name_their_reason(args, words):
    with pytest.raises(na.NeuralAudioError) as e:
        na.resample_plan(*args)
    for w in words:
        assert w in str(e.value), str(e.value)
    if args[0] == 44101:  # the reduced ratio itself (44101 and 48000 are coprime)
        assert "44101 : 48000" in str(e.value)
        with pytest.raises(na.NeuralAudioError):
            na.resample_prototype(44101, 48000)
        with pytest.raises(na.NeuralAudioError):
            na.resample_model_frames(44101, 48000, 0, 10)


@pytest.mark.parametrize("fe,fm", PAIRS)
def test_the_prototype_is_symmetric_flat_in_the_pass_band_and_100_db_down_in_the_stop_band(fe, fm):
    te, tm = _terms(fe, fm)
    h = na.resample_prototype(fe, fm)
    assert h.dtype == np.float32 and h.size == T * max(te, tm) + 1
    assert np.array_equal(h, h[::-1])
    fc_rate = fe * te  # the common rate
    fmin = min(fe, fm)
    nfft = 1 << 21
    H = np.abs(np.fft.rfft(h.astype(np.float64), nfft))
    f = np.arange(H.size) * (fc_rate / nfft)
    pass_band = H[f <= (16000.0 / 22050.0) * fmin / 2]
    stop_band = H[f >= fmin / 2]
    dev = np.max(np.abs(20 * np.log10(pass_band)))
    stop = 20 * np.log10(np.max(stop_band))
    print("%d -> %d: pass-band deviation %.6f dB, stop band %.2f dB" % (fe, fm, dev, stop))
    assert dev <= 0.001
    assert stop <= -100.0
    # the worst-case gain of one phase (what the rounding bounds of the GPU tests are built from) is about 2
    gains = [np.sum(np.abs(te * h[p::te].astype(np.float64))) for p in range(te)]
    assert 1.0 < max(gains) < 3.0


@pytest.mark.parametrize("fe,fm", PAIRS)
@pytest.mark.parametrize("q", [1, 32, 128])
def test_model_frames_are_whole_blocks_and_causal_for_random_call_lengths(fe, fm, q):
    te, tm = _terms(fe, fm)
    S, _ = _shift(te, tm, q)
    rng = np.random.RandomState(fe % 1000 + q)
    E, P, total = 0, 0, 0
    for n in rng.randint(1, 300, size=3000):
        E += int(n)
        P1 = na.resample_model_frames(fe, fm, q, E)
        assert P1 == (_J(E, te, tm) // q) * q
        assert P1 >= P and (P1 - P) % q == 0
        total += P1 - P
        P = P1
        # every model frame the newest output sample reads has been run
        assert ((E - 1) * te - S) // tm <= P - 1
    assert total == na.resample_model_frames(fe, fm, q, E)


def test_128_sample_calls_at_44100_hz_give_the_model_whole_chain_blocks():
    seq = lambda q: [na.resample_model_frames(44100, 48000, q, 128 * (i + 1)) - na.resample_model_frames(44100, 48000, q, 128 * i) for i in range(12)]
    assert set(seq(32)) == {128, 160} and seq(32)[:3] == [128, 128, 160]
    assert set(seq(1)) == {139, 140}
