"""The drive stage's contract (include/neuralaudio_amd.h, csrc/drive_stage.h) restated in plain numpy, in a given dtype, and the cases the
CPU and GPU tests share.  Helper code only."""
import json

import numpy as np

import na_oracle as O

T = 32
TANH, CUBIC, HARD = 0, 1, 2
N = 408  # 3 x 128 + 24
BOUND = 2e-6  # RMS of every 32-frame window, relative to max(1, level)
# (shape, oversample, drive, bias, mix, level): shape x L, and one case with a bias and a half mix
CASES = [(s, L, 8.0, 0.0, 1.0, 1.0) for s in (TANH, CUBIC, HARD) for L in (2, 4, 8)] + [(TANH, 4, 8.0, 0.3, 0.5, 1.5)]


def params(case):
    return dict(zip(("shape", "oversample", "drive", "bias", "mix", "level"), case))


def signal(n=N, seed=5):
    """O.signal_noise at amplitude 1"""
    return (4.0 * O.signal_noise(n, seed).astype(np.float64)).clip(-1.0, 1.0).astype(np.float32)


def prototype(L):
    c = np.arange(L * T + 1) - L * T / 2
    h = np.sinc(c / L) * np.i0(9.0 * np.sqrt(np.maximum(0.0, 1.0 - (2.0 * c / (L * T)) ** 2))) / np.i0(9.0)
    return h / h.sum()


def shape(kind, v):
    if kind == TANH:
        return 1 - 2 / (np.exp2(v * v.dtype.type(2.885390081777927)) + 1)
    if kind == CUBIC:
        return np.where(np.abs(v) < 1, v.dtype.type(1.5) * (v - v * v * v / 3), np.sign(v))
    return np.clip(v, -1, 1)


def ramp(frm, to, R, n, dt):
    k = np.arange(n)
    w = np.where(k >= R - 1, 1.0, (k + 1) / max(R, 1)).astype(np.float32).astype(dt)
    return dt(frm) + (dt(to) - dt(frm)) * w


def restate(x, p, R=0, dtype=np.float64):
    """the row a NEW entry set in front of x[0] with rampSamples = R hands to the model"""
    dt, L, n = dtype, p["oversample"], len(x)
    x = np.nan_to_num(np.asarray(x, np.float32), nan=0.0).astype(dt)
    h = prototype(L).astype(np.float32).astype(dt)
    z = np.zeros(L * n, dt)
    z[::L] = x
    u = np.convolve(z, dt(L) * h)[:L * n]
    g, b = (np.repeat(ramp(p[k], p[k], R, n, dt), L) for k in ("drive", "bias"))
    s = shape(p["shape"], g * u + b) - shape(p["shape"], b)
    w = np.convolve(s, h)[:L * n:L]
    mix, level = ramp(0.0 if R else p["mix"], p["mix"], R, n, dt), ramp(1.0 if R else p["level"], p["level"], R, n, dt)
    return (level * (mix * w + (1 - mix) * np.concatenate([np.zeros(T, dt), x])[:n])).astype(dt)


def worst_window(y, ref, level=1.0):
    """the largest 32-frame window RMS of y - ref, as a fraction of BOUND * max(1, level)"""
    d = (np.asarray(y, np.float64) - np.asarray(ref, np.float64))[:len(ref) // 32 * 32].reshape(-1, 32)
    return float(np.sqrt((d * d).mean(axis=1)).max() / (BOUND * max(1.0, level)))


def passthrough_json():
    """a one-layer keras dense model with weight 1 and no bias: the row the model reads comes out as it is"""
    return json.dumps({"in_shape": [None, None, 1], "in_skip": 0, "samplerate": 48000.0,
                       "layers": [{"type": "dense", "activation": "", "shape": [None, None, 1], "weights": [[[1.0]], [0.0]]}]})
