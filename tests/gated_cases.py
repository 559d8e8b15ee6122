"""Gated WaveNet layer arrays (the A1-format key "gated") -- TEST INFRASTRUCTURE ONLY: a plain numpy restatement of the contract, the
case list of tests/test_gated_cpu.py / tests/test_gpu_gated.py and the .nam writer.  Every model is synthetic (no trained gated capture
was available).  Per layer (C channels; conv [2C][C][K], conv bias [2C], mix-in [2C], 1x1 [C][C], 1x1 bias [C]; rows 0 .. C-1 filter,
C .. 2C-1 gate; a plain array has C rows and no sigmoid):
    a, g = bconv + wmix c + sum_k Wconv[:, :, k] x[t - d (K-1-k)];  z = act(a) sigmoid(g);  head += z;  x_next = x + W1 z + b1
sigmoid: FastMath 0.5 (FastTanh(0.5 g) + 1), StdMath 1 / (1 + exp(-g))."""
import json

import numpy as np

import na_oracle as O
from wide_cases import chain

SAMPLES = 408  # 3 x 128 + 24 = 1 + 11 x 37
TOL_RMS, WINDOW = 2e-6, 32  # test_gpu_frame.py's rule: every 32-frame window, relative to max(1, level)


def _fast_tanh(x):
    """Activation.h:83-91 in x's own precision"""
    ax, x2, t = np.abs(x), x * x, x.dtype.type
    num = x * (t(2.45550750702956) + t(2.45550750702956) * ax + (t(0.893229853513558) + t(0.821226666969744) * ax) * x2)
    return num / (t(2.44506634652299) + (t(2.44506634652299) + x2) * np.abs(x + t(0.814642734961073) * x * ax))


def unpack(arrays, w):
    """views into the flat weights, in file order: ([(rechannel, [(conv, conv bias, mix-in, 1x1, 1x1 bias) per layer], head, head bias)], scale)"""
    pos, out = 0, []

    def take(*shape):
        nonlocal pos
        pos += int(np.prod(shape))
        return w[pos - int(np.prod(shape)):pos].reshape(shape)

    for a in arrays:
        c, rows = a["channels"], a["channels"] * (2 if a["gated"] else 1)
        out.append((take(c, a["input_size"]), [(take(rows, c, k), take(rows), take(rows), take(c, c), take(c)) for k in a["kernel_sizes"]],
                    take(a["head_size"], c), take(a["head_size"]) if a["has_head_bias"] else None))
    scale = take(1)
    assert pos == w.size, (pos, w.size)
    return out, scale


def forward(arrays, weights, x, dtype=np.float64, std=False):
    """The whole signal at once in `dtype`, from the state of a prewarmed stream: every layer's history holds its zero-input steady-state
    column, which a first pass computes (one frame of silence in which every tap reads the layer's own input)."""
    w = np.asarray(weights, dtype=np.float32).astype(dtype)
    t = w.dtype.type
    cols = None
    for cond in (np.zeros(1, dtype), np.asarray(x, dtype=np.float32).astype(dtype)):
        T, seen, xin, head = cond.size, [], cond[None, :], 0
        tensors, scale = unpack(arrays, w)
        for a, (rech, layers, wh, bh) in zip(arrays, tensors):
            c, xc = a["channels"], rech @ xin
            for (wc, bc, wm, w1, b1), d in zip(layers, a["dilations"]):
                seen.append(xc[:, 0].copy())
                acc = bc[:, None] + wm[:, None] * cond[None, :]
                for j in range(wc.shape[2]):  # taps in ascending order
                    shift = min(d * (wc.shape[2] - 1 - j), T)
                    acc = acc + wc[:, :, j] @ (xc if cols is None else np.concatenate([np.repeat(cols[len(seen) - 1][:, None], shift, axis=1), xc[:, :T - shift]], axis=1))
                fa = acc[:c]
                z = np.where(fa > 0, fa, t(0.01) * fa) if a["activation"] == O.ACT_LEAKYRELU else (np.tanh(fa) if std else _fast_tanh(fa))
                if a["gated"]:
                    z = z * (t(1) / (t(1) + np.exp(-acc[c:])) if std else t(0.5) * (_fast_tanh(acc[c:] * t(0.5)) + t(1)))
                head = head + z
                xc = xc + w1 @ z + b1[:, None]
            xin, head = xc, wh @ head + (0 if bh is None else bh[:, None])
        cols = seen
    return scale[0] * head[0]


def weights(case):
    """seeded U(-a, a), a = 1 / sqrt(fan-in) per tensor; the last weight (head scale) 1: outputs at the level the parity bound is stated for"""
    rng = np.random.default_rng(case["seed"])
    w = np.zeros(sum(a["channels"] * a["input_size"] + a["head_size"] * (a["channels"] + a["has_head_bias"]) + sum(
        (a["channels"] * k + 2) * a["channels"] * (1 + a["gated"]) + a["channels"] * (a["channels"] + 1) for k in a["kernel_sizes"]) for a in case["arrays"]) + 1, np.float32)
    tensors, scale = unpack(case["arrays"], w)
    for rech, layers, wh, bh in tensors:
        for v, fan_in in [(rech, rech.shape[1]), (wh, wh.shape[1])] + ([(bh, wh.shape[1])] if bh is not None else []) + [
                (v, f) for wc, bc, wm, w1, b1 in layers for v, f in ((wc, wc[0].size), (bc, wc[0].size), (wm, 1), (w1, w1.shape[1]), (b1, w1.shape[1]))]:
            v[...] = rng.uniform(-1.0, 1.0, size=v.shape) / np.sqrt(fan_in)
    scale[0] = 1.0
    return w


def nam_json(arrays, w):
    """A1-format .nam document (one kernel size per array, 1x1 heads), with the trainer's "gated" key"""
    layers = [{"input_size": a["input_size"], "condition_size": 1, "head_size": a["head_size"], "channels": a["channels"],
               "kernel_size": a["kernel_sizes"][0], "dilations": list(a["dilations"]), "activation": "LeakyReLU" if a["activation"] == O.ACT_LEAKYRELU else "Tanh",
               "gated": bool(a["gated"]), "head_bias": bool(a["has_head_bias"])} for a in arrays]
    return json.dumps({"version": "0.5.4", "architecture": "WaveNet", "metadata": {"loudness": -10.0},
                       "config": {"layers": layers, "head": None, "head_scale": float(w[-1])}, "weights": [float(v) for v in w], "sample_rate": 48000})


def case(name, channels, ksize, dilations, seed, gated=None, act=O.ACT_TANH, std=False):
    arrays = chain(channels, [([ksize] * len(dilations), dilations)] * len(channels), act)
    for i, a in enumerate(arrays):
        a["gated"] = True if gated is None else gated[i]
    return dict(name=name, arrays=arrays, seed=seed, std=std)


LONG = [1, 2, 64, 200]  # LDS taps, ring taps, a tap beyond a 128-frame block
MAX_K16 = 35  # largest gated kernel size at 13 .. 16 channels (frame_lds.h FrameMaxKernelSize(4, true): 162 432 of 163 840 bytes)
CASES = [case("c16-8", [16, 8], 3, LONG, 1), case("c4", [4], 3, LONG, 2), case("c6", [6], 3, LONG, 3), case("c12", [12], 3, LONG, 4),
         case("gated-plain", [8, 4], 3, [1, 64], 5, gated=[True, False]), case("plain-gated", [8, 4], 3, [1, 64], 6, gated=[False, True]),
         case("k1", [5], 1, [1, 1], 7), case("k2", [16], 2, [1, 70], 8), case("k5-d70", [12], 5, [70, 1], 9),
         case("leaky", [8], 3, [1, 64], 10, act=O.ACT_LEAKYRELU), case("stdmath", [8, 4], 3, [1, 64], 11, std=True)]


def worst_window(y, ref):
    """worst 32-frame window error relative to max(1, level), as a fraction of TOL_RMS"""
    return max(O.rms(y[a:a + WINDOW] - ref[a:a + WINDOW]) / max(1.0, O.rms(ref[a:a + WINDOW])) for a in range(0, y.size, WINDOW)) / TOL_RMS
