"""Model shapes of the tests of the keras-stack tails (recurrent_tail.h DenseTail / ConvTail, the tail branch at the end of
lstm_kernels.hip RecurrentWaveRtKernel, the DenseTail calls of LstmGenericKernel / GruGenericKernel) -- TEST INFRASTRUCTURE ONLY.

Shared by tests/test_gpu_tails.py (which runs them) and tests/test_host_cpu.py (which proves without a GPU that every case loads or is
refused by name, that it runs where it is listed, that its output depends on its input, that float32 arithmetic alone stays far below
the GPU bound and that a wrong tap, a wrong dilation or a missing softmax in the checker would be noticed).

Weights: ref_np.synth_keras_stack draws kernels and biases of the same size, so that the bias decides most of the output (the five
stacks of the older tests: rms(out - out for a zero input) 1e-4 .. 1e-2 of an rms(out) of 0.07 .. 0.5).  Here every dense, conv1d and
recurrent INPUT kernel is scaled by the case's `gain` and every dense / conv1d bias by `bias_scale`, then rounded to 7 decimals as the
generator does: the signal path dominates, and one stale history row or one wrong tap moves the output by far more than the bound.
The gain is per case: a case that misses the conditions of tests/test_host_cpu.py gets another gain, never an exemption (gains and
seeds were settled on the CPU against those conditions alone, before any case ran on a GPU).

Sizes that depend on what the loader admits are read from the library's own shape predicate (NA_DebugRecurrentShapePlan through
recurrent_cases.shape_plan), not typed in."""
import functools
import json

import numpy as np

import na_oracle as O
import recurrent_cases as RC
import ref_np as R

GAIN, BIAS_SCALE = 6.0, 0.2
MAX_FRAMES = 128           # LSTM_MAX_FRAMES: a longer call is cut into launches of this many samples
FIXED_CALLS = [129, 300, 63, 64, 65, 127, 128]  # behind the leading 1, 1, 2, 3 of every partition
LEVELS = RC.LEVELS


def recurrent(spec):
    return [l for l in spec if l[0] in ("lstm", "gru")]


def lowered(spec):
    """The tail as the loader lowers it (model_loader.cpp AppendKerasTailLayer): [in, out, taps, dilation, linear] per dense / conv1d layer.
    tests/test_host_cpu.py holds this against the plan of the loaded model."""
    rec = recurrent(spec)
    cur = rec[-1][1] if rec else 1
    tail = []
    for l in spec[len(rec):]:
        kind = l[0]
        if kind in ("dense", "conv1d"):
            taps, dil = (l[2], l[3]) if kind == "conv1d" else (1, 1)
            act = (l[4] if len(l) > 4 else "") if kind == "conv1d" else (l[2] if len(l) > 2 else "")
            tail.append([cur, l[1], taps, dil, act in ("", "linear")])
            cur = l[1]
        elif kind == "activation":
            if tail and tail[-1][4]:
                tail[-1][4] = l[2] in ("", "linear")
            else:
                tail.append([cur, cur, 1, 1, False])
        elif kind == "batchnorm":
            if not (tail and tail[-1][4]):
                tail.append([cur, cur, 1, 1, True])
        elif kind == "prelu":  # relu(x) - alpha relu(-x): twice the width in between
            if tail and tail[-1][4]:
                p = tail.pop()
                tail.append([p[0], 2 * cur, p[2], p[3], False])
            else:
                tail.append([cur, 2 * cur, 1, 1, False])
            tail.append([2 * cur, cur, 1, 1, True])
        else:
            raise ValueError(kind)
    return tail


def history(spec):
    """(taps - 1) x dilation of the longest conv1d layer: 0 for a dense tail."""
    return max((t[2] - 1) * t[3] for t in lowered(spec))


def dims(spec):
    """(kind, hidden, recurrent layers, tail layers, tail width, tail history) as the loader hands them to RecurrentKernelFor; a stack
    without a recurrent layer is an "lstm" of no layers and one unit."""
    rec, tail, hist = recurrent(spec), lowered(spec), history(spec)
    width = max((max(t[0], t[1]) if hist > 0 else t[1]) for t in tail)
    return (rec[0][0] if rec else "lstm"), (rec[0][1] if rec else 1), len(rec), len(tail), width, hist


def plan(spec):
    return RC.shape_plan(*dims(spec))


@functools.lru_cache(maxsize=None)
def max_history():
    """LSTM_MAX_TAIL_HISTORY as the shape predicate sees it: the longest conv1d history it admits behind a one-unit input."""
    return max(h for h in range(1, 2049) if RC.shape_plan("lstm", 1, 0, 1, 1, h)["admitted"])


def _conv_probe(kind, hidden, taps, dil):
    return [(kind, hidden), ("conv1d", 4, taps, dil, "tanh"), ("dense", 1)]


@functools.lru_cache(maxsize=None)
def widest_conv_input(kind, taps=2, dil=1):
    """The widest one-layer recurrent model in front of conv1d(4, taps, dil) + dense 1 that RecurrentWaveShape admits (its two
    [widest layer][history + 128] scratch arrays must fit the LDS beside the [samples][H] buffer)."""
    return max(h for h in range(1, RC.MAX_HIDDEN + 1) if plan(_conv_probe(kind, h, taps, dil))["admitted"])


def scaled_stack(spec, seed, gain=GAIN, bias_scale=BIAS_SCALE):
    """synth_keras_stack with a signal path: input kernels x gain, dense / conv1d biases x bias_scale, rounded as the generator rounds."""
    mj = R.synth_keras_stack(spec, seed)
    for l in mj["layers"]:
        if l["type"] in ("dense", "conv1d", "lstm", "gru"):
            l["weights"][0] = (np.array(l["weights"][0]) * gain).round(7).tolist()
        if l["type"] in ("dense", "conv1d"):
            l["weights"][1] = (np.array(l["weights"][1]) * bias_scale).round(7).tolist()
    return mj


def call_sizes(samples, hist, seed):
    """A partition of `samples`: 1, 1, 2, 3 first; then, in a seeded order, 129 and 300 (launches chunk at LSTM_MAX_FRAMES), 63 .. 128 and --
    where they are at most 300 -- the case's hist - 1, hist, hist + 1; the rest is drawn from the same sizes."""
    rng = np.random.default_rng(seed)
    due = FIXED_CALLS + [h for h in (hist - 1, hist, hist + 1) if 1 <= h <= 300 and hist > 0]
    assert samples >= 7 + sum(due), (samples, due)
    sizes, left = [1, 1, 2, 3] + [int(v) for v in rng.permutation(due)], samples - 7 - sum(due)
    while left > 0:
        c = min(int(rng.choice(RC.CALL_SIZES[:-1])), left)
        sizes.append(c)
        left -= c
    return sizes


def _case(name, form, spec, why, runs, seed, gain=GAIN, bias_scale=BIAS_SCALE, prewarm=False, refused=None):
    hist = history(spec)
    due = 7 + sum(FIXED_CALLS) + sum(h for h in (hist - 1, hist, hist + 1) if 1 <= h <= 300 and hist > 0)
    return dict(name=name, form=form, spec=spec, why=why, runs=runs, seed=seed, gain=gain, bias_scale=bias_scale, prewarm=prewarm, refused=refused,
                hist=hist, samples=max(3 * hist + 300, due))


def case_id(c):
    return c["name"]


@functools.lru_cache(maxsize=None)
def cases():
    """Every case that must load.  `runs`: what the case is listed for -- kernel by default, and of the runtime-shaped kernel's plan the
    fields named (waves: "one" | "many"; l2w).  form: "conv" (ConvTail) | "dense" (DenseTail)."""
    hm = max_history()
    wl, wg = widest_conv_input("lstm"), widest_conv_input("gru")
    wh = widest_conv_input("lstm", 3, hm // 2)  # the widest layer in front of a conv1d layer with the longest history
    rt = "RecurrentWaveRtKernel"
    out = [
        # ---- ConvTail
        _case("conv-raw-k12", "conv", [("conv1d", 4, 12, 1, "elu"), ("dense", 1)],
              "no recurrent layer: Hin == 0, the first conv1d layer has in = 1 and reads xin", dict(kernel=rt, waves="one", l2w=0), 11),
        _case("conv-dense-first", "conv", [("dense", 6, "tanh"), ("conv1d", 3, 3, 170, "tanh"), ("conv1d", 1, 1, 1)],
              "layer 0 has one tap: the region at tailHistRow[0] is empty and layer 1 owns the first history rows", dict(kernel=rt, waves="one", l2w=0), 12),
        _case("conv-hist-64-1-40", "conv", [("gru", 12), ("conv1d", 6, 2, 64, "tanh"), ("conv1d", 5, 2, 1, "elu"), ("conv1d", 4, 2, 40, "tanh"), ("dense", 1)],
              "histories large, small, large: layers with hist < tailHistMax sit at HM - hist", dict(kernel=rt, waves="one", l2w=0), 13, prewarm=True),
        _case("conv-hist-40-1-64", "conv", [("lstm", 10), ("conv1d", 5, 2, 40, "tanh"), ("conv1d", 6, 2, 1, "sigmoid"), ("conv1d", 4, 2, 64, "tanh"), ("dense", 1)],
              "the reverse order: the longest history belongs to the last conv1d layer", dict(kernel=rt, waves="one", l2w=0), 14, prewarm=True),
        _case("conv-hist-127", "conv", [("lstm", 8), ("conv1d", 4, 2, 127, "relu"), ("dense", 1)],
              "history one short of LSTM_MAX_FRAMES", dict(kernel=rt, waves="one", l2w=0), 15),
        _case("conv-hist-128", "conv", [("conv1d", 8, 5, 32, "elu"), ("dense", 1)],
              "history of LSTM_MAX_FRAMES: a full launch replaces every history row", dict(kernel=rt, waves="one", l2w=0), 16),
        _case("conv-hist-129", "conv", [("gru", 8), ("conv1d", 4, 4, 43, "tanh"), ("dense", 1)],
              "history one beyond LSTM_MAX_FRAMES: no launch replaces every history row", dict(kernel=rt, waves="one", l2w=0), 17),
        _case("conv-hist-limit", "conv", [("lstm", wh), ("conv1d", 4, 3, hm // 2, "tanh"), ("dense", 1)],
              "hist = LSTM_MAX_TAIL_HISTORY behind the widest layer the shape predicate admits with it", dict(kernel=rt), 18),
        _case("conv-widest-lstm", "conv", _conv_probe("lstm", wl, 2, 1),
              "the widest LSTM in front of a conv1d layer: several waves, only the first runs the tail", dict(kernel=rt, waves="many"), 19),
        _case("conv-widest-gru", "conv", _conv_probe("gru", wg, 2, 1),
              "the widest GRU in front of a conv1d layer: several waves, only the first runs the tail", dict(kernel=rt, waves="many"), 20),
        _case("conv-lstm40", "conv", [("lstm", 40), ("conv1d", 6, 3, 64, "tanh"), ("dense", 1)],
              "four waves with the gate weights in LDS in front of a conv1d layer", dict(kernel=rt, waves="many", l2w=0), 21, prewarm=True),
        _case("conv-one-wave-l2", "conv", [("lstm", 16), ("lstm", 16), ("lstm", 16), ("conv1d", 16, 3, 500, "tanh"), ("dense", 1)],
              "one wave whose LDS is filled by the conv1d scratch: gate weights streamed from L2", dict(kernel=rt, waves="one", l2w=1), 22),
        _case("conv-softmax-2", "conv", [("gru", 10), ("conv1d", 2, 2, 3, "softmax"), ("dense", 1)],
              "softmax (act == 5 inside ConvTail) over two units", dict(kernel=rt, waves="one", l2w=0), 123, prewarm=True),
        _case("conv-softmax-64", "conv", [("gru", 8), ("conv1d", 64, 3, 2, "softmax"), ("dense", 1)],
              "softmax inside ConvTail over 64 units, eight times the width of its input", dict(kernel=rt, waves="one", l2w=0), 24, gain=12.0),
        _case("conv-eight-layers", "conv",
              [("gru", 10), ("conv1d", 6, 3, 7), ("prelu", 6), ("dense", 5, "tanh"), ("batchnorm", 5), ("activation", 5, "elu"), ("conv1d", 4, 2, 20), ("batchnorm", 4),
               ("activation", 4, "sigmoid"), ("dense", 3), ("prelu", 3, "scalar"), ("dense", 1)],
              "LSTM_MAX_TAIL layers after lowering: prelu behind a linear conv1d and a linear dense layer, batchnorm folded and on its own, activation layers",
              dict(kernel=rt, waves="one", l2w=0, tail_layers=8), 25, prewarm=True),
        # ---- DenseTail
        _case("dense-lstm-63-64-softmax", "dense", [("lstm", 12), ("dense", 63, "tanh"), ("dense", 64, "sigmoid"), ("dense", 4, "softmax"), ("dense", 1)],
              "widths 63 and 64 behind an LSTM, softmax in the middle", dict(kernel=rt, waves="one", l2w=0), 31, gain=24.0, prewarm=True),
        # (width 1 is the last layer of every stack but one: a one-unit layer in the middle leaves rms(out - zero-input out) below 0.01 at any gain)
        _case("dense-gru-65-softmax", "dense", [("gru", 9), ("dense", 65, "elu"), ("dense", 5, "softmax"), ("dense", 1)],
              "width 65 behind a GRU, softmax in the middle", dict(kernel=rt, waves="one", l2w=0), 132, prewarm=True),
        _case("dense-lstm-256-softmax-last", "dense", [("lstm", 10), ("dense", 256, "relu"), ("dense", 3, "softmax")],
              "the widest dense layer (LSTM_MAX_TAIL_WIDTH), softmax at the end", dict(kernel=rt, waves="one", l2w=0), 33, gain=24.0),
        _case("dense-tail-only", "dense", [("dense", 8, "tanh"), ("dense", 16, "elu"), ("dense", 1)],
              "no recurrent layer: the first dense layer reads the scalar x0", dict(kernel=rt, waves="one", l2w=0), 34),
        _case("dense-lstm130-64", "dense", [("lstm", 130), ("dense", 64, "relu"), ("dense", 1)],
              "several waves write h and c while the first evaluates the dense tail", dict(kernel=rt, waves="many"), 35, prewarm=True),
        _case("dense-gru24-sigmoid", "dense", [("gru", 24), ("dense", 7, "sigmoid"), ("dense", 3), ("dense", 1)],
              "two waves of a GRU, a linear layer in the middle", dict(kernel=rt, waves="many", l2w=0), 236, gain=12.0),
    ]
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def refused_cases():
    """Stacks that must be refused at load, by name.  LSTM 130 and GRU 171 in front of a conv1d layer -- the issue's multi-wave conv-tail
    shapes -- are here for a reason: ConvTail's two scratch arrays are [widest INPUT or output][history + 128] floats, 2 x 130 x 129 x 4 =
    134 KB beside the 66 KB [samples][H] buffer, beyond the 160 KB LDS, so RecurrentWaveShape does not admit them.  The multi-wave conv-tail
    code (the first wave runs ConvTail while the others write h and c) is reached by conv-widest-lstm, conv-widest-gru (eight waves) and
    conv-lstm40 (four waves) instead."""
    hm = max_history()
    unsupported = "is not supported"
    return (
        _case("conv-hist-over-limit", "conv", [("lstm", 8), ("conv1d", 4, 2, hm + 1, "tanh"), ("dense", 1)], "hist = LSTM_MAX_TAIL_HISTORY + 1", None, 41,
              refused="more than %d samples of history" % hm),
        _case("conv-lstm130", "conv", _conv_probe("lstm", 130, 2, 1), "beyond the widest conv-tail input", None, 42, refused=unsupported),
        _case("conv-gru171", "conv", _conv_probe("gru", 171, 2, 1), "beyond the widest conv-tail input", None, 43, refused=unsupported),
        _case("conv-nine-layers", "conv", list(by_name("conv-eight-layers")["spec"]) + [("dense", 1, "tanh")], "one layer more than LSTM_MAX_TAIL", None, 44,
              refused="more than 8 dense layers"),
    )


@functools.lru_cache(maxsize=None)
def next_up_cases():
    """One size above the widest conv-tail inputs: must fail to load with the "is not supported" message or be right."""
    return tuple(_case("conv-widest-%s-plus-1" % kind, "conv", _conv_probe(kind, widest_conv_input(kind) + 1, 2, 1), "next size up", None, 50 + i)
                 for i, kind in enumerate(("lstm", "gru")))


# softmax over ONE unit is constant 1: everything behind it is a constant, so the stack cannot meet the signal-path condition of the table
# and is kept out of it; tests/test_gpu_tails.py holds its output to the same bound in a test of its own
SOFTMAX_ONE = [("lstm", 8), ("conv1d", 1, 2, 5, "softmax"), ("dense", 1)]


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


# ---- the cases of the other parts of tests/test_gpu_tails.py
GROWTH_CASES = ["conv-hist-64-1-40", "dense-gru-65-softmax"]            # hist <= 64; 65 streams and capacity growth
LEAVE_JOIN_CASE = "conv-hist-40-1-64"
MIXED_CASES = ["conv-hist-64-1-40", "conv-softmax-2", "dense-lstm-63-64-softmax"]  # two conv-tail models and a dense-tail model in one launch list
IN_PLACE_CASES = ["conv-raw-k12", "dense-gru-65-softmax"]
LEVEL_CASES = ["conv-hist-64-1-40", "conv-softmax-2", "dense-lstm-63-64-softmax"]  # elu + tanh | softmax | tanh + sigmoid + softmax
LANE_CASES = ["dense-lstm-63-64-softmax", "dense-gru-65-softmax"]      # lane = stream under NA_LSTM_NO_WAVE_RT / NA_LSTM_LANE_KERNEL
LANE_STREAMS = [1, 3, 64, 65, 130]


class Built:
    """The model document of a case and its float64 walk."""

    def __init__(self, c):
        self.case = c
        self.mj = scaled_stack(c["spec"], c["seed"], c["gain"], c["bias_scale"])
        self.doc = json.dumps(self.mj)

    def load(self, na, prewarm=None):
        m = na.NeuralModelLoader().CreateFromString(self.doc, ".json", doPrewarm=self.case["prewarm"] if prewarm is None else prewarm)
        assert m is not None, self.case["name"]
        return m

    def f64(self, x, prewarm=None, mj=None, dtype=np.float64):
        pw = 2048 if (self.case["prewarm"] if prewarm is None else prewarm) else 0
        return R.keras_stack_forward(mj or self.mj, x, prewarm=pw, dtype=dtype)

    def sizes(self):
        return call_sizes(self.case["samples"], self.case["hist"], self.case["seed"])


def signal(c, amp=1.0, stream=0, samples=None):
    return (np.float32(amp) * O.signal_noise(samples or c["samples"], 100 * c["seed"] + stream)).astype(np.float32)


def bound(want):
    return RC.bound(want)


def kernel_under_knobs(na, c):
    """The kernel that runs the case under the process's own tuning knobs ("": none -- beyond the lane = stream kernels' LDS bound)."""
    return na.recurrent_kernel(*dims(c["spec"]), knobs=None)


# ---- mutants of the float64 restatement, as documents: each is what a kernel with that defect would compute

def mutants(mj):
    """(name, document) one at a time: the oldest tap of a conv1d layer with several taps reads zeros; its dilation is one larger; softmax
    is the identity."""
    out = []
    for i, l in enumerate(mj["layers"]):
        if l["type"] == "conv1d" and int(l["kernel_size"][-1]) > 1:
            m = json.loads(json.dumps(mj))
            w = np.array(m["layers"][i]["weights"][0])
            w[0] = 0.0  # (weights [taps][in][out], tap 0 is the oldest)
            m["layers"][i]["weights"][0] = w.tolist()
            out.append(("layer %d oldest tap reads zeros" % i, m))
            m = json.loads(json.dumps(mj))
            m["layers"][i]["dilation"] = [int(l["dilation"][-1]) + 1]
            out.append(("layer %d dilation + 1" % i, m))
    if any(l.get("activation") == "softmax" for l in mj["layers"]):
        m = json.loads(json.dumps(mj))
        for l in m["layers"]:
            if l.get("activation") == "softmax":
                l["activation"] = ""
        out.append(("softmax is the identity", m))
    return out
