"""Model shapes of the tests of the runtime-shaped recurrent kernel (lstm_kernels.hip RecurrentWaveRtKernel) -- TEST INFRASTRUCTURE ONLY.

Shared by tests/test_gpu_recurrent_rt.py (which runs them) and tests/test_host_cpu.py (which proves without a GPU that every shape
loads, that it sits in the regime it is named for, that the set reaches every regime, and that the C oracle keeps its headroom under
the bound against the float64 restatement).

The edge units are not typed in: they are read from the library's own plan function (lstm_dev.h RecurrentWavePlan through
NA_DebugRecurrentShapePlan, evaluated with the default tuning whatever the environment says, so that a forced run gets the same cases):
a hidden size is an edge where a field of the plan differs from that of the size below it."""
import functools
import json
import os

import numpy as np

import na_oracle as O
import ref_np as R

MAX_HIDDEN = 1024
CALL_SIZES = [1, 1, 2, 3, 63, 64, 65, 127, 128, 129, 300]  # (300: chunking above LSTM_MAX_FRAMES = 128)
TOL = 5e-6  # the project's RMS tolerance, scaled as TOL * max(1, rms(want))
# tuning knobs that change the regime a shape runs in: the regime assertions are skipped under them, the parity assertions are not
KNOBS = ("NA_REC_L2W", "NA_REC_RPL", "NA_LSTM_NO_WAVE_RT", "NA_LSTM_LANE_KERNEL", "NA_LSTM_NO_DPP", "NA_GRU_NO_DPP", "NA_REC_NO_DPP32")
FIELDS = ("waves", "rows_per_lane", "l2w", "head_in_loop")
LEVELS = [1e-5, 30.0, 1000.0]


def knob_set():
    return any(os.environ.get(k) for k in KNOBS)


def bound(want):
    return TOL * max(1.0, O.rms(want))


def shape_plan(kind, hidden, layers=1, tail_layers=0, tail_width=0, tail_history=0):
    """The plan of a shape with the DEFAULT tuning (one gate row per lane, weights in LDS when they fit)."""
    import neuralaudio_amd as na
    return na.recurrent_shape_plan(kind, hidden, layers, tail_layers, tail_width, tail_history, rpl=1, force_l2w=0)


@functools.lru_cache(maxsize=None)
def edges(kind, field, layers=1):
    """Hidden sizes h in 2 .. 1024 whose plan[field] differs from that of h - 1 (a model of `layers` layers with the classic head)."""
    out, prev = [], shape_plan(kind, 1, layers)[field]
    for h in range(2, MAX_HIDDEN + 1):
        cur = shape_plan(kind, h, layers)[field]
        if cur != prev:
            out.append(h)
        prev = cur
    return out


def regime(kind, hidden, layers):
    p = shape_plan(kind, hidden, layers)
    return {f: int(p[f]) for f in FIELDS}


def _case(kind, layers, hidden, why, std=False, prewarm=False):
    # models above 256 units start from the loaded state (doPrewarm=False / prewarm off in the references) and run 150 samples
    big = hidden > 256
    return dict(kind=kind, layers=layers, hidden=hidden, why=why, std=std, prewarm=bool(prewarm and not big), samples=150 if big else 300,
                seed=1000 + 7 * hidden + layers, regime=regime(kind, hidden, layers))


def case_id(c):
    return "%s-%dx%d%s%s" % (c["kind"], c["layers"], c["hidden"], "-std" if c["std"] else "", "-pw" if c["prewarm"] else "")


def _layers_for(hidden):
    """One layer of up to 32 units runs on the LDS-free kernels (and 8 .. 32 on shaped one-wave instances): three layers put a small
    hidden size on the runtime-shaped kernel."""
    return 3 if hidden <= 32 else 1


@functools.lru_cache(maxsize=None)
def edge_cases():
    """Every edge shape: both sides of every wave-count, rows-per-lane, LDS-to-L2 and head-in-loop edge of both cell types, the largest
    sizes, H % 4 in {1, 2, 3} on both weight paths, 2 and 3 layers on multi-wave shapes, a three-layer 16-unit model."""
    cases, seen = [], set()

    def add(kind, layers, hidden, why, **kw):
        key = (kind, layers, hidden, kw.get("std", False))
        if key in seen or hidden < 1 or hidden > MAX_HIDDEN:
            return
        seen.add(key)
        cases.append(_case(kind, layers, hidden, why, **kw))

    prewarmed = {("lstm", 65), ("lstm", 129), ("gru", 86), ("gru", 171)}
    for kind in ("lstm", "gru"):
        for field in FIELDS:
            for h in edges(kind, field, 1):
                if field == "l2w":
                    continue  # (one-layer edge of the weight path: below, by name)
                for hh in (h - 1, h):
                    add(kind, _layers_for(hh), hh, "%s edge %d|%d" % (field, h - 1, h), prewarm=(kind, hh) in prewarmed)
        # the largest one-layer model whose weights sit in LDS, and the next size up
        for h in edges(kind, "l2w", 1):
            add(kind, 1, h - 1, "largest in LDS")
            add(kind, 1, h, "first streamed from L2")
        # the top of the rows-per-lane range
        add(kind, 1, MAX_HIDDEN - 1, "ragged last row block")
        add(kind, 1, MAX_HIDDEN, "largest")
    # a size in the 600s: three rows per lane, dispatch case 5 when eight rows per lane are forced; H % 4 == 1
    add("lstm", 1, 613, "three rows per lane, H % 4 == 1")
    # H % 4 on the LDS path (up to the weight-path edge) and on the L2 path
    for kind, sizes in (("lstm", (41, 42, 43, 97, 98, 99)), ("gru", (44, 45, 46, 47, 121, 122, 123))):
        for h in sizes:
            add(kind, 1, h, "H %% 4 == %d" % (h % 4))
    # 2 and 3 layers on multi-wave shapes (layer l > 0 has I = H: the input part has quads too), in LDS and streamed
    add("lstm", 2, 40, "two layers, LDS")
    add("lstm", 3, 33, "three layers, LDS, H % 4 == 1")
    add("lstm", 2, 64, "two layers, streamed")
    add("lstm", 3, 70, "three layers, streamed, H % 4 == 2")
    add("lstm", 2, 131, "two layers, head in loop, H % 4 == 3")
    add("gru", 2, 50, "two layers, LDS, H % 4 == 2")
    add("gru", 3, 91, "three layers, streamed, H % 4 == 3")
    add("gru", 2, 171, "two layers, head in loop")
    add("lstm", 3, 16, "three layers of 16 units: one wave, LDS")
    # StdMath (LSTM only) on a multi-wave shape and on a rows-per-lane > 1 shape
    add("lstm", 1, 65, "StdMath, multi-wave", std=True)
    add("lstm", 1, 257, "StdMath, two rows per lane", std=True)
    return tuple(cases)


def call_sizes(samples, seed):
    """A partition of `samples` into calls drawn from CALL_SIZES: n = 1 first, one call above LSTM_MAX_FRAMES where the signal allows."""
    rng = np.random.default_rng(seed)
    sizes, left = [1, 1, 2, 3], samples - 7
    for big in (129, 300):
        if left >= big + 8:
            sizes.append(big)
            left -= big
    while left > 0:
        c = min(int(rng.choice(CALL_SIZES[:-1])), left)
        sizes.append(c)
        left -= c
    return sizes


def run_in_calls(process, x, sizes):
    """process(chunk) over the partition; x is [samples] or [streams, samples]."""
    out, pos = [], 0
    for n in sizes:
        out.append(process(x[..., pos:pos + n]))
        pos += n
    assert pos == x.shape[-1]
    return np.concatenate(out, axis=-1)


class Built:
    """The model document of a case and its references."""

    def __init__(self, c):
        self.case = c
        if c["kind"] == "lstm":
            self.weights = O.synth_lstm_weights(c["layers"], c["hidden"], seed=c["seed"])
            self.doc, self.ext = O.nam_json_lstm(c["layers"], c["hidden"], self.weights), ".nam"
        else:
            self.gj = O.synth_keras_gru(c["layers"], c["hidden"], seed=c["seed"])
            self.doc, self.ext = json.dumps(self.gj), ".json"

    def load(self, na, loader=None):
        ld = loader or na.NeuralModelLoader()
        if self.case["std"]:
            ld = na.NeuralModelLoader()
            ld.SetLSTMMathMode(na.EMathMode.StdMath)
        m = ld.CreateFromString(self.doc, self.ext, doPrewarm=self.case["prewarm"])
        assert m is not None, case_id(self.case)
        return m

    def oracle(self, prewarm=None):
        """A fresh C oracle (float32, the reference's arithmetic and term order)."""
        c = self.case
        pw = c["prewarm"] if prewarm is None else prewarm
        if c["kind"] == "lstm":
            return O.OracleLSTM.from_nam(c["layers"], c["hidden"], self.weights, math_mode=O.MATH_STD if c["std"] else O.MATH_FAST, prewarm=pw)
        return O.OracleGRU(self.gj, prewarm=pw)

    def f64(self, x, prewarm=None):
        """The float64 restatement."""
        c = self.case
        pw = 2048 if (c["prewarm"] if prewarm is None else prewarm) else 0
        if c["kind"] == "lstm":
            if c["std"]:
                return R.lstm_forward_nam(c["layers"], c["hidden"], self.weights, x, prewarm=pw, tanh=np.tanh, sigmoid=R.std_sigmoid)
            return R.lstm_forward_nam(c["layers"], c["hidden"], self.weights, x, prewarm=pw)
        return R.gru_forward_keras(self.gj, x, prewarm=pw)


def signal(c, amp=1.0):
    return (np.float32(amp) * O.signal_noise(c["samples"], c["seed"] % 97 + 3)).astype(np.float32)


# ---- the shapes of the other parts of tests/test_gpu_recurrent_rt.py (name -> (kind, layers, hidden)) ------------------------------
BATCH_SHAPES = [("lstm", 1, 65), ("gru", 1, 86), ("lstm", 2, 64), ("lstm", 1, 257)]
SNAPSHOT_SHAPES = [("lstm", 2, 131), ("gru", 1, 171)]
POOL_SHAPES = [("lstm", 1, 129), ("gru", 1, 86)]
LEVEL_SHAPES = [("lstm", 1, 129), ("gru", 1, 171)]
TAIL_STACKS = [[("gru", 160), ("dense", 8, "tanh"), ("dense", 1)],
               [("lstm", 130), ("dense", 64, "relu"), ("dense", 1)],
               [("lstm", 40), ("conv1d", 6, 3, 64, "tanh"), ("dense", 1)],
               # one wave whose LDS is filled by the conv1d history scratch: the only way to ONE wave on L2-streamed weights by default
               [("lstm", 16), ("lstm", 16), ("lstm", 16), ("conv1d", 16, 3, 500, "tanh"), ("dense", 1)]]
TAIL_DENSE = 8  # width of the dense layer behind the widest recurrent layer that still fits


def small_case(kind, layers, hidden, prewarm=True, samples=300):
    c = _case(kind, layers, hidden, "named shape", prewarm=prewarm)
    c["samples"] = samples
    return c


def stack_dims(spec):
    """(kind, hidden, recurrent layers, tail layers, tail width, tail history) of a keras stack spec as the loader lowers it."""
    rec = [l for l in spec if l[0] in ("lstm", "gru")]
    tail = [l for l in spec if l[0] not in ("lstm", "gru")]
    hist = max([(l[2] - 1) * l[3] for l in tail if l[0] == "conv1d"] + [0])
    width, cur = 0, rec[-1][1] if rec else 1
    for l in tail:
        width = max(width, max(cur, l[1]) if hist > 0 else l[1])
        cur = l[1]
    return rec[0][0], rec[0][1], len(rec), len(tail), width, hist


def stack_id(spec):
    return "-".join("%s%d" % (l[0], l[1]) for l in spec)


def stack_regime(spec):
    p = shape_plan(*stack_dims(spec))
    return {f: int(p[f]) for f in FIELDS}


@functools.lru_cache(maxsize=None)
def widest_with_dense_tail(kind):
    """The widest one-layer recurrent model with a [TAIL_DENSE tanh, 1] dense tail that RecurrentWaveShape still admits;
    the next size up must fail to load or be right."""
    best = 0
    for h in range(1, MAX_HIDDEN + 1):
        if shape_plan(kind, h, 1, 2, TAIL_DENSE, 0)["admitted"]:
            best = h
    return best
