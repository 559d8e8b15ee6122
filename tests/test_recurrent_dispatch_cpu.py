"""Which kernel runs a recurrent model (lstm_dev.h RecurrentKernelFor through NA_DebugRecurrentKernel), without a GPU.

The rule is restated below in Python from the launch cascades the function replaced (LaunchLstmBlock / LaunchLstmWave / LaunchGruBlock /
LaunchRecurrentWaveRt and the plan they read), step by step as they tried their kernels, and compared with the library over a grid of
shapes, tails and knob sets.  The runtime-shaped kernel's plan (NA_DebugRecurrentShapePlan) is compared with the values the library gave
before the decision moved (tests/golden/recurrent_plan_grid.npz: `python tests/test_recurrent_dispatch_cpu.py FILE` records the grid from
whatever build of the package is first on the path; the file in the tree is from the commit before RecurrentKernelFor).

Hidden sizes: 1 .. 72, both sides of every edge that recurrent_cases.edges() finds in a field of the plan (one to three layers), 1023
and 1024 -- the whole range 1 .. 1024 over ten knob sets is some millions of calls through ctypes."""
import collections
import os

import numpy as np
import pytest

import recurrent_cases as RC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "recurrent_plan_grid.npz")
LDS = 160 * 1024
MAX_FRAMES = 128
LAYERS = range(0, 9)
# (tail layers, widest tail layer, conv1d history)
TAILS = [(0, 0, 0), (2, 8, 0), (2, 256, 0), (2, 8, 10), (2, 8, 1000), (2, 64, 1000)]
KNOB_SETS = [dict(), dict(NA_LSTM_NO_DPP=1, NA_GRU_NO_DPP=1), dict(NA_LSTM_NO_DPP=1), dict(NA_GRU_NO_DPP=1), dict(NA_LSTM_LANE_KERNEL=1),
             dict(NA_LSTM_NO_WAVE_RT=1), dict(NA_REC_NO_DPP32=1), dict(NA_REC_RPL=4), dict(NA_REC_RPL=8), dict(NA_REC_L2W=1)]
# the plan's own knobs, as NA_DebugRecurrentShapePlan takes them: (rpl, forceL2w)
PLAN_KNOBS = [(1, 0), (4, 0), (8, 0), (1, 1)]


def hidden_sizes():
    hs = set(range(1, 73)) | {1023, 1024}
    for kind in ("lstm", "gru"):
        for field in RC.FIELDS:
            for layers in (1, 2, 3):
                for h in RC.edges(kind, field, layers):
                    hs |= {h - 1, h}
    return sorted(hs)


# ---- the parent's code, restated ------------------------------------------------------------------------------------------------------
def tail_scratch(tw, th):
    return 2 * tw * (th + MAX_FRAMES) if th > 0 else 2 * tw * 64


def wave_lds_floats(gru, H, L, tw, th, has_tail, weights):
    rows, biases = (3 if gru else 4) * H, (6 if gru else 4) * H
    hseq = not (H >= 129 and not has_tail)
    f = MAX_FRAMES + 2 * L * H + 6 * H + (2 * (H if L > 0 else 1) * 64 if hseq else 0) + tail_scratch(tw, th)
    if weights:
        for l in range(L):
            f += rows * (((1 if l == 0 else H) + H) | 1) + biases
    return f


def wave_shape(H, L, tw, th):
    if not (1 <= H <= 1024 and (0 if tw > 0 else 1) <= L <= 8 and tw <= max(256, H if th > 0 else 0) and th <= 1024):
        return False
    hseq = not (H >= 129 and not tw > 0)
    return (MAX_FRAMES + 2 * L * H + 6 * H + (2 * (H if L > 0 else 1) * 64 if hseq else 0) + tail_scratch(tw, th) + 64) * 4 <= LDS


def lstm_generic_lds(H, L, tw, n=MAX_FRAMES):
    return (64 * (n + 1) + L * 2 * H * 64 + H * 64 + 2 * tw * 64) * 4


def lstm_block_lds(H, L, n=MAX_FRAMES):
    return (64 * (n + 1) + L * 2 * H * 64) * 4


def gru_generic_lds(H, L, tw, n=MAX_FRAMES):
    return (64 * (n + 1) + L * H * 64 + 6 * H * 64 + 2 * tw * 64) * 4


def lstm_shape_supported(H, L, tw, th):
    lane = H >= 1 and (0 if tw > 0 else 1) <= L <= 8 and tw <= 256 and lstm_generic_lds(H, L, tw) <= LDS
    return (th == 0 and lane) or wave_shape(H, L, tw, th)


def gru_shape_supported(H, L, tw, th):
    lane = H >= 1 and 1 <= L <= 8 and tw <= 256 and gru_generic_lds(H, L, tw) <= LDS
    return (th == 0 and lane) or (L >= 1 and wave_shape(H, L, tw, th))


def dpp_shape(H, L, tl, knobs):
    if tl != 0:
        return False
    if L == 1 and 16 < H <= 32:
        return not knobs.get("NA_REC_NO_DPP32")
    return 1 <= H <= 16 and L in (1, 2)


def wave_plan(gru, H, L, tl, tw, th, have_wt, knobs):
    """RecurrentWavePlan as it was: `runs` restates who the two cascades let go first."""
    rpl = knobs.get("NA_REC_RPL", 1)
    has_tail, conv = tl > 0, tl > 0 and th > 0
    gate_rows = (3 if gru else 4) * H
    waves = 1
    while waves < 16 and gate_rows > 64 * rpl * waves:
        waves *= 2
    tw, th = (tw, th) if has_tail else (0, 0)
    lds = wave_lds_floats(gru, H, L, tw, th, has_tail, True) * 4
    l2w = lds > LDS or bool(knobs.get("NA_REC_L2W") and L > 0)
    if l2w:
        lds = wave_lds_floats(gru, H, L, tw, th, has_tail, False) * 4
    shaped_first = False
    if not has_tail:
        listed = H in (8, 12, 16, 20) or (not gru and H in (24, 32))
        shaped_first = (not knobs.get("NA_GRU_NO_DPP" if gru else "NA_LSTM_NO_DPP") and dpp_shape(H, L, tl, knobs)) or (listed and L in (1, 2))
    off = bool(knobs.get("NA_LSTM_NO_WAVE_RT") or (not gru and knobs.get("NA_LSTM_LANE_KERNEL"))) and not conv
    runs = not shaped_first and not off and 1 <= H <= 1024 and L >= 0 and not (L == 0 and not has_tail) and (not l2w or have_wt) and lds <= LDS
    return dict(runs=int(runs), waves=waves, rows_per_lane=(gate_rows + 64 * waves - 1) // (64 * waves), l2w=int(l2w),
                head_in_loop=int(H >= 129 and not has_tail), lds_bytes=lds)


def lstm_cascade(H, L, tl, tw, th, have_wt, knobs):
    """LaunchLstmBlock, LaunchLstmWave"""
    conv = tl > 0 and th > 0
    lane = bool(knobs.get("NA_LSTM_LANE_KERNEL")) and not conv
    if not lane and tl == 0:
        if not knobs.get("NA_LSTM_NO_DPP") and dpp_shape(H, L, tl, knobs):
            return "RecurrentDppKernel"
        if H in (8, 12, 16, 20, 24, 32) and L in (1, 2):
            return "LstmWaveKernel"
    if not lane and wave_plan(False, H, L, tl, tw, th, have_wt, knobs)["runs"]:
        return "RecurrentWaveRtKernel"
    if conv:
        return ""
    if tl > 0:
        return "LstmGenericKernel" if lstm_generic_lds(H, L, tw) <= LDS else ""
    if H in (4, 8, 12, 16, 20, 24, 32, 40):
        return "LstmBlockKernel" if lstm_block_lds(H, L) <= LDS else ""
    return "LstmGenericKernel" if lstm_generic_lds(H, L, 0) <= LDS else ""


def gru_cascade(H, L, tl, tw, th, have_wt, knobs):
    """LaunchGruBlock"""
    if not gru_shape_supported(H, L, tw if tl > 0 else 0, th if tl > 0 else 0):
        return ""
    rt = wave_plan(True, H, L, tl, tw, th, have_wt, knobs)["runs"]
    if tl > 0:
        if rt:
            return "RecurrentWaveRtKernel"
        if th > 0:
            return ""
        return "GruGenericKernel" if gru_generic_lds(H, L, tw) <= LDS else ""
    if not knobs.get("NA_GRU_NO_DPP") and dpp_shape(H, L, tl, knobs):
        return "RecurrentDppKernel"
    if H in (8, 12, 16, 20) and L <= 2:
        return "GruWaveKernel"
    if rt:
        return "RecurrentWaveRtKernel"
    return "GruGenericKernel" if gru_generic_lds(H, L, 0) <= LDS else ""


def cascade(kind, *a):
    return gru_cascade(*a) if kind == "gru" else lstm_cascade(*a)


NAMES = ["", "RecurrentDppKernel", "LstmWaveKernel", "GruWaveKernel", "RecurrentWaveRtKernel", "LstmBlockKernel", "LstmGenericKernel", "GruGenericKernel"]


def library_kernel(na, kind, H, L, tail, have_wt, knobs):
    """NA_DebugRecurrentKernel's answer as a name (the raw entry point: the grid is some hundred thousand calls)"""
    mask = sum(na.RECURRENT_KNOB_BITS[k] for k in knobs if k != "NA_REC_RPL")
    r = na.capi.load_library().NA_DebugRecurrentKernel(int(kind == "gru"), H, L, tail[0], tail[1], tail[2], int(have_wt), mask, knobs.get("NA_REC_RPL", 0), None, 0)
    assert r >= 0
    return NAMES[r]


def plan_grid(na, hs):
    """The seven outputs of NA_DebugRecurrentShapePlan over the grid: int32 [plan knobs][cell][hidden][layers][tail][output]; the last is its
    return value (the loader's shape predicate of the runtime-shaped kernel admits the shape)"""
    import ctypes
    fn, six = na.capi.load_library().NA_DebugRecurrentShapePlan, (ctypes.c_int * 6)()
    out = np.zeros((len(PLAN_KNOBS), 2, len(hs), len(LAYERS), len(TAILS), 7), np.int32)
    for a, (rpl, l2w) in enumerate(PLAN_KNOBS):
        for cell in (0, 1):
            for c, H in enumerate(hs):
                for L in LAYERS:
                    for e, tail in enumerate(TAILS):
                        r = fn(cell, H, L, tail[0], tail[1], tail[2], rpl, l2w, six)
                        out[a, cell, c, L, e] = list(six) + [r]
    return out


def ranges(values):
    """[1, 2, 3, 7, 9, 10] -> '1-3, 7, 9-10'"""
    out, values = [], sorted(values)
    for v in values:
        if out and v == out[-1][1] + 1:
            out[-1][1] = v
        else:
            out.append([v, v])
    return ", ".join("%d" % a if a == b else "%d-%d" % (a, b) for a, b in out)


def describe(na, knobs):
    """{kernel: ['lstm 1 layer: 1-32', ...]} for the models with the classic head that the loader admits (the table of DESIGN.md 6a)"""
    table = collections.defaultdict(list)
    for kind, supported in (("lstm", lstm_shape_supported), ("gru", gru_shape_supported)):
        by = collections.defaultdict(lambda: collections.defaultdict(list))
        for L in range(1, 9):
            for H in range(1, 1025):
                if supported(H, L, 0, 0):
                    by[library_kernel(na, kind, H, L, (0, 0, 0), True, knobs)][L].append(H)
        for name, per_layers in by.items():
            merged = collections.defaultdict(list)  # layer counts with the same hidden sizes on one line
            for L, hs in per_layers.items():
                merged[ranges(hs)].append(L)
            table[name] += ["%s x %s layers: %s units" % (kind, ranges(Ls), hs) for hs, Ls in merged.items()]
    return table


def render_enumeration(na):
    """The block of DESIGN.md 6a between the lines `<!-- recurrent kernel enumeration` and `-->`... its fenced text, generated"""
    out, default = [], describe(na, {})
    for knobs in KNOB_SETS:
        table = describe(na, knobs)
        out.append("%s:%s" % (", ".join("%s=%s" % kv for kv in knobs.items()) or "no knob set", " as with no knob set" if knobs and table == default else ""))
        for name, lines in sorted(table.items()) if not knobs or table != default else []:
            out += ["  %s" % (name or "(no kernel: the launch is an error)")] + ["    " + l for l in lines]
    return "\n".join(out) + "\n"


# ---- the tests ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    return neuralaudio_amd


def test_the_library_chooses_what_the_launch_cascades_chose(na):
    """Every cell type, hidden size, layer count, tail, weight image and knob set of the grid: the library's answer is the cascades'."""
    wrong, count = [], 0
    for knobs in KNOB_SETS:
        for kind in ("lstm", "gru"):
            for H in hidden_sizes():
                for L in LAYERS:
                    for tail in TAILS:
                        for have_wt in (False, True):
                            want, got = cascade(kind, H, L, *tail, have_wt, knobs), library_kernel(na, kind, H, L, tail, have_wt, knobs)
                            count += 1
                            if want != got and len(wrong) < 20:
                                wrong.append((knobs, kind, H, L, tail, have_wt, want, got))
    print("%d decisions compared" % count)
    assert not wrong, wrong


def test_every_shape_the_loader_admits_has_a_kernel_and_the_default_set_is_known(na, capsys):
    """With no knob set: no model loads and then has no kernel; and the kernels a default load can reach, with the transposed weight image
    every model with a recurrent layer has (the source of DESIGN.md 6a's sentence on the lane = stream kernels)."""
    reached = collections.defaultdict(set)
    for kind, supported in (("lstm", lstm_shape_supported), ("gru", gru_shape_supported)):
        for H in range(1, 1025):
            for L in LAYERS:
                for tail in TAILS:
                    if supported(H, L, tail[1], tail[2]):
                        name = library_kernel(na, kind, H, L, tail, L > 0, {})
                        assert name != "", (kind, H, L, tail)
                        reached[name].add((kind, L, H) if tail[0] == 0 else (kind, L, H, tail))
    with capsys.disabled():
        print("\nkernels reachable with no knob set: " + ", ".join("%s (%d shapes of the grid)" % (k, len(v)) for k, v in sorted(reached.items())))
    assert set(reached) == {"RecurrentDppKernel", "LstmWaveKernel", "GruWaveKernel", "RecurrentWaveRtKernel"}
    # the default table of DESIGN.md 6a, from the enumeration
    assert {s for s in reached["LstmWaveKernel"]} == {("lstm", 2, h) for h in (20, 24, 32)}
    assert {s for s in reached["GruWaveKernel"]} == {("gru", 2, 20)}
    dpp = {s for s in reached["RecurrentDppKernel"]}
    assert dpp == {(k, 1, h) for k in ("lstm", "gru") for h in range(1, 33)} | {(k, 2, h) for k in ("lstm", "gru") for h in range(1, 17)}


def test_design_md_holds_the_enumeration_as_generated(na):
    """DESIGN.md 6a's listing of which kernel takes which shapes under which knob is this module's output, not typed in:
    `python tests/test_recurrent_dispatch_cpu.py --enumeration` prints the block."""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md"), encoding="utf-8").read()
    begin, end = "<!-- recurrent kernel enumeration: generated -->\n```\n", "```\n<!-- end of the generated enumeration -->"
    assert begin in text and end in text
    assert text[text.index(begin) + len(begin):text.index(end)] == render_enumeration(na)


def test_the_plan_is_what_it_was_and_says_runs_where_the_decision_says_the_runtime_shaped_kernel(na):
    """The whole grid, hidden sizes 1 .. 1024: the outputs of NA_DebugRecurrentShapePlan are the recorded ones, and plan.runs == (kernel ==
    WaveRt) under the knobs the plan was asked with."""
    gold = load_golden()
    hs = list(range(1, 1025))
    now = plan_grid(na, hs)
    assert now.shape == gold.shape
    assert np.array_equal(now[..., 1:], gold[..., 1:])
    # `runs`: as recorded, except where the recorded plan said 1 for a GRU shape that the launcher then refused (LaunchGruBlock returned
    # hipErrorInvalidValue on !GruShapeSupported before it asked the plan; no such model loads): those say 0 now
    refused = np.zeros(now.shape[:-1], bool)
    for c, H in enumerate(hs):
        for L in LAYERS:
            for e, tail in enumerate(TAILS):
                refused[:, 1, c, L, e] = not gru_shape_supported(H, L, tail[1], tail[2])
    diff = now[..., 0] != gold[..., 0]
    print("runs differs from the recording at %d of %d points; refused GRU shapes: %d" % (diff.sum(), diff.size, refused.sum()))
    assert np.array_equal(now[..., 0][~refused], gold[..., 0][~refused])
    assert not now[..., 0][refused].any()
    for a, knobs in enumerate(({}, {"NA_REC_RPL": 4}, {"NA_REC_RPL": 8}, {"NA_REC_L2W": 1})):
        for cell, kind in enumerate(("lstm", "gru")):
            for c, H in enumerate(hs):
                for L in LAYERS:
                    for e, tail in enumerate(TAILS):
                        assert bool(now[a, cell, c, L, e, 0]) == (library_kernel(na, kind, H, L, tail, True, knobs) == "RecurrentWaveRtKernel"), (kind, H, L, tail, knobs)


def load_golden():
    """[plan knobs][cell][hidden][layers][tail][output] from the file's two arrays: the six small outputs as int8, the LDS bytes as
    differences along the hidden axis (they compress to a tenth that way)"""
    g = np.load(GOLDEN)
    small = g["small"].astype(np.int32)
    return np.concatenate([small[..., :5], np.cumsum(g["lds_step"], axis=2, dtype=np.int64).astype(np.int32)[..., None], small[..., 5:]], axis=-1)


if __name__ == "__main__":
    import sys
    import neuralaudio_amd  # (the build on PYTHONPATH)
    if sys.argv[1] == "--enumeration":
        sys.stdout.write(render_enumeration(neuralaudio_amd))
        sys.exit(0)
    grid = plan_grid(neuralaudio_amd, list(range(1, 1025)))
    np.savez_compressed(sys.argv[1], small=np.delete(grid, 5, axis=-1).astype(np.int8), lds_step=np.diff(grid[..., 5], axis=2, prepend=0))
