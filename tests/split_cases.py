"""Model shapes of the tests of the f16-split stage interpreter (wavenet_split_kernels.hip: WaveNetSplitKernel<T, SPB, WPS, GEN, PK>) on
models that are NOT one of the official architectures -- TEST INFRASTRUCTURE ONLY.

Shared by tests/test_gpu_split.py (which runs them) and tests/test_host_cpu.py (which proves without a GPU that every generated shape
loads, is predicted on the f16-split kernel with the pack factor it claims at 1 and at 600 streams, that the generator reaches every
path it names and that every case is well conditioned).  Pure Python and numpy, seeded, never skips.

The complement of tests/frame_cases.py: a WaveNet of at most 16 channels with K = 3 in every layer, 1x1 heads, last head size 1 and a
proven f16 range lands on the f16-split kernels by default (wavenet_choice.h WaveNetKernelFor; wavenet_plan.cpp splitFastT,
WaveNetPackFactor, WaveNetWantsPadding), in one of three layouts -- restated here in Python (layout_of) and held against
NA_ModelKernelInfo by the CPU proof:

* plain:   every array has exactly 8 or 16 channels (it fills its lane mode) and one of them has 16;
* padded:  every array has 5 .. 16 channels, one more than 8 and one neither 8 nor 16: 13 .. 15 (and 9 .. 12) are widened to 16,
           5 .. 7 to 8.  13 / 8 is a PADDED model (13 -> 16): only 8 and 16 fill a lane mode;
* packed:  every array has at most 8 channels: P = 2 streams per virtual stream; at most 4: P = 4.  Exactly 4 / 2 is the dense pack.

A 4-channel (or narrower) array beside a wider one takes away padding and packing alike (16 / 4, 12 / 4: the frame kernel).  The
kernel's own arrays therefore always have G = 2 or G = 4 channel groups; G = 1 exists only as one real stream's share of a pack.

LeakyReLU: the static range proof holds for the weights synth_wavenet_weights draws as long as a model has few layers (the bound grows
with the product of the layers' row sums, about x 11 per 16-channel layer): the A1-style two-array cases below pass it unscaled in
every layout -- three layers at 16 / 8 and 12 / 6, four at 8 / 4; the fuzz draws LeakyReLU on at most LEAKY_MAX_LAYERS layers.  The
same 16 / 8 with a fourth layer fails the proof, and so does a 16-channel array of 14 layers: both are decision edges.

Last head size: a PLAIN model whose last head has two channels stays on the split kernels (the plan keeps head channel 0, the only one
that reaches the output); padding and packing both require a last head of one channel, so 12 / 6 and 8 / 4 with such a head are
decision edges and plain-16-8-head2 is a case."""
import numpy as np

import na_oracle as O
from wide_cases import chain

SAMPLES = 1536              # 12 blocks: every ring of every case (at most 736 frames) wraps at least twice
BLOCK = 128
TILE = 16
COMPACT_MAX_HISTORY = 32    # WN_COMPACT_MAX_HISTORY: roundup16(2 d) <= 32 -> a compact ring of three times that (d <= 16)
MAX_SPLIT_RINGS = 63        # WN_RANGE_EVENT_SLOT: WaveNetKernelFor keeps more rings off the split kernels
WORK_CAP = 2e8              # sum over layers of channels^2 x K x samples: oracle plus GPU stay far under a second
NUM_FUZZ_SEEDS = 24
# The GPU parity bound is absolute below an output level of 1 (2e-6 RMS), and synth_wavenet_weights' head scale of 0.02 leaves these
# small models at a level of 0.002 .. 0.07: a kernel error of 1e-4 of the signal would pass.  The head scale -- one f32 multiplication at
# the very end, in the kernel, the oracle and the float64 reference alike -- is therefore raised as far as the conditioning rule of the
# CPU proof allows (the f32 oracle within 1 / 16 of the bound from float64; at x 16 the cases use 0.03 .. 0.6 of that).  The 63-ring
# model accumulates the oracle's own rounding over 63 layers and uses 0.24 of it unscaled: x 2.
HEAD_GAIN = 16.0
RINGS_HEAD_GAIN = 2.0
LEAKY_MAX_LAYERS = 2        # (all arrays together) of a LeakyReLU draw of the fuzz: every such draw passes the range proof at any width
DILATIONS = [1, 3, 5, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 200, 300]
SHIFT_GROUPS = [DILATIONS[i:i + 4] for i in range(0, 20, 4)]
CALL_SIZES = [1, 31, 63, 64, 65, 127, 128, 129, 200, 300]
EDGES = (16, 32, 64, 128)   # frames: the tile, the compact-ring limit, half a block, the block


def lane_mode(channels):
    """channel groups an array of the split kernel occupies (wavenet_plan.cpp LaneMode): 1, 2 or 4"""
    return 1 if channels <= 4 else (2 if channels <= 8 else 4)


def pack_factor(arrays):
    widest = max((a["channels"] + 3) // 4 * 4 for a in arrays)
    return 4 if widest <= 4 else (2 if widest <= 8 else 1)


def is_dense(arrays):
    return pack_factor(arrays) == 4 and [a["channels"] for a in arrays] == [4, 2]


def layout_of(arrays):
    """"plain" | "padded" | "packed" | None (None: not a model of the fast split flavour -- the frame kernel takes it)"""
    cs = [a["channels"] for a in arrays]
    if any(k != 3 for a in arrays for k in a["kernel_sizes"]) or any(a["head_kernel_size"] != 1 for a in arrays) or max(cs) > 16:
        return None
    if all(c in (8, 16) for c in cs) and max(cs) == 16:
        return "plain"  # (whatever the last head size: only head channel 0 reaches the output, the plan drops the other rows)
    if arrays[-1]["head_size"] != 1:
        return None     # neither packed nor padded (WaveNetPackFactor, WaveNetWantsPadding)
    if pack_factor(arrays) > 1:
        return "packed"
    return "padded" if min(cs) > 4 else None


def kernel_groups(arrays):
    """channel groups G of every array as the KERNEL sees it: of the packed virtual model, or of the padded one"""
    p, dense, out = pack_factor(arrays), is_dense(arrays), []
    for i, a in enumerate(arrays):
        c = a["channels"]
        if p > 1:
            out.append(p * (c if dense and i == len(arrays) - 1 else (c + 3) // 4 * 4) // 4)
        else:
            out.append(lane_mode(c))
    return out


def ring_kind(dilation, first_of_array):
    """a K = 3 layer's history ring in the split kernels' state format (wavenet_plan.cpp AddRing): "compact" (three times its padded
    history), "exact" (exactly 2 d frames) or "roomy" (padded history + a block)"""
    history = 2 * dilation
    if (history + TILE - 1) // TILE * TILE <= COMPACT_MAX_HISTORY:
        return "compact"
    if not first_of_array and dilation >= BLOCK and history >= 2 * BLOCK and history % TILE == 0:
        return "exact"
    return "roomy"


def ring_frames(dilation, first_of_array):
    h = (2 * dilation + TILE - 1) // TILE * TILE
    return {"compact": 3 * h, "exact": 2 * dilation, "roomy": h + BLOCK}[ring_kind(dilation, first_of_array)]


def num_rings(arrays):
    return sum(len(a["dilations"]) for a in arrays)


def shifts(arrays):
    """every tap shift d and 2 d"""
    return sorted({m * d for a in arrays for d in a["dilations"] for m in (1, 2)})


def work(arrays, samples=SAMPLES):
    return sum(a["channels"] ** 2 * k * samples for a in arrays for k in a["kernel_sizes"])


def receptive_field(arrays):
    return sum((k - 1) * d for a in arrays for k, d in zip(a["kernel_sizes"], a["dilations"]))


def k3(channels, dilations, act=O.ACT_TANH, head_bias=None):
    """A1 chaining, K = 3 everywhere, 1x1 heads: dilations[i] is the list of array i"""
    return chain(list(channels), [([3] * len(d), list(d)) for d in dilations], act, head_bias)


def _case(name, family, path, arrays, seed, samples=SAMPLES, gain=HEAD_GAIN):
    layout = layout_of(arrays)
    return dict(name=name, family=family, path=path, arrays=arrays, seed=seed, samples=samples, layout=layout, gain=gain,
                pack=pack_factor(arrays) if layout else 1, dense=bool(layout) and is_dense(arrays))


def weights(case):
    """synth_wavenet_weights with the head scale (its last weight, 0.02) times the case's gain"""
    return O.scale_wavenet_tensors(case["arrays"], O.synth_wavenet_weights(case["arrays"], seed=case["seed"]), {"head_scale": case["gain"]})


D2 = ([1, 3, 17, 64], [5, 128, 2])   # the default dilations of the width cases: neither Standard's nor Lite's, both ring kinds


def _name(cs):
    return "-".join(str(c) for c in cs)


def named_cases():
    cases = []

    # ---- layouts and widths (a first array without head bias like A1's; "-hb" cases give it one)
    for i, cs in enumerate([(16, 8), (16, 16), (16,), (16, 8, 8)]):
        ds = [D2[j % 2] for j in range(len(cs))]
        cases.append(_case("plain-" + _name(cs), "widths", "plain: every array fills its lane mode", k3(cs, ds, head_bias=[False] * (len(cs) - 1) + [True]), 100 + i))
    for i, cs in enumerate([(13, 8), (12, 6), (13, 5), (9, 7), (16, 5), (10,), (6, 16)]):
        ds = [D2[j % 2] for j in range(len(cs))]
        cases.append(_case("padded-" + _name(cs), "widths", "padded to %s" % _name(4 * lane_mode(c) for c in cs),
                           k3(cs, ds, head_bias=[i % 2 == 1] * (len(cs) - 1) + [True]), 110 + i))
    for i, cs in enumerate([(8, 4), (7, 3), (5, 5), (8,), (6, 8), (8, 1), (8, 4, 2)]):
        ds = [D2[j % 2] for j in range(len(cs))]
        cases.append(_case("packed2-" + _name(cs), "widths", "P = 2, virtual %s" % _name(2 * ((c + 3) // 4 * 4) for c in cs),
                           k3(cs, ds, head_bias=[i % 2 == 0] * (len(cs) - 1) + [True]), 120 + i))
    for i, cs in enumerate([(4, 2), (4, 4), (4, 3), (3, 1), (2, 2), (2, 4), (1,)]):
        ds = [D2[j % 2] for j in range(len(cs))]
        cases.append(_case("packed4-" + _name(cs), "widths", "P = 4, %s" % ("dense: virtual 16-8" if cs == (4, 2) else "virtual " + _name([16] * len(cs))),
                           k3(cs, ds, head_bias=[i % 2 == 1] * (len(cs) - 1) + [True]), 130 + i))
    cases.append(_case("plain-16-8-hb", "widths", "plain, first array with a head bias", k3((16, 8), D2, head_bias=[True, True]), 140))
    cases.append(_case("packed4-4-2-hb", "widths", "dense pack, first array with a head bias", k3((4, 2), D2, head_bias=[True, False]), 141))
    # a last head of two channels: a plain model stays here (the plan keeps head row 0 and walks past the other's weights and bias)
    cases.append(_case("plain-16-8-head2", "widths", "plain, last head size 2 (only channel 0 is the output)", last_head_2((16, 8)), 142))

    # ---- tap shifts d and 2 d on both sides of 16 (the tile), 32 (compact rings), 64 and 128 (the block): the twenty dilations in
    # groups of four, ascending in the first array and descending in the second (so both ends of a group open an array), on a plain
    # 16 / 8 (kernel G = 4 and 2), a P = 2 pack 8 / 4 (virtual 16 / 8) and a P = 4 pack of 3 channels (one real group per stream)
    for j, ds in enumerate(SHIFT_GROUPS):
        for i, cs in enumerate([(16, 8), (8, 4), (3,)]):
            cases.append(_case("shift-d%d-%s" % (ds[0], _name(cs)), "tap shifts", "dilations %s, %s" % (ds, layout_of(k3(cs, [ds] * len(cs)))),
                               k3(cs, [ds, ds[::-1]][:len(cs)]), 200 + 3 * j + i))

    # ---- layer count: arrays of one layer; 63 rings (cursor 62 lies beside the range-event word; 64 rings are refused)
    cases.append(_case("one-layer-16-8", "layers", "one layer per array, plain", k3((16, 8), ([17], [3])), 300))
    cases.append(_case("one-layer-4-2", "layers", "one layer per array, dense pack", k3((4, 2), ([64], [1])), 301))
    cases.append(_case("one-layer-10", "layers", "one array of one layer, padded", k3((10,), ([129],)), 302))
    cases.append(rings_model(MAX_SPLIT_RINGS))

    # ---- LeakyReLU on A1-style arrays (the range proof holds for them as drawn: see the module docstring)
    for i, (cs, ds) in enumerate([((16, 8), ([1, 17], [64])), ((12, 6), ([5, 128], [2])), ((8, 4), ([1, 33], [16, 200])), ((4, 2), ([3, 65], [17]))]):
        cases.append(_case("leaky-" + _name(cs), "activation", "LeakyReLU, " + layout_of(k3(cs, ds)), k3(cs, ds, O.ACT_LEAKYRELU, head_bias=[False, True]), 320 + i))
    return cases


def rings_model(rings):
    """one array of two channels with `rings` layers (P = 4): 63 is the most the split kernels take"""
    ds = [[1, 2, 3, 5, 8, 16, 17, 33][i % 8] for i in range(rings)]
    return _case("rings-%d" % rings, "layers", "%d rings" % rings, k3((2,), (ds,)), 310, gain=RINGS_HEAD_GAIN)


def last_head_2(channels):
    arrays = k3(channels, D2)
    arrays[-1]["head_size"] = 2
    return arrays


def decision_edges():
    """(name, arrays, seed): models next to the table's that must NOT land on the split kernels -- asserted on the CPU only"""
    leaky = [dict(input_size=1, condition_size=1, head_size=1, head_kernel_size=1, head_dilation=1, channels=16, has_head_bias=True,
                  activation=O.ACT_LEAKYRELU, kernel_sizes=[3] * 14, dilations=[1 << (i % 9) for i in range(14)])]
    return [("16-4", k3((16, 4), D2), 1), ("12-4", k3((12, 4), D2), 2), ("rings-64", rings_model(MAX_SPLIT_RINGS + 1)["arrays"], 310),
            ("k2", chain([16], [([2], [1])]), 3), ("padded-last-head-2", last_head_2((12, 6)), 4), ("packed-last-head-2", last_head_2((8, 4)), 5),
            ("leaky-16-8-four-layers", k3((16, 8), ([1, 17], [64, 3]), O.ACT_LEAKYRELU, head_bias=[False, True]), 320), ("leaky-14-layers", leaky, 7)]


_POOLS = {"plain": [8, 16], "padded": [5, 6, 7, 9, 10, 12, 13, 15, 16, 8], "packed2": [5, 6, 7, 8, 1, 3, 4], "packed4": [1, 2, 3, 4]}


def fuzz_case(seed):
    """(case, call sizes) of fuzz seed `seed`: a layout by the seed, widths, array count, dilations, bias and activation drawn; redrawn
    from the seed's own generator until the draw has the layout it was drawn for."""
    rng = np.random.default_rng(9500 + seed)
    want = ["plain", "padded", "packed2", "packed4"][seed % 4]
    while True:
        leaky = bool(rng.integers(0, 3) == 0)  # (then at most LEAKY_MAX_LAYERS layers: one or two arrays of one)
        n = int(rng.integers(1, 3 if leaky else 4))
        cs = [int(rng.choice(_POOLS[want])) for _ in range(n)]
        ds = [[int(rng.choice(DILATIONS)) for _ in range(1 if leaky else int(rng.integers(1, 5)))] for _ in range(n)]
        bias = [bool(rng.integers(0, 2)) for _ in range(n)]
        arrays = k3(cs, ds, O.ACT_LEAKYRELU if leaky else O.ACT_TANH, bias)
        got = layout_of(arrays)
        if got == "packed":
            got = "packed%d" % pack_factor(arrays)
        if got == want and work(arrays) <= WORK_CAP:
            break
    sizes, left = [1, 1, 17, 300], SAMPLES - 319  # (one size above 128 whatever the draw: the host cuts it)
    while left > 0:
        c = min(int(rng.choice(CALL_SIZES)), left)
        sizes.append(c)
        left -= c
    return _case("fuzz-%d" % seed, "fuzz " + want, "seeded draw", arrays, 600 + seed), sizes


# ---- the batch tests' models (tests/test_gpu_split.py b .. e): custom throughout

def plain_custom():
    return _case("batch-plain-16-8", "batch", "plain custom 16 / 8", k3((16, 8), ([1, 17, 64], [3, 128])), 400)


def packed2_custom():
    return _case("batch-p2-8-4", "batch", "P = 2 custom 8 / 4", k3((8, 4), ([3, 16, 65], [1, 33])), 401)


def packed4_custom():
    return _case("batch-p4-3-1", "batch", "P = 4 custom 3 / 1 (not dense)", k3((3, 1), ([1, 17, 64], [5, 129])), 402)


def dense_custom():
    return _case("batch-p4-4-2", "batch", "P = 4 custom 4 / 2 (dense), not Nano's dilations", k3((4, 2), ([3, 16, 65], [1, 33, 128])), 403)


def batch_models():
    return [plain_custom(), packed2_custom(), packed4_custom(), dense_custom()]
