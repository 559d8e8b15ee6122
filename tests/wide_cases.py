"""Model shapes of the tests of the 17 .. 128 channel WaveNet kernels (wavenet_generic_kernels.hip) -- TEST INFRASTRUCTURE ONLY.

Shared by tests/test_gpu_wide.py (which runs them) and tests/test_host_cpu.py (which proves without a GPU that every generated shape
loads and that the generator reaches every edge it is meant to reach)."""
import os

import numpy as np

import na_oracle as O

# channel counts at and just past every 16- and 64-boundary of the kernels' tiling (quad, 16-block, 64-half), and the ends
EDGE_CHANNELS = [17, 18, 19, 31, 32, 33, 47, 48, 49, 63, 64, 65, 67, 80, 81, 96, 97, 113, 127, 128]
NARROW_CHANNELS = [1, 3, 8, 16]  # for arrays beside a wide one
KERNEL_SIZES = [1, 2, 3, 4, 7, 16]  # (4: the first K on the per-tap history path)
DILATIONS = [1, 2, 7, 64, 127, 128, 129, 300, 1000]  # (around the block length)
CALL_SIZES = [1, 15, 16, 17, 64, 127, 128, 129, 300]
FUZZ_SAMPLES = 1500
FUZZ_WORK_CAP = 4e9  # sum over layers of channels^2 x K x samples: oracle plus GPU stay under about two seconds
NUM_FUZZ_SEEDS = int(os.environ.get("NA_FUZZ_WIDE_SEEDS", "48"))  # (a longer campaign: NA_FUZZ_WIDE_SEEDS=400)


def chain(channels, layers, act=O.ACT_TANH, head_bias=None, head_kernel=1):
    """Layer arrays in A1 chaining (head_size[i] == channels[i + 1], last head 1): channels[i] wide, layers[i] = (kernel sizes, dilations)."""
    arrays = []
    for i, c in enumerate(channels):
        last = i == len(channels) - 1
        ks, ds = layers[i]
        arrays.append(dict(input_size=1 if i == 0 else channels[i - 1], condition_size=1, head_size=1 if last else channels[i + 1],
                           head_kernel_size=head_kernel if last else 1, head_dilation=1, channels=c,
                           has_head_bias=(last if head_bias is None else bool(head_bias[i])), activation=act,
                           kernel_sizes=list(ks), dilations=list(ds)))
    return arrays


def two_array(channels, head, act=O.ACT_TANH):
    """The two-array model of test_wavenet_of_65_to_128_channels_matches_oracle ("channels / head"; receptive field 646)."""
    return chain([channels, head], [([3, 3, 2, 3], [1, 7, 64, 200]), ([3, 5], [3, 40])], act)


def max_channels(arrays):
    """What selects the kernel (WaveNetPlan::maxChannels): the widest of channels, head size and input size."""
    return max(max(a["channels"], a["head_size"], a["input_size"]) for a in arrays)


def fuzz_work(arrays, samples=FUZZ_SAMPLES):
    return sum(a["channels"] ** 2 * k * samples for a in arrays for k in a["kernel_sizes"])


def fuzz_case(seed):
    """(arrays, call sizes) of fuzz seed `seed`.  One array's width walks through EDGE_CHANNELS with the seed, so that every edge count
    occurs whatever the number of seeds >= 20; everything else is drawn, and redrawn from the seed's own generator until the model fits
    the work cap."""
    rng = np.random.default_rng(7000 + seed)
    while True:
        n = int(rng.integers(1, 4))
        channels = [int(rng.choice(EDGE_CHANNELS + NARROW_CHANNELS)) for _ in range(n)]
        channels[int(rng.integers(0, n))] = EDGE_CHANNELS[seed % len(EDGE_CHANNELS)]
        layers = []
        for _ in range(n):
            nl = int(rng.integers(1, 5))
            layers.append(([int(rng.choice(KERNEL_SIZES)) for _ in range(nl)], [int(rng.choice(DILATIONS)) for _ in range(nl)]))
        act = O.ACT_LEAKYRELU if rng.integers(0, 2) else O.ACT_TANH
        bias = [bool(rng.integers(0, 2)) for _ in range(n)]
        # a conv head: the loader admits one on a single array of up to 64 channels only
        head_kernel = int(rng.choice([2, 7, 16])) if (n == 1 and channels[0] <= 64 and rng.integers(0, 3) == 0) else 1
        arrays = chain(channels, layers, act, bias, head_kernel)
        if fuzz_work(arrays) <= FUZZ_WORK_CAP:
            break
    sizes, left = [1, 1, 17], FUZZ_SAMPLES - 19
    while left > 0:
        c = min(int(rng.choice(CALL_SIZES)), left)
        sizes.append(c)
        left -= c
    return arrays, sizes


# the named edges, independent of the draw: channel counts of the chained arrays, activation
FIXED_LAYERS = ([1, 4, 3], [128, 129, 1000])
FIXED_CASES = [((17, 1), O.ACT_TANH), ((33, 5), O.ACT_TANH), ((49, 17), O.ACT_TANH), ((8, 40), O.ACT_TANH), ((12, 100, 24), O.ACT_TANH),
               ((65, 2), O.ACT_TANH), ((127, 127), O.ACT_LEAKYRELU), ((128, 128), O.ACT_TANH)]


def fixed_case(channels, act):
    return chain(list(channels), [FIXED_LAYERS] * len(channels), act)


# the models of the range-contract tests: (channels, head, activation) of two_array(), weight seed = channels
RANGE_MODELS = {"32/8 tanh": (32, 8, O.ACT_TANH), "128/64 tanh": (128, 64, O.ACT_TANH), "80/72 tanh": (80, 72, O.ACT_TANH),
                "24/12 leaky": (24, 12, O.ACT_LEAKYRELU), "128/128 leaky": (128, 128, O.ACT_LEAKYRELU)}
F16_MAX = 65504.0
SPLIT_SAFE = 32752.0  # half the f16 range: what the static proof keeps every split value under


def range_model(name):
    c, h, act = RANGE_MODELS[name]
    arrays = two_array(c, h, act)
    return arrays, O.synth_wavenet_weights(arrays, seed=c)


WEIGHT_SCALINGS = {"mix-in x 1e5": {"mixin": 1e5}, "1x1 x 4000": {"1x1": 4000.0},
                   "all x 1e-3": {"rechannel": 1e-3, "conv": 1e-3, "conv_bias": 1e-3, "mixin": 1e-3, "1x1": 1e-3, "1x1_bias": 1e-3, "head": 1e-3,
                                  "head_bias": 1e-3, "head_scale": 1e-3}}
