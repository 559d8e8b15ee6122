"""Model shapes of the tests of the f32 frame kernel (wavenet_frame_kernels.hip: WaveNetFrameKernel, every WaveNet of at most 16
channels that the f16-split kernels do not take) -- TEST INFRASTRUCTURE ONLY.

Shared by tests/test_gpu_frame.py (which runs them) and tests/test_host_cpu.py (which proves without a GPU that every generated shape
loads, is predicted to run on the frame kernel at 1 and at 600 streams, and that the generator reaches every path it names).  Pure
Python and numpy, seeded, never skips.

What lands a model of <= 16 channels on the frame kernel by default (wavenet_choice.h WaveNetKernelFor): a layer kernel size
other than 3 or a conv head (unless it is one of the two official A2 shapes), or a failed range proof.  Every case below has one of
the three, and says which path of the kernel it is for.  The complement -- K = 3 everywhere, 1x1 heads and a proven range: the f16-split
kernels -- is tests/split_cases.py."""
import numpy as np

import na_oracle as O
from wide_cases import chain

SAMPLES = 1536           # 12 blocks: every ring of every case (at most 736 frames, MAX_REACH) wraps at least twice
BLOCK = 128
TILE = 16
MAX_REACH = 600          # (K - 1) d of any layer: a ring of roundup16(reach) + 128 <= 736 frames
STAGER_F4 = 384          # float4 the kernel's WeightStager copies without its tail loop at up to two waves per workgroup (6 KB) ...
STAGER_F4_SPB = 512      # ... and at four or eight (two or four streams per workgroup)
HPF_WIDE = 5             # shifted taps whose history is requested a layer ahead in runs of G <= 2 layers of a model with a K > 3
HEAD_SHORT_REACH = 16    # head reach (K - 1) x dilation up to which HeadConvLds runs (OtherStage: shortReach), HeadConvPk beyond
WORK_CAP = 2e8           # sum over layers of channels^2 x K x samples: oracle plus GPU stay far under a second
NUM_FUZZ_SEEDS = 28
RULE_F32, RULE_F64 = "f32 oracle, per 32-frame window", "float64 reference, 4 x the oracle's distance"

CHANNELS = [1, 3, 4, 5, 8, 10, 12, 13, 16]
SHIFT_DILATIONS = [1, 63, 64, 65, 127, 128, 129, 200]
PREFETCH_KERNELS = [4, 5, 6, 7, 15]
CALL_SIZES = [1, 31, 63, 64, 65, 127, 128, 129, 200, 300]


def groups(channels):
    return (channels + 3) // 4


def layer_block_f4(ksize, channels):
    """float4 of a layer stage's staged weight block (frame_lds.h FrameLayerBlockFloats): K taps and the 1x1, three vectors"""
    g = groups(channels)
    return ((ksize + 1) * 64 * g + 12 * g) // 4


def ring_frames(reach):
    """frames of a layer's history ring in the frame kernel's state format (wavenet_plan.cpp AddRing)"""
    return (reach + TILE - 1) // TILE * TILE + BLOCK


def layer_shifts(arrays):
    """every (K - 1 - t) d of every shifted tap"""
    return sorted({(k - 1 - t) * d for a in arrays for k, d in zip(a["kernel_sizes"], a["dilations"]) for t in range(k - 1)})


def work(arrays, samples=SAMPLES):
    return sum(a["channels"] ** 2 * k * samples for a in arrays for k in a["kernel_sizes"])


def receptive_field(arrays):
    return sum((k - 1) * d for a in arrays for k, d in zip(a["kernel_sizes"], a["dilations"])) + \
        (arrays[-1]["head_kernel_size"] - 1) * arrays[-1]["head_dilation"]


def _case(name, family, path, arrays, seed, rule=RULE_F32, scale=None, samples=SAMPLES):
    return dict(name=name, family=family, path=path, arrays=arrays, seed=seed, rule=rule, scale=scale, samples=samples)


def weights(case):
    w = O.synth_wavenet_weights(case["arrays"], seed=case["seed"])
    return O.scale_wavenet_tensors(case["arrays"], w, case["scale"]) if case["scale"] else w


def _act(i):
    return O.ACT_LEAKYRELU if i % 2 else O.ACT_TANH


def named_cases():
    cases = []

    # ---- G sweep: every channel-group count 1 .. 4 with channel counts that do not fill the group; K = 2 lands them on this kernel with
    # ordinary weights.  Two arrays: equal G on both sides of the link (8 -> 5, 16 -> 13: the link sits between two runs of one
    # instantiation of RunLayers) and different G (13 -> 3, 4 -> 10, 1 -> 12: the next run is another instantiation).
    for i, c in enumerate(CHANNELS):
        cases.append(_case("g-%d" % c, "g sweep", "RunLayers<G = %d>, %d of %d channels of the last group real" % (groups(c), c - 4 * (groups(c) - 1), 4),
                           chain([c], [([2, 2], [1, 3])], _act(i)), 100 + i))
    for i, (c1, c2) in enumerate([(13, 3), (8, 5), (16, 13), (4, 10), (1, 12)]):
        same = groups(c1) == groups(c2)
        cases.append(_case("g-%d-%d" % (c1, c2), "g sweep", "array link between runs of %s G (%d -> %d)" % ("equal" if same else "different", groups(c1), groups(c2)),
                           chain([c1, c2], [([2, 2], [1, 3]), ([2, 2], [2, 1])], _act(i), head_bias=[i % 2 == 0, True]), 120 + i))

    # ---- tap shifts (K - 1 - t) d on both sides of 64 and 128 frames: FetchFrame's whole wave in block / in history / straddling, the
    # predicated LoadHistory of the prefetched taps; 6 channels (G = 2: K = 4 makes its run HPF_WIDE) and 16 (G = 4: HPF_NARROW, the
    # third tap of K = 4 loads in line)
    for k in (2, 4):
        for j, ds in enumerate((SHIFT_DILATIONS[:4], SHIFT_DILATIONS[4:])):
            for c in (6, 16):
                cases.append(_case("shift-k%d-d%d-c%d" % (k, ds[0], c), "tap shifts", "K = %d, dilations %s, G = %d" % (k, ds, groups(c)),
                                   chain([c], [([k] * 4, list(ds))], _act(j)), 140 + 10 * k + 2 * j + (c == 16)))
    cases.append(_case("shift-k1", "tap shifts", "a K = 1 layer (no history, no ring read) between K = 2 layers",
                       chain([5], [([2, 1, 2], [64, 7, 1])], O.ACT_TANH), 190))

    # ---- prefetch depth: G <= 2 models with a K > 3 run HPF_WIDE (five shifted taps requested a layer ahead): K - 1 = 3, 4 below, 5 at,
    # 6 and 14 above (the rest load in line); the same sizes at G = 3 and 4 run HPF_NARROW (two ahead, the rest in line)
    for c in (2, 8, 10, 16):
        for i, k in enumerate(PREFETCH_KERNELS):
            cases.append(_case("prefetch-c%d-k%d" % (c, k), "prefetch depth", "%s at G = %d, %d shifted taps" % ("HPF_WIDE" if c <= 8 else "HPF_NARROW", groups(c), k - 1),
                               chain([c], [([k, k], [1, 9])], _act(i)), 200 + 10 * groups(c) + i))

    # ---- staged block size: WeightStager copies 384 float4 per stage at up to two waves per workgroup and finishes larger blocks in the
    # tail loop of End().  16 channels: K = 4 -> 332, K = 5 -> 396, K = 6 -> 460, K = 7 -> 524 float4 (the 1x1 counts as a tap: K = 5 is
    # the first size ABOVE 384, K = 7 the first above the 512 of a four-wave workgroup); 4 channels: K = 22 -> 371, K = 23 -> 387
    for i, (c, k) in enumerate([(16, 4), (16, 5), (16, 6), (16, 7), (4, 22), (4, 23)]):
        cases.append(_case("staged-c%d-k%d" % (c, k), "staged block", "%d float4 staged (stager: %d)" % (layer_block_f4(k, c), STAGER_F4),
                           chain([c], [([k, 2], [1, 5])], _act(i)), 260 + i))

    # ---- conv heads (head dilation is 1 in every .nam file: the reach is head_kernel_size - 1, so a reach above 16 always comes from K):
    # reach 15 and 16 run HeadConvLds (shortReach: reach <= 16), 17 runs HeadConvPk; head G = 1 .. 4; bias on and off on both sides.
    # Reach 69: taps whose whole first wave lies in the history ring.
    for i, hk in enumerate((16, 17, 18)):
        for j, c in enumerate((3, 8, 10, 16)):
            cases.append(_case("head-k%d-c%d" % (hk, c), "conv head", "%s, head G = %d, reach %d" % ("HeadConvLds" if hk - 1 <= HEAD_SHORT_REACH else "HeadConvPk", groups(c), hk - 1),
                               chain([c], [([2, 3], [1, 2])], _act(i + j), head_bias=[(i + j) % 2 == 0], head_kernel=hk), 300 + 4 * i + j))
    cases.append(_case("head-k2-c5", "conv head", "HeadConvLds, reach 1", chain([5], [([3, 3], [1, 2])], O.ACT_TANH, head_bias=[False], head_kernel=2), 320))
    cases.append(_case("head-k70-c4", "conv head", "HeadConvPk, reach 69 (beyond a wave)", chain([4], [([2], [1])], O.ACT_LEAKYRELU, head_bias=[True], head_kernel=70), 321))

    # ---- no range proof: A1 Standard (K = 3 everywhere: the split chain's shape) with its 1x1 weights x 4000, the scaling of
    # test_models_without_a_range_proof_run_on_the_f32_kernel.  Badly conditioned on purpose: held to the float64 rule.  Its longest ring
    # (d = 512: 1152 frames) wraps twice in 2560 samples.
    cases.append(_case("no-proof-a1", "no range proof", "A1 Standard shape without the f16 range proof", O.a1_arrays(16, 8), 21,
                       rule=RULE_F64, scale={"1x1": 4000.0}, samples=2560))
    return cases


def fuzz_case(seed):
    """(case, call sizes) of fuzz seed `seed`: the families above, drawn; redrawn from the seed's own generator until the model is certain
    to land on the frame kernel (a layer with K != 3 or a conv head) within the reach and work caps."""
    rng = np.random.default_rng(9000 + seed)
    family = ["g sweep", "tap shifts", "prefetch depth", "staged block", "conv head", "mixed"][seed % 6]
    while True:
        n = int(rng.integers(1, 3))
        channels = [int(rng.choice(CHANNELS + [2, 6])) for _ in range(n)]
        channels[int(rng.integers(0, n))] = (CHANNELS + [2, 6])[seed % 11]  # every channel count occurs whatever the draw
        kpool = {"g sweep": [2], "tap shifts": [1, 2, 4], "prefetch depth": PREFETCH_KERNELS, "staged block": [4, 5, 6, 7, 22, 23],
                 "conv head": [2, 3], "mixed": [1, 2, 3, 4, 5, 6, 7, 15, 22, 23]}[family]
        layers = []
        for _ in range(n):
            nl = int(rng.integers(1, 5))
            ks = [int(rng.choice(kpool)) for _ in range(nl)]
            ds = [int(rng.choice([d for d in SHIFT_DILATIONS + [2, 7] if (k - 1) * d <= MAX_REACH])) for k in ks]
            layers.append((ks, ds))
        head_kernel = int(rng.choice([2, 16, 17, 18, 33])) if family == "conv head" or (family == "mixed" and rng.integers(0, 3) == 0) else 1
        bias = [bool(rng.integers(0, 2)) for _ in range(n)]
        arrays = chain(channels, layers, _act(int(rng.integers(0, 2))), bias, head_kernel)
        lands = head_kernel > 1 or any(k != 3 for ks, _ in layers for k in ks)
        if lands and work(arrays) <= WORK_CAP:
            break
    sizes, left = [1, 1, 17, 300], SAMPLES - 319  # (one size above 128 whatever the draw: the host cuts it)
    while left > 0:
        c = min(int(rng.choice(CALL_SIZES)), left)
        sizes.append(c)
        left -= c
    return _case("fuzz-%d" % seed, family, "seeded draw", arrays, 500 + seed), sizes


# ---- the batch tests' models (tests/test_gpu_frame.py b .. e)

def small_k2_model():
    """8 channels, K = 2: the two-streams-per-workgroup and shadow-wave test"""
    return _case("spb-k2-c8", "batch", "Launch<2, 1, 2>, shadow wave", chain([8], [([2, 2], [1, 65])], O.ACT_TANH), 400)


def table_models():
    """the two models of the index-table test"""
    return [_case("table-c5", "batch", "slots / rows tables", chain([5], [([2, 4], [1, 64])], O.ACT_TANH), 410),
            _case("table-c12-head", "batch", "slots / rows tables", chain([12], [([2], [3])], O.ACT_LEAKYRELU, head_bias=[True], head_kernel=17), 411)]


def fused_models():
    """Nine different frame models of one batch: launches of eight groups plus one.  maxKsize differs per group inside the first launch
    (3 in an A1-shaped model, 6 at two channels and 15 at eight: HPF_WIDE beside HPF_NARROW groups); its largest staged block (16 channels,
    K = 7: 524 float4, above the stager's 512 at any workgroup shape) belongs to one group and sizes the LDS of all."""
    a1 = chain([16, 8], [([3, 3, 3, 3], [1, 2, 64, 128]), ([3, 3], [2, 128])], O.ACT_TANH, head_kernel=2)
    return [_case("fused-k3-c16-8", "batch", "K = 3 everywhere (here for its two-tap conv head)", a1, 420),
            _case("fused-k6-c2", "batch", "K = 6, two channels", chain([2], [([6, 6], [1, 7])], O.ACT_LEAKYRELU), 421),
            _case("fused-k15-c8", "batch", "K = 15, eight channels", chain([8], [([15, 2], [1, 63])], O.ACT_LEAKYRELU), 422),
            _case("fused-head-c10", "batch", "conv head", chain([10], [([2, 3], [1, 2])], O.ACT_TANH, head_bias=[True], head_kernel=18), 423),
            _case("fused-k7-c16", "batch", "staged block of 524 float4", chain([16], [([7, 2], [1, 5])], O.ACT_TANH), 424),
            _case("fused-c13-3", "batch", "two arrays, G 4 -> 1", chain([13, 3], [([2, 2], [1, 3]), ([2], [129])], O.ACT_TANH), 425),
            _case("fused-c1", "batch", "one channel", chain([1], [([2, 4], [1, 65])], O.ACT_TANH), 426),
            _case("fused-c5-k1", "batch", "K = 1 layer", chain([5], [([2, 1, 2], [64, 7, 1])], O.ACT_LEAKYRELU), 427),
            _case("fused-c12", "batch", "the ninth group: a launch of its own", chain([12], [([4, 2], [127, 1])], O.ACT_TANH), 428)]


def lds_model(ksize):
    """16 channels, one layer of kernel size `ksize`, d = 1: the LDS limit (frame_lds.h).  K = 62 / 63: 162176 / 164224 bytes at two
    streams per workgroup; K = 70 / 71: the same two figures at one."""
    return _case("lds-k%d" % ksize, "lds limit", "staged block of %d float4" % layer_block_f4(ksize, 16), chain([16], [([ksize], [1])], O.ACT_TANH), 430 + ksize)
