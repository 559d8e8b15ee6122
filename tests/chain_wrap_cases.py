"""Batches that take every compiled WaveNet chain instantiation past its ring wraps -- TEST INFRASTRUCTURE ONLY.

Shared by tests/test_gpu_chain_wraps.py (which runs the cases on the device), tests/test_chain_wraps_cpu.py (which proves without a GPU
that every sequence is long enough, that every case lands on the instantiation it names, that the cases together reach every chain
instantiation the launch switches hold, and that the oracle notices a long tap that is one frame off) and the table-launch cases of
tests/test_gpu_batch.py.  Pure Python and numpy, seeded, never skips.

A chain instantiation is WaveNetSpecKernel<family, NF, SPB, PK, NT> (wavenet_spec_impl.h LaunchChain and its callers in the Lite and A2
translation units): a separately compiled body with its own register allocation, wave-to-frame mapping and ring addressing.  A case is a
batch (model groups and stream counts), a block sequence and, per block length the chains take, the instantiation (chain, NF, SPB, PK)
the launch must land on.  The stream counts leave a partial last workgroup and, in a pack, a partly filled last virtual stream.

Which launch a batch makes.  WaveNetLaunchFor decides per LAUNCH.  A host-buffer call of 512 or more kernel-level streams runs as two
half-batch launches of half the streams each (gpu_batch_chains.cpp PrepareHalves), so Standard x 515 through Batch.Process is two launches
of 258 and 257 streams, both at SPB = 1.  The cases therefore go through ProcessDevice on a stream the caller owns (host_route.h
DeviceOrdered): ONE launch of all the groups, which is what predict() asks NA_DebugWaveNetLaunch about.

Which instantiations default knobs reach.  Packed Nano is the dense 16 / 8 pack by default (wavenet_choice.h "Dense packs"), a LITE
architecture: the one-tile-per-wave chain (Lite16T1) takes launches of 16 / 16 virtual streams only, which exist under NA_WN_DENSE=0.  The
tuning knobs are read once per process, so the Lite16T1 cases name that knob and the GPU test runs them in a child process.

A2 and the Infinity Cache.  A stream of the A2 container owns state in both submodels (about 460 KB), so 1030 of them are beyond the 400 MiB
from which 128-frame launches at SPB = 2 take the non-temporal variant.  The SPB = 2 case of A2 is 810 streams (372 MB): halfGroups =
ceil(405 / 2) + 405 = 608 > 2 x 256 CUs, 405 three-channel streams leave one of four slots of the last workgroup filled, 405 eight-channel
streams one of two.  The one launch of Lite + Feather + Nano keeps the same distance from that threshold with 515 + 1029 + 1031 streams
(1288 virtual streams: SPB = 2; an odd Lite count, a half-filled Feather pack, a Nano pack with three of four streams).  The GPU test
asserts the state size it assumed.  The non-temporal variants are run by the child-process test of tests/test_gpu_chain_wraps.py."""
import os

import numpy as np

import na_oracle as O

TOL_RMS = 2e-6              # the project's bound of a chain against the C oracle (tests/test_gpu_spec.py)
CONTROL_FACTOR = 100.0      # the suite's control convention (tests/test_gpu_snapshot.py CONTROL_RMS)
LATE = 1024                 # the window behind the wraps: every long tap reads frames the kernel stored itself
BLOCK = 128
BASE_ROWS = 9               # seeded noise rows, repeated over the streams
CUS = 256                   # MI355X
NT_STATE_BYTES = 400 << 20  # tuning.h wnNtFromMB: stream state from which a batch is "beyond the cache"

# csrc/wavenet_launch_choice.h WnLaunchKernel, WnChain and csrc/wavenet_dev.h WnSpecArch, as tests/test_wavenet_dispatch_cpu.py names them
K_CHAIN, K_TABLE, K_INTERPRETER = 1, 2, 3
CH_STD, CH_LITE, CH_LITE_PACKED, CH_LITE16T1, CH_A2 = range(5)
CHAIN_NAMES = ("Std", "Lite", "LitePacked", "Lite16T1", "A2")
SPEC_NONE, SPEC_STD, SPEC_LITE, SPEC_LITE16, SPEC_A2FULL, SPEC_A2LITE = range(6)
CHAIN_LENGTHS = (128, 64, 32)

# Every chain instantiation without the NT bit, (chain, NF, SPB, PK), written out from the switches:
#   wavenet_spec_impl.h LaunchChain<F, PK>: SPB 2 at 128 / 64 and, where every member runs one or two tiles per wave, 32; SPB 1 the same
#   unless the family runs one tile per wave;
#   wavenet_spec_kernels.hip: FamStd, PK false;  wavenet_spec_lite_kernels.hip LaunchSpecLite: FamLite16T1 and FamLitePacked with PK true,
#   FamLite with PK false;  wavenet_spec_a2_kernels.hip LaunchSpecA2: FamA2 (a four-tile member: no 32-frame body), PK false.
INSTANTIATIONS = [
    (CH_STD, 128, 2, 0), (CH_STD, 64, 2, 0), (CH_STD, 32, 2, 0), (CH_STD, 128, 1, 0), (CH_STD, 64, 1, 0), (CH_STD, 32, 1, 0),
    (CH_LITE, 128, 2, 0), (CH_LITE, 64, 2, 0), (CH_LITE, 32, 2, 0), (CH_LITE, 128, 1, 0), (CH_LITE, 64, 1, 0), (CH_LITE, 32, 1, 0),
    (CH_LITE_PACKED, 128, 2, 1), (CH_LITE_PACKED, 64, 2, 1), (CH_LITE_PACKED, 32, 2, 1),
    (CH_LITE_PACKED, 128, 1, 1), (CH_LITE_PACKED, 64, 1, 1), (CH_LITE_PACKED, 32, 1, 1),
    (CH_LITE16T1, 128, 2, 1), (CH_LITE16T1, 64, 2, 1), (CH_LITE16T1, 32, 2, 1),
    (CH_A2, 128, 2, 0), (CH_A2, 64, 2, 0), (CH_A2, 128, 1, 0), (CH_A2, 64, 1, 0),
]

# The members of a launch, as sorted (spec arch, pack) of its groups, that each chain family is run with: a body is compiled per family, and
# a family's members (its two architectures, its pack factors) take different paths through it.  The one launch of three lite-family
# groups exists at SPB = 2 only (its 1288 virtual streams are the point of it).
SIG_STD, SIG_LITE, SIG_FEATHER, SIG_NANO, SIG_NANO16 = ((SPEC_STD, 1),), ((SPEC_LITE, 1),), ((SPEC_LITE, 2),), ((SPEC_LITE, 4),), ((SPEC_LITE16, 4),)
SIG_A2 = ((SPEC_A2FULL, 1), (SPEC_A2LITE, 1))
SIG_THREE = ((SPEC_LITE, 1), (SPEC_LITE, 2), (SPEC_LITE, 4))
MEMBERS = {CH_STD: [SIG_STD], CH_LITE: [SIG_LITE], CH_LITE_PACKED: [SIG_FEATHER, SIG_NANO, SIG_THREE], CH_LITE16T1: [SIG_NANO16], CH_A2: [SIG_A2]}
# what the cases must reach: (instantiation, members, "pure" | "mixed") -- in a sequence of that one block length, and in the mixed one
REQUIRED = [(inst, sig, kind) for inst in INSTANTIATIONS for sig in MEMBERS[inst[0]] if not (sig == SIG_THREE and inst[2] == 1) for kind in ("pure", "mixed")]

MIXED = [128, 37, 64, 100, 32, 128, 1, 64, 128, 128]
SEQUENCES = {"128": [128] * 22, "64": [64] * 44, "32": [32] * 88, "mixed": MIXED * 4}
SEQUENCE_SEEDS = {"128": 101, "64": 102, "32": 103, "mixed": 104}

MODEL_FILES = {"standard": "BossWN-standard.nam", "feather": "BossWN-feather.nam", "nano": "BossWN-nano.nam", "a2": "BossWN-a2.nam"}
LITE_SEED = 33              # the synthetic A1 Lite 12 / 6 of tests/test_gpu_spec.py _lite
A2_QUALITIES = (0.0, 1.0, 0.3, 0.9)  # as tests/test_gpu_spec.py splits an A2 batch: both submodels, two AddStreams calls each


def _split4(streams):
    return [streams // 4 + (1 if k < streams % 4 else 0) for k in range(4)]


def _batch(model, streams):
    """[(model, quality, streams)] in AddStreams order"""
    if model == "a2":
        return [("a2", q, c) for q, c in zip(A2_QUALITIES, _split4(streams))]
    return [(model, 1.0, streams)]


# (name, batch, family, SPB, PK, knobs): the regime the batch is there for
_REGIMES = [
    ("std-3", _batch("standard", 3), CH_STD, 1, 0, {}),
    ("std-515", _batch("standard", 515), CH_STD, 2, 0, {}),
    ("lite-3", _batch("lite", 3), CH_LITE, 1, 0, {}),
    ("lite-513", _batch("lite", 513), CH_LITE, 2, 0, {}),
    ("feather-5", _batch("feather", 5), CH_LITE_PACKED, 1, 1, {}),
    ("feather-1029", _batch("feather", 1029), CH_LITE_PACKED, 2, 1, {}),
    ("nano-1031", _batch("nano", 1031), CH_LITE_PACKED, 1, 1, {}),      # two tiles per wave: 258 virtual streams, at most two workgroups per CU
    ("nano-2057", _batch("nano", 2057), CH_LITE_PACKED, 2, 1, {}),      # 515 virtual streams, the last one holds one real stream
    ("nano16-6", _batch("nano", 6), CH_LITE16T1, 2, 1, {"NA_WN_DENSE": 0}),  # one tile per wave: two 16 / 16 virtual streams, the second half filled
    ("a2-5", _batch("a2", 5), CH_A2, 1, 0, {}),
    ("a2-810", _batch("a2", 810), CH_A2, 2, 0, {}),
    ("lite-feather-nano", [("lite", 1.0, 515), ("feather", 1.0, 1029), ("nano", 1.0, 1031)], CH_LITE_PACKED, 2, 1, {}),  # one launch, packs 1 / 2 / 4
]


def _lengths(family, seq):
    return [n for n in CHAIN_LENGTHS if n in SEQUENCES[seq] and not (family == CH_A2 and n == 32)]


def cases():
    """Every regime with every block sequence its family has a chain for.  expect: per chain block length of the sequence the
    instantiation (chain, NF, SPB, PK); every other length of the sequence runs the stage interpreter."""
    out = []
    for name, batch, family, spb, pk, knobs in _REGIMES:
        for seq in SEQUENCES:
            lengths = _lengths(family, seq)
            if seq != "mixed" and not lengths:
                continue  # (A2 has no 32-frame chain)
            out.append(dict(name="%s-%s" % (name, seq), regime=name, batch=batch, seq=seq, knobs=dict(knobs),
                            expect={n: (family, n, spb, pk) for n in lengths}))
    return out


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


def num_streams(case):
    return sum(c for _, _, c in case["batch"])


# ---- models and oracles ---------------------------------------------------------------------------------------------------------------
def lite_arrays_weights():
    arrays = O.a1_arrays(12, 6)
    return arrays, O.synth_wavenet_weights(arrays, seed=LITE_SEED)


def load(loader, model):
    if model == "lite":
        arrays, w = lite_arrays_weights()
        return loader.CreateFromString(O.nam_json_wavenet_a1(12, 6, w), ".nam", doPrewarm=False)
    return loader.CreateFromFile(os.path.join(O.MODELS_DIR, MODEL_FILES[model]), doPrewarm=False)


def submodel(model, quality):
    """the member of the A2 container a quality selects (0 for every other model)"""
    return O.quality_to_submodel(O.load_json(MODEL_FILES["a2"]), quality) if model == "a2" else 0


def oracle(model, quality=1.0):
    if model == "lite":
        return O.OracleWaveNet(*lite_arrays_weights())
    return O.oracle_from_file(MODEL_FILES[model], quality=quality)


def longest_ring(arrays):
    """An upper bound of every history ring of a model in any state format: the padded history plus a block (the bound
    tests/test_gpu_stdmath.py _longest_ring uses).  1152 for A1, 1328 for A2."""
    reach = max([(k - 1) * d for a in arrays for k, d in zip(a["kernel_sizes"], a["dilations"])] +
                [(a["head_kernel_size"] - 1) * a["head_dilation"] for a in arrays])
    return (reach + 15) // 16 * 16 + BLOCK


def off_by_one_oracle(ora):
    """The oracle of the same weights with the dilation of the layer of the longest reach (the last of them: the A1 architectures have
    a d = 512 layer in both arrays) lowered by one: what a chain body computes whose longest tap reads one frame too late.  The weight
    shapes do not change."""
    arrays = [dict(a, dilations=list(a["dilations"]), kernel_sizes=list(a["kernel_sizes"])) for a in ora.arrays]
    _, ai, li = max(((k - 1) * d, i, j) for i, a in enumerate(arrays) for j, (k, d) in enumerate(zip(a["kernel_sizes"], a["dilations"])))
    arrays[ai]["dilations"][li] -= 1
    return O.OracleWaveNet(arrays, ora.weights)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def base_rows(seq):
    """BASE_ROWS rows of clipped noise for a sequence; stream s of every case is fed row s % BASE_ROWS"""
    rng = np.random.default_rng(SEQUENCE_SEEDS[seq])
    return (0.3 * rng.standard_normal((BASE_ROWS, sum(SEQUENCES[seq])))).clip(-1, 1).astype(np.float32)


def group_ranges(case):
    """[(model, quality, first stream, count)]"""
    out, first = [], 0
    for model, quality, count in case["batch"]:
        out.append((model, quality, first, count))
        first += count
    return out


def picks(case):
    """The streams held to the oracle, [(stream, model, quality)]: of every AddStreams call the first stream, the last one and one at an
    odd position in the middle -- inside a pack and, at SPB = 2, the second stream of a workgroup."""
    out = []
    for model, quality, first, count in group_ranges(case):
        for s in sorted({0, min(count - 1, (count // 2) | 1), count - 1}):
            out.append((first + s, model, quality))
    return out


# ---- the prediction -------------------------------------------------------------------------------------------------------------------
def launch_groups(na, models, batch, knobs=()):
    """The group facts of the ONE launch a batch makes (NA_DebugWaveNetLaunch): one group per model description -- the two AddStreams
    calls that select the same A2 submodel share it --, packed groups count virtual streams, and in a packed launch every group passes
    its index lists (launch_plan.h).  models: {model: handle}."""
    merged = {}
    for model, quality, count in batch:
        key = (model, submodel(model, quality))
        merged.setdefault(key, [quality, 0])[1] += count
    facts = []
    for (model, _), (quality, count) in merged.items():
        k = na.wavenet_kernel(models[model], count, quality, knobs)
        assert k["family"] == "f16-split", (model, k)
        facts.append((k["spec_arch"], k["pack"], 0 if k["spec_arch"] in (SPEC_A2FULL, SPEC_A2LITE) else 2, -(-count // k["pack"])))
    packed = any(f[1] > 1 for f in facts)
    return [f + (int(packed), 2048) for f in facts]


def predict(na, models, batch, n, cus=CUS, beyond_cache=False, knobs=()):
    """(kernel, chain, NF, SPB, PK, NT) of the launch of n frames"""
    r = na.wavenet_launch(launch_groups(na, models, batch, knobs), n, cus=cus, beyond_cache=beyond_cache, knobs=knobs)
    assert r[1] == 0, r
    return (r[0], r[2], r[3], r[4], r[9], r[5])


def signature(groups):
    """sorted (spec arch, pack) of the groups of a launch"""
    return tuple(sorted((g[0], g[1]) for g in groups))


def instantiation_name(inst):
    chain, nf, spb, pk = inst
    return "WaveNetSpecKernel<Fam%s, %d, %d, %s>" % (CHAIN_NAMES[chain], nf, spb, "true" if pk else "false")


# ---- table launches (tests/test_gpu_batch.py) ------------------------------------------------------------------------------------------
# More than eight model groups of one family run as ONE launch of WaveNetSpecTableKernel<family, NF, SPB, PK> at 128 / 64 frames
# (wavenet_launch_choice.h TableFor).  Workgroup size: SPB = 1 where more than a quarter of the full-size workgroups' stream slots would
# idle.  One stream per handle: SPB = 1.  Standard x 5: 6 slots for 5 streams, SPB = 2 with a half-filled last workgroup per group;
# Feather x 3 and Nano x 5: two virtual streams, the second partly filled; A2 x 7: the three-channel groups fill 7 of 8 slots, the
# eight-channel groups 7 of 8.  (model, handles, streams per handle, chain, SPB, PK)
TABLE_HANDLES = 9
TABLE_CASES = [("standard", 1, CH_STD, 1, 0), ("standard", 5, CH_STD, 2, 0), ("feather", 1, CH_LITE_PACKED, 1, 1), ("feather", 3, CH_LITE_PACKED, 2, 1),
               ("nano", 1, CH_LITE_PACKED, 1, 1), ("nano", 5, CH_LITE_PACKED, 2, 1), ("a2", 1, CH_A2, 1, 0), ("a2", 7, CH_A2, 2, 0)]
TABLE_SEQUENCES = ("128", "64")


def table_quality(model, handle):
    """A2: both submodels of the container, handle by handle (the last handle runs the eight-channel one)"""
    return (1.0 if handle % 2 == 0 else 0.2) if model == "a2" else 1.0


def table_groups(na, handle, model, per):
    """the group facts of the table launch of TABLE_HANDLES handles of one file with `per` streams each"""
    facts = []
    for i in range(TABLE_HANDLES):
        k = na.wavenet_kernel(handle, per, table_quality(model, i))
        facts.append((k["spec_arch"], k["pack"], 0 if k["spec_arch"] in (SPEC_A2FULL, SPEC_A2LITE) else 2, -(-per // k["pack"])))
    packed = any(f[1] > 1 for f in facts)
    return [f + (int(packed), 2048) for f in facts]
