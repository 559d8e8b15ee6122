"""Which kernel runs a WaveNet model (csrc/wavenet_choice.h WaveNetKernelFor / WaveNetLaunchFor through NA_DebugWaveNetKernel /
NA_DebugWaveNetLaunch), without a GPU.

What a model group decides once -- family, pack, input limit, range proof -- is compared with the values the library gave before the
decision moved into one function (tests/golden/wavenet_choice_grid.npz: `python tests/test_wavenet_dispatch_cpu.py FILE` records the grid,
through NA_ModelKernelInfo and NA_DebugPackedWeights, from whatever build of the package is first on the path, one fresh child process per
knob set because the tuning knobs are parsed once per process; the file in the tree is from the commit before WaveNetKernelFor).

What one launch decides is restated below in Python from the launch cascades the function replaced (LaunchWaveNetSplitFused,
LaunchWaveNetSpecFused + LaunchNF + LaunchSpecLite / LaunchSpecA2, LaunchWaveNetSpecTable, LaunchWaveNetFrameFused and the list launch of
GpuBatch::LaunchWaveNetList), step by step as they tried their kernels, and compared with the library over a grid that crosses every
edge in those functions."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import frame_cases as FC
import na_oracle as O
import split_cases as SC
import wide_cases as WC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wavenet_choice_grid.npz")
GROUP_KNOB_SETS = [dict(), dict(NA_WN_KERNEL="split"), dict(NA_WN_KERNEL="frame"), dict(NA_WN_KERNEL="generic"), dict(NA_WN_PACK=0), dict(NA_WN_PAD=0),
                   dict(NA_WN_DENSE=0)]
GROUP_KNOB_NAMES = ("NA_WN_KERNEL", "NA_WN_PACK", "NA_WN_PAD", "NA_WN_DENSE")
STREAMS = (1, 2048)
QUALITIES = (0.0, 1.0)  # (a slimmable container: its smallest and its largest submodel; every other model ignores it)
FAMILIES = ["recurrent", "f16-split", "frame", "generic"]


# ---- the grid of models -------------------------------------------------------------------------------------------------------------------
def grid_models():
    """[(name, file name or None, arrays, weights)]: every file under tests/golden/models (the A2 file is a slimmable container), every model
    of split_cases.py and frame_cases.py, the wide-channel shapes tests/test_gpu_wide.py builds"""
    models = [(f, f, None, None) for f in sorted(os.listdir(O.MODELS_DIR)) if f.endswith((".nam", ".json"))]
    split = SC.named_cases() + [SC.fuzz_case(s)[0] for s in range(SC.NUM_FUZZ_SEEDS)] + SC.batch_models()
    models += [("split:" + c["name"], None, c["arrays"], SC.weights(c)) for c in split]
    models += [("split-edge:" + name, None, arrays, O.synth_wavenet_weights(arrays, seed=seed)) for name, arrays, seed in SC.decision_edges()]
    frame = FC.named_cases() + [FC.fuzz_case(s)[0] for s in range(FC.NUM_FUZZ_SEEDS)] + [FC.small_k2_model()] + FC.table_models() + FC.fused_models() + \
        [FC.lds_model(k) for k in (62, 63, 70)]
    models += [("frame:" + c["name"], None, c["arrays"], FC.weights(c)) for c in frame]
    wide = [("-".join(map(str, ch)), WC.fixed_case(ch, act)) for ch, act in WC.FIXED_CASES] + \
        [("chain-%d" % c, WC.chain([c], [([3, 3], [1, 64])])) for c in (24, 32)] + [("chain-65", WC.chain([65], [([3], [1])]))] + \
        [("two-%d" % c, WC.two_array(c, c // 2)) for c in (40, 96)]
    models += [("wide:" + name, None, arrays, O.synth_wavenet_weights(arrays, seed=sum(a["channels"] for a in arrays))) for name, arrays in wide]
    models += [("wide-range:" + name, None) + WC.range_model(name) for name in WC.RANGE_MODELS]
    return models


def load(loader, model):
    name, file, arrays, w = model
    if file:
        return loader.CreateFromFile(os.path.join(O.MODELS_DIR, file), doPrewarm=False)
    return loader.CreateFromString(O.nam_json_wavenet_generic(arrays, w), ".nam", doPrewarm=False)


def packed_count(na, m):
    """(weights of the packed virtual model, pack factor) of NA_DebugPackedWeights"""
    import ctypes as C
    pf = C.c_int(0)
    n = na.capi.load_library().NA_DebugPackedWeights(m._h, C.byref(pf), None, 0)
    return n, pf.value


def record_own_knobs(na):
    """int32 [model][streams][quality][family, pack, range proven, weights ok, input limit bits] and [model][packed weights, pack factor],
    under the process's own knobs, from entry points the library has had all along"""
    loader = na.NeuralModelLoader()
    models = grid_models()
    info = np.zeros((len(models), len(STREAMS), len(QUALITIES), 5), np.int32)
    packed = np.zeros((len(models), 2), np.int32)
    for i, model in enumerate(models):
        m = load(loader, model)
        assert m is not None, model[0]
        for s, streams in enumerate(STREAMS):
            for q, quality in enumerate(QUALITIES):
                k = m.KernelInfo(quality, streams)
                limit = int(np.float32(k["input_limit"]).view(np.int32))
                info[i, s, q] = [FAMILIES.index(k["kernel"]), k["pack"], k["range_proven"], k["weights_ok"], limit]
        packed[i] = packed_count(na, m)
    return info, packed


def knob_env(knobs):
    env = {k: v for k, v in os.environ.items() if not k.startswith("NA_")}
    env.update({k: str(v) for k, v in knobs.items()})
    return env


def record(path):
    """One child per knob set (this file with --child prints its grid as JSON)"""
    infos, packs = [], []
    for knobs in GROUP_KNOB_SETS:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=knob_env(knobs), check=True, capture_output=True, text=True).stdout
        got = json.loads(out.splitlines()[-1])
        infos.append(np.array(got["info"], np.int32))
        packs.append(np.array(got["packed"], np.int32))
    np.savez_compressed(path, names=np.array([m[0] for m in grid_models()]), info=np.stack(infos), packed=np.stack(packs))


# ---- the parent's launch cascades, restated -------------------------------------------------------------------------------------------
INVALID, NOT_SUPPORTED = 1, 801  # hipErrorInvalidValue, hipErrorNotSupported
NONE, STD, LITE, LITE16, A2FULL, A2LITE = range(6)
MAX_GROUPS, MAX_FRAMES, LDS_LIMIT = 8, 128, 160 * 1024
# group facts: (spec_arch, pack, split_fast_T, streams, has_lists, max_a4_floats, max_G, max_split_ops)
ARCH, PACK, FAST_T, NSTREAMS, LISTS, MAX_A4, MAX_G, MAX_OPS = range(8)
# results, as NA_DebugWaveNetLaunch reports them: (kernel, error, chain, NF, SPB, NT, T, WPS, GEN, PK, PF)
K_NONE, K_CHAIN, K_TABLE, K_INTERPRETER, K_FRAME, K_PIECES = range(6)
CH_STD, CH_LITE, CH_LITE_PACKED, CH_LITE16T1, CH_A2 = range(5)
# tiles per wave of the two members of a chain family (wavenet_spec_impl.h FamStd .. FamLite16T1)
FAMILY_TILES = {CH_STD: (2, 2), CH_LITE: (2, 2), CH_LITE_PACKED: (2, 2), CH_A2: (2, 4), CH_LITE16T1: (1, 1)}


def refused(error):
    return (K_NONE, error) + (0,) * 9


def chain(kernel, member, nf, spb, pk, nt=0):
    return (kernel, 0, member, nf, spb, nt, 0, 0, 0, int(pk), 0)


def spec_on(knobs):
    return not (knobs.get("NA_WN_SPEC") == 0 or "NA_SP_T" in knobs or "NA_SP_GEN" in knobs)


def launch_nf(member, pk, n, spb, beyond):
    """spk::LaunchNF<F, PK>"""
    t0, t1 = FAMILY_TILES[member]
    if t0 != 1 and beyond and n == 128 and spb >= 2:
        return chain(K_CHAIN, member, 128, 2, pk, 1)
    if t0 == 1:
        return chain(K_CHAIN, member, n, 2, pk)
    if n in (128, 64):
        return chain(K_CHAIN, member, n, 2 if spb >= 2 else 1, pk)
    if t0 == 2 and t1 == 2:
        return chain(K_CHAIN, member, 32, 2 if spb >= 2 else 1, pk)
    return NOT_SUPPORTED


def spec_fused(groups, n, sharing, beyond, cus, knobs):
    """LaunchWaveNetSpecFused, LaunchSpecLite, LaunchSpecA2"""
    if len(groups) <= 0 or len(groups) > MAX_GROUPS or n not in (128, 64, 32):
        return NOT_SUPPORTED
    if not spec_on(knobs):
        return NOT_SUPPORTED
    arch = groups[0][ARCH]
    if arch == NONE:
        return NOT_SUPPORTED
    family_of = lambda a: 1 if a in (LITE, LITE16) else (2 if a in (A2FULL, A2LITE) else 0)
    fam = family_of(arch)
    packed = lite16 = False
    for g in groups:
        a = g[ARCH]
        if g[NSTREAMS] <= 0 or a == NONE or family_of(a) != fam or (fam == 0 and a != arch):
            return NOT_SUPPORTED
        packed = packed or g[PACK] > 1
        lite16 = lite16 or a == LITE16
    if packed and any(not g[LISTS] for g in groups):
        return NOT_SUPPORTED
    spb_env = knobs.get("NA_SP_SPB", 0)
    half_groups = sum((g[NSTREAMS] + (2 if g[ARCH] == A2LITE else 1) - 1) // (2 if g[ARCH] == A2LITE else 1) for g in groups)
    spb = spb_env if spb_env > 0 else (2 if half_groups * max(sharing, 1) > 2 * cus else 1)
    if fam == 0:
        return NOT_SUPPORTED if packed else launch_nf(CH_STD, False, n, spb, beyond)
    if fam == 2:
        return NOT_SUPPORTED if packed else launch_nf(CH_A2, False, n, spb, beyond)
    if not packed and lite16:
        return NOT_SUPPORTED
    all16 = packed and "NA_SP_NO_T1" not in knobs and all(g[ARCH] == LITE16 for g in groups)
    t1 = all16 and spb_env == 0 and sum(g[NSTREAMS] for g in groups) <= cus
    if packed and t1:
        return launch_nf(CH_LITE16T1, True, n, 2, False)
    if packed:
        return launch_nf(CH_LITE_PACKED, True, n, spb, beyond)
    return launch_nf(CH_LITE, False, n, spb, beyond)


def split_lds(spb, pk, max_g, max_ops):
    """sp::Launch: block images, planes of 16 + 128 quads, two weight buffers"""
    return (spb * 4 * 128 * 8 if pk else spb * 128 * 16) + spb * 2 * max_g * 144 * 16 + 2 * max_ops * 64 * 16 + 1024


def sp_launch(groups, t, spb, wps, gen, pk):
    """sp::Launch<T, SPB, WPS, GEN, PK>"""
    for g in groups:
        if g[PACK] > 1 and not pk:
            return refused(INVALID)
        if pk and not g[LISTS]:
            return refused(INVALID)
    if split_lds(spb, pk, max([1] + [g[MAX_G] for g in groups]), max([16] + [g[MAX_OPS] for g in groups])) > LDS_LIMIT:
        return refused(INVALID)
    return (K_INTERPRETER, 0, 0, 0, spb, 0, t, wps, int(gen), int(pk), 0)


def split_fused(groups, n, sharing, beyond, cus, knobs):
    """LaunchWaveNetSplitFused"""
    if n <= 0 or len(groups) <= 0:
        return refused(0)
    if n > MAX_FRAMES or len(groups) > MAX_GROUPS:
        return refused(INVALID)
    e = spec_fused(groups, n, sharing, beyond, cus, knobs)
    if e != NOT_SUPPORTED:
        return e
    total = 0
    for g in groups:
        if g[NSTREAMS] <= 0:
            return refused(INVALID)
        total += g[NSTREAMS]
    t_env, spb_env, gen = knobs.get("NA_SP_T", 0), knobs.get("NA_SP_SPB", 0), "NA_SP_GEN" in knobs
    spb = spb_env if spb_env > 0 else (2 if total >= 512 else 1)
    tiles = (n + 15) // 16
    t = t_env if t_env in (2, 4) else 2
    for g in groups:
        if g[FAST_T] == 0:
            gen = True
        else:
            t = max(t, g[FAST_T])
    if any(g[PACK] > 1 for g in groups):
        if any(g[FAST_T] != 2 for g in groups):
            return refused(INVALID)
        if tiles > 4:
            return sp_launch(groups, 2, 2 if spb >= 2 else 1, 4, False, True)
        if tiles > 2:
            return sp_launch(groups, 2, 2 if spb >= 2 else 1, 2, False, True)
        return sp_launch(groups, 2, 2 if spb >= 2 else 1, 1, False, True)
    if t == 4:
        if tiles > 4:
            return sp_launch(groups, 4, 2 if spb >= 2 else 1, 2, gen, False)
        return sp_launch(groups, 4, 2 if spb >= 2 else 1, 1, gen, False)
    if tiles > 4:
        return sp_launch(groups, 2, 4 if spb >= 4 else (2 if spb >= 2 else 1), 4, gen, False)
    if tiles > 2:
        return sp_launch(groups, 2, 2 if spb >= 2 else 1, 2, gen, False)
    return sp_launch(groups, 2, 2 if spb >= 2 else 1, 1, gen, False)


def spec_table(groups, n, knobs):
    """LaunchWaveNetSpecTable, LaunchSpecLiteTable, LaunchSpecA2Table"""
    if len(groups) <= MAX_GROUPS or n not in (128, 64) or not spec_on(knobs) or knobs.get("NA_SP_SPB", 0) > 0:
        return NOT_SUPPORTED
    arch = groups[0][ARCH]
    lite, a2 = arch in (LITE, LITE16), arch in (A2FULL, A2LITE)
    if arch != STD and not lite and not a2:
        return NOT_SUPPORTED
    packed, streams, slots2 = False, 0, 0
    for g in groups:
        a = g[ARCH]
        same = a in (LITE, LITE16) if lite else (a in (A2FULL, A2LITE) if a2 else a == STD)
        if g[NSTREAMS] <= 0 or not same:
            return NOT_SUPPORTED
        packed = packed or g[PACK] > 1
        per2 = 4 if a == A2LITE else 2
        streams += g[NSTREAMS]
        slots2 += (g[NSTREAMS] + per2 - 1) // per2 * per2
    if not lite and packed:
        return NOT_SUPPORTED
    if packed and any(not g[LISTS] for g in groups):
        return NOT_SUPPORTED
    if not packed and any(g[ARCH] == LITE16 for g in groups):
        return NOT_SUPPORTED
    spb = 1 if slots2 * 4 > streams * 5 else 2
    if a2:
        return chain(K_TABLE, CH_A2, n, spb, False)
    if not lite:
        return chain(K_TABLE, CH_STD, n, spb, False)
    return chain(K_TABLE, CH_LITE_PACKED if packed else CH_LITE, n, spb, packed)


def frame_lds(a4, wps, spb, pf):
    """frame_lds.h FrameLaunchLdsBytes"""
    nw = wps * spb
    stride = max((384 + 64 * nw - 1) // (64 * nw) * 64 * nw, (a4 + 3) // 4)
    return spb * 2 * wps * 4 * 64 * 16 + 2 * stride * 16 + (nw * 2 * 4 * 64 * 16 if pf == 2 else 0)


def frame_fits(a4, wps, spb, pf):
    return frame_lds(a4, wps, spb, pf) <= LDS_LIMIT


def fr_launch(groups, wps, pf, spb):
    """fr::Launch<WPS, PF, SPB>"""
    if not frame_fits(max([0] + [g[MAX_A4] for g in groups]), wps, spb, pf):
        return refused(INVALID)
    return (K_FRAME, 0, 0, 0, spb, 0, 0, wps, 0, 0, pf)


def frame_fused(groups, n, knobs):
    """LaunchWaveNetFrameFused"""
    if n <= 0 or len(groups) <= 0:
        return refused(0)
    if n > MAX_FRAMES or len(groups) > MAX_GROUPS:
        return refused(INVALID)
    total = max_a4 = 0
    for g in groups:
        if g[NSTREAMS] <= 0:
            return refused(INVALID)
        total += g[NSTREAMS]
        max_a4 = max(max_a4, g[MAX_A4])
    prefetch, spb_env = knobs.get("NA_FR_PF", 1), knobs.get("NA_FR_SPB", 0)
    spb = spb_env if spb_env > 0 else (2 if total >= 512 else 1)
    if n > 64:
        if not prefetch:
            return fr_launch(groups, 2, 0, 1)
        if spb >= 4 and frame_fits(max_a4, 2, 4, 1):
            return fr_launch(groups, 2, 1, 4)
        if prefetch == 2:
            if spb >= 2 and frame_fits(max_a4, 2, 2, 2):
                return fr_launch(groups, 2, 2, 2)
            if frame_fits(max_a4, 2, 1, 2):
                return fr_launch(groups, 2, 2, 1)
        if spb >= 2 and frame_fits(max_a4, 2, 2, 1):
            return fr_launch(groups, 2, 1, 2)
        return fr_launch(groups, 2, 1, 1)
    return fr_launch(groups, 1, 0, 1)


def list_launch(frame, groups, n, sharing, beyond, cus, knobs):
    """One chunk of GpuBatch::LaunchWaveNetList: the launches it issued, in order"""
    if not frame and len(groups) > MAX_GROUPS:
        te = spec_table(groups, n, knobs)
        if te != NOT_SUPPORTED:
            return [te]
    pieces = [groups[i:i + MAX_GROUPS] for i in range(0, len(groups), MAX_GROUPS)]
    return [frame_fused(p, n, knobs) if frame else split_fused(p, n, sharing, beyond, cus, knobs) for p in pieces]


# ---- the grid of launches ---------------------------------------------------------------------------------------------------------------
BLOCKS = [1, 16, 17, 31, 32, 33, 48, 63, 64, 65, 80, 96, 127, 128]
CUS = [64, 256, 304]
LAUNCH_KNOB_SETS = [dict(), dict(NA_SP_T=2), dict(NA_SP_T=4), dict(NA_SP_SPB=1), dict(NA_SP_SPB=2), dict(NA_SP_SPB=4), dict(NA_SP_GEN=1), dict(NA_SP_NO_T1=1),
                    dict(NA_WN_SPEC=0), dict(NA_FR_PF=0), dict(NA_FR_PF=2), dict(NA_FR_SPB=1), dict(NA_FR_SPB=2), dict(NA_FR_SPB=4)]
# stream counts on both sides of 512 (total streams), of CUs (the one-tile rule) and of 2 CUs / sharing (half-size workgroups), for all CUS
COUNTS = [1, 3, 64, 65, 128, 129, 152, 153, 256, 257, 304, 305, 511, 512, 513, 608, 609]


def frame_fit_edges():
    """the largest max_a4_floats that fits and the first that does not, for every shape LaunchWaveNetFrameFused asks or launches"""
    edges = set()
    for wps, spb, pf in [(2, 4, 1), (2, 2, 2), (2, 1, 2), (2, 2, 1), (2, 1, 1), (2, 1, 0), (1, 1, 0)]:
        lo, hi = 0, 1 << 20
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if frame_fits(mid, wps, spb, pf) else (lo, mid)
        edges |= {lo, hi}
    return sorted(edges)


def group(arch, streams, pack=1, lists=None, fast=None, a4=2048, max_g=4, max_ops=16):
    fast = {NONE: 2, STD: 2, LITE: 2, LITE16: 2, A2FULL: 0, A2LITE: 0}[arch] if fast is None else fast
    return (arch, pack, fast, streams, int(pack > 1 if lists is None else lists), a4, max_g, max_ops)


def split_lists():
    lists = []
    for count in COUNTS:
        lists += [[group(STD, count)], [group(LITE, count)], [group(LITE, count, 2)], [group(LITE16, count, 4)], [group(A2FULL, count)], [group(A2LITE, count)],
                  [group(NONE, count)], [group(NONE, count, fast=4)], [group(NONE, count, fast=0)], [group(NONE, count, 2)], [group(NONE, count, 4)]]
    # what the launchers refuse or hand on: no index lists under a pack, 16 / 16 unpacked, a pack on a family that has none, a packed
    # group whose plan is not a fast one, no streams, an interpreter launch beyond the LDS
    lists += [[group(LITE, 8, 2, lists=0)], [group(LITE16, 8, 4, lists=0)], [group(LITE16, 8, 1)], [group(LITE16, 8, 1, lists=1)], [group(STD, 8, 2)], [group(A2FULL, 8, 2)],
              [group(NONE, 8, 2, fast=4)], [group(NONE, 8, 2, fast=0)], [group(NONE, 8, 2, lists=0)], [group(STD, 0)], [group(NONE, 0)], [group(STD, 5), group(STD, 0)],
              [group(NONE, 600, max_ops=39)], [group(NONE, 600, max_ops=40)], [group(NONE, 600, max_ops=75)], [group(NONE, 600, max_ops=76)],
              [group(NONE, 600, max_g=16)], [group(NONE, 8, 4, max_g=16, max_ops=40)]]
    # several groups: one family, mixed members of a family, mixed families, plain groups riding in a packed launch
    lists += [[group(STD, 200), group(STD, 57)], [group(STD, 300), group(STD, 212)], [group(LITE, 100), group(LITE, 30, 2)], [group(LITE, 100, lists=1), group(LITE, 30, 2)],
              [group(LITE, 30, 2), group(LITE16, 30, 4)], [group(LITE16, 100, 4), group(LITE16, 156, 4)], [group(LITE16, 100, 4), group(LITE16, 157, 4)],
              [group(LITE16, 30, 4), group(LITE, 3, lists=1)], [group(A2FULL, 100), group(A2LITE, 313)], [group(A2LITE, 257), group(A2LITE, 256)],
              [group(STD, 100), group(LITE, 100)], [group(STD, 100), group(NONE, 100)], [group(NONE, 100), group(STD, 100)], [group(STD, 100), group(A2FULL, 100)],
              [group(LITE, 30, 2), group(STD, 3, lists=1)], [group(LITE, 30, 2), group(STD, 3)], [group(NONE, 300, fast=4), group(NONE, 300)],
              [group(NONE, 30, 2), group(NONE, 30, lists=1)], [group(NONE, 30, 4), group(A2FULL, 3, lists=1)]]
    # the table edge: 8, 9 and 40 groups; one stream each (half-size workgroups), even counts, a mix (slots2 * 4 against streams * 5)
    for count in (8, 9, 40):
        for arch, pack in [(STD, 1), (LITE, 1), (LITE, 2), (LITE16, 4), (A2FULL, 1), (A2LITE, 1), (NONE, 1)]:
            lists += [[group(arch, 1, pack)] * count, [group(arch, 2, pack)] * count, [group(arch, 4, pack)] * (count - 3) + [group(arch, 1, pack)] * 3,
                      [group(arch, 4, pack)] * (count - 4) + [group(arch, 1, pack)] * 4, [group(arch, 70, pack)] * count]
        lists += [[group(STD, 1)] * (count - 1) + [group(LITE, 1)], [group(LITE, 1, 2)] * (count - 1) + [group(LITE16, 1, 4)], [group(LITE, 1, lists=1)] * (count - 1) + [group(LITE16, 1, 4)],
                  [group(LITE, 1)] * (count - 1) + [group(LITE16, 1, 4)], [group(A2FULL, 3)] * (count - 1) + [group(A2LITE, 5)], [group(STD, 1)] * (count - 1) + [group(NONE, 1)],
                  [group(STD, 1)] * (count - 1) + [group(STD, 0)], [group(NONE, 1)] + [group(STD, 1)] * (count - 1)]
    return lists


def frame_lists():
    lists = [[group(NONE, count)] for count in COUNTS]
    lists += [[group(NONE, count, a4=a4)] for a4 in frame_fit_edges() for count in (3, 600)]
    lists += [[group(NONE, 300), group(NONE, 211)], [group(NONE, 300), group(NONE, 212)], [group(NONE, 600, a4=512), group(NONE, 1, a4=frame_fit_edges()[2])],
              [group(NONE, 0)], [group(NONE, 3), group(NONE, 0)]]
    for count in (8, 9, 40):
        lists += [[group(NONE, 1)] * count, [group(NONE, 70)] * count, [group(NONE, 70)] * (count - 1) + [group(NONE, 0)]]
    return lists


def library_launch(lib, frame, groups, n, sharing, beyond, cus, mask, vals):
    import ctypes as C
    flat = (C.c_int * (8 * len(groups)))(*[v for g in groups for v in g])
    out = (C.c_int * 11)()
    assert lib.NA_DebugWaveNetLaunch(int(frame), n, len(groups), flat, sharing, int(beyond), cus, mask, vals, out) == 0
    return tuple(out)


# ---- the tests ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def na():
    import neuralaudio_amd
    return neuralaudio_amd


def test_every_launch_lands_on_the_kernel_the_cascades_launched(na):
    """Every list, block length, device size, sharing, cache bit and knob set of the grid: one choice per launch, the instantiation (or the
    refusal, with its error code) the cascades ended on; a list of more than eight groups: the table launch, or the same launches of eight."""
    from neuralaudio_amd import _wavenet_knob_args
    lib = na.capi.load_library()
    wrong, count = [], 0
    for frame, lists in ((False, split_lists()), (True, frame_lists())):
        for knobs in LAUNCH_KNOB_SETS:
            mask, vals = _wavenet_knob_args(knobs)
            for groups in lists:
                for n in BLOCKS:
                    for cus in CUS:
                        for sharing, beyond in ((1, False), (2, False), (1, True), (2, True)) if not frame else ((1, False),):
                            want = list_launch(frame, groups, n, sharing, beyond, cus, knobs)
                            got = library_launch(lib, frame, groups, n, sharing, beyond, cus, mask, vals)
                            if got[0] == K_PIECES:  # (the caller cuts the list and asks again)
                                got = [library_launch(lib, frame, groups[i:i + MAX_GROUPS], n, sharing, beyond, cus, mask, vals) for i in range(0, len(groups), MAX_GROUPS)]
                                assert len(groups) > MAX_GROUPS
                            else:
                                got = [got]
                            count += 1
                            if want != got and len(wrong) < 10:
                                wrong.append((frame, knobs, groups[:9], len(groups), n, cus, sharing, beyond, want, got))
    print("%d launches compared" % count)
    assert not wrong, wrong


def test_the_launch_grid_reaches_every_kernel_and_only_instantiations_that_exist(na):
    """What the restated cascades reach over the grid: every interpreter instantiation of the library (11 plain shapes x GEN, 6 packed),
    every frame-kernel shape, every chain family at every block length it has -- and nothing else"""
    reached = set()
    for frame, lists in ((False, split_lists()), (True, frame_lists())):
        for knobs in LAUNCH_KNOB_SETS:
            for groups in lists:
                for n in BLOCKS:
                    for cus in CUS:
                        for beyond in (False, True):
                            reached |= set(list_launch(frame, groups, n, 2, beyond, cus, knobs))
    interp = {(r[6], r[4], r[7], r[8], r[9]) for r in reached if r[0] == K_INTERPRETER}
    plain = [(4, 2, 2), (4, 1, 2), (4, 2, 1), (4, 1, 1), (2, 4, 4), (2, 2, 4), (2, 1, 4), (2, 2, 2), (2, 1, 2), (2, 2, 1), (2, 1, 1)]
    assert interp == {p + (g, 0) for p in plain for g in (0, 1)} | {(2, s, w, 0, 1) for s in (1, 2) for w in (4, 2, 1)}
    assert {(r[7], r[10], r[4]) for r in reached if r[0] == K_FRAME} == {(2, 0, 1), (2, 1, 4), (2, 2, 2), (2, 2, 1), (2, 1, 2), (2, 1, 1), (1, 0, 1)}
    chains = {(r[2], r[3], r[4], r[9], r[5]) for r in reached if r[0] == K_CHAIN}
    want = {(m, nf, s, pk, 0) for m, pk in ((CH_STD, 0), (CH_LITE, 0), (CH_LITE_PACKED, 1)) for nf in (128, 64, 32) for s in (1, 2)}
    want |= {(CH_A2, nf, s, 0, 0) for nf in (128, 64) for s in (1, 2)} | {(CH_LITE16T1, nf, 2, 1, 0) for nf in (128, 64, 32)}
    want |= {(m, 128, 2, pk, 1) for m, pk in ((CH_STD, 0), (CH_LITE, 0), (CH_LITE_PACKED, 1), (CH_A2, 0))}
    assert chains == want
    tables = {(r[2], r[3], r[4], r[9]) for r in reached if r[0] == K_TABLE}
    assert tables == {(m, nf, s, pk) for m, pk in ((CH_STD, 0), (CH_LITE, 0), (CH_LITE_PACKED, 1), (CH_A2, 0)) for nf in (128, 64) for s in (1, 2)}
    assert {r[1] for r in reached if r[0] == K_NONE} == {INVALID}


def own_group_knobs():
    return {k: (int(v) if k != "NA_WN_KERNEL" else v) for k, v in os.environ.items() if k in GROUP_KNOB_NAMES}


def test_every_group_decides_what_it_decided_before(na):
    """Every model, stream count, quality and knob set of the grid, in this one process: NA_DebugWaveNetKernel's family, pack, input limit,
    range proof and weight check are the recorded ones; the dense layout is the one NA_DebugPackedWeights showed; and NA_ModelKernelInfo /
    NA_DebugPackedWeights themselves still answer as recorded for the knobs this process runs under."""
    gold = np.load(GOLDEN)
    models = grid_models()
    assert [m[0] for m in models] == list(gold["names"])
    loader = na.NeuralModelLoader()
    own = own_group_knobs()
    dense_off = GROUP_KNOB_SETS.index(dict(NA_WN_DENSE=0))
    checked = 0
    for i, model in enumerate(models):
        m = load(loader, model)
        assert m is not None, model[0]
        for k, knobs in enumerate(GROUP_KNOB_SETS):
            for s, streams in enumerate(STREAMS):
                for q, quality in enumerate(QUALITIES):
                    fam, pack, proven, wok, limit = (int(v) for v in gold["info"][k, i, s, q])
                    what = (model[0], knobs, streams, quality)
                    if fam == 0:  # a recurrent model: no WaveNet decision to ask
                        with pytest.raises(na.NeuralAudioError):
                            na.wavenet_kernel(m, streams, quality, knobs)
                        continue
                    c = na.wavenet_kernel(m, streams, quality, knobs)
                    got = (c["family"], c["pack"], c["range_proven"], c["weights_ok"], int(np.float32(c["input_limit"]).view(np.int32)))
                    assert got == (FAMILIES[fam], pack, bool(proven), bool(wok), limit), (what, got)
                    # (the packed weights have another count under NA_WN_DENSE=0 exactly where the default layout is the dense one)
                    was_dense = pack > 1 and gold["packed"][k, i, 0] != gold["packed"][dense_off, i, 0]
                    assert c["dense"] == was_dense and c["virtual"] >= (pack > 1), (what, c)
                    assert c["kernel_name"] == {"f16-split": "WaveNetSpecKernel" if c["spec_arch"] else "WaveNetSplitKernel", "frame": "WaveNetFrameKernel"}.get(
                        c["family"], c["kernel_name"]), (what, c)
                    checked += 1
                    if knobs == own:
                        info = m.KernelInfo(quality, streams)
                        assert (FAMILIES.index(info["kernel"]), info["pack"], info["range_proven"], info["weights_ok"]) == (fam, pack, bool(proven), bool(wok)), what
                        assert int(np.float32(info["input_limit"]).view(np.int32)) == limit, what
            if knobs == own:
                assert packed_count(na, m) == tuple(int(v) for v in gold["packed"][k, i]), (model[0], knobs)
        # the process's own knobs (knob mask -1) are what NA_ModelKernelInfo decides with, whatever they are
        if gold["info"][0, i, 0, 0, 0] != 0:
            for streams in STREAMS:
                c, info = na.wavenet_kernel(m, streams, 1.0, None), m.KernelInfo(1.0, streams)
                assert (c["family"], c["pack"], c["input_limit"], c["range_proven"], c["weights_ok"]) == \
                    (info["kernel"], info["pack"], info["input_limit"], info["range_proven"], info["weights_ok"]), model[0]
    print("%d group decisions compared" % checked)


def test_the_entry_points_that_read_the_environment_answer_as_recorded_under_every_knob_set():
    """NA_ModelKernelInfo and NA_DebugPackedWeights decide with the knobs the process was started with (WaveNetKnobs::FromTuning): one
    fresh child process per knob set, all at once -- the recorder's own child -- gives the recorded grid."""
    gold = np.load(GOLDEN)
    children = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child"], env=knob_env(knobs), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
                for knobs in GROUP_KNOB_SETS]
    for k, (knobs, child) in enumerate(zip(GROUP_KNOB_SETS, children)):
        out, err = child.communicate()
        assert child.returncode == 0, (knobs, err[-2000:])
        got = json.loads(out.splitlines()[-1])
        assert np.array_equal(np.array(got["info"], np.int32), gold["info"][k]), knobs
        assert np.array_equal(np.array(got["packed"], np.int32), gold["packed"][k]), knobs


def test_the_group_grid_reaches_every_family_layout_and_chain():
    """The recording itself: all three families, packs of 2 and 4, dense and 16 / 16 packs, and knob sets that move models"""
    gold = np.load(GOLDEN)
    info, packed = gold["info"], gold["packed"]
    assert set(np.unique(info[0, ..., 0])) == {0, 1, 2, 3} and set(np.unique(info[0, ..., 1])) == {1, 2, 4}
    for k in range(1, len(GROUP_KNOB_SETS)):
        assert (info[k, ..., :2] != info[0, ..., :2]).any() or (packed[k] != packed[0]).any(), GROUP_KNOB_SETS[k]
    assert (info[GROUP_KNOB_SETS.index(dict(NA_WN_PACK=0)), ..., 1] == 1).all()
    assert not (info[GROUP_KNOB_SETS.index(dict(NA_WN_KERNEL="frame")), ..., 0] == 1).any()


if __name__ == "__main__":
    sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # (a build earlier on PYTHONPATH wins: the recorder)
    import neuralaudio_amd
    if sys.argv[1] == "--child":
        grid, packs = record_own_knobs(neuralaudio_amd)
        print(json.dumps(dict(info=grid.tolist(), packed=packs.tolist())))
    else:
        record(sys.argv[1])
