"""CPU-side tests of the product's host code through the C ABI: no GPU needed, no compute calls.

  * the shared library loads and exports every symbol include/*.h declares
  * the loader (C++) agrees with the independent Python reading of the same files (tests/na_oracle.py)
  * error behaviour of the boundary (missing file -> NULL, malformed / wrong weight count -> error, no exception leaks)
  * the product never touches oracle/ and fails loudly without a GPU
"""
import ctypes as C
import copy
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import na_oracle as O
import ref_np
import frame_cases as FC
import recurrent_cases as RC
import split_cases as SC
import tail_cases as TC
import wide_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def na():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "neuralaudio_amd", "libNeuralAudioCAPI.so")):
        g.build()
    import neuralaudio_amd
    return neuralaudio_amd


def _declared_symbols():
    names = []
    for hdr in ("NeuralAudioCApi.h", "neuralaudio_amd.h"):
        text = open(os.path.join(ROOT, "include", hdr)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))
        names += re.findall(r"NA_EXTERN\s+[\w\s\*]+?\b(\w+)\s*\(", text)
    return names


def test_library_exports_every_declared_symbol(na):
    from neuralaudio_amd import capi
    lib = capi.load_library()
    declared = _declared_symbols()
    assert len(declared) >= 15 + 20
    for legacy in capi.LEGACY_SYMBOLS:
        assert legacy in declared  # the reference's 15 symbols, NeuralAudioCApi.h:18-46
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    for name in declared:
        assert name in exported, name
        getattr(lib, name)
    assert sorted(capi.LEGACY_SYMBOLS + capi.NA_SYMBOLS) == sorted(declared)


def test_every_pool_and_stage_entry_point_refuses_a_null_batch_by_name(na):
    """NA_BatchCreate returns NULL where no HIP device is visible, so a host without a GPU reaches these calls with a null batch: each
    returns the failure value include/neuralaudio_amd.h documents for it and leaves an error that begins with its own name.  The
    entry points of the stream pool and of the four per-stream stages share one null check (capi.cpp BatchCall / BatchValue)."""
    from neuralaudio_amd import capi
    lib = capi.load_library()
    gate, sec = capi.NA_GateParams(), (capi.NA_EqSection * 8)()
    cab_info, gate_info, eq_info = capi.NA_CabinetInfo(), capi.NA_GateInfo(), capi.NA_EqInfo()
    taps = (C.c_float * 4)(1.0, 0.0, 0.0, 0.0)
    nonzero, negative, below_dry = (lambda rc: rc != 0), (lambda rc: rc < 0), (lambda rc: rc <= -2)
    calls = [("NA_BatchReserveStreams", (None, 4, 1), negative),
             ("NA_BatchActivateStream", (0, 1.0), nonzero),
             ("NA_BatchParkStream", (0,), nonzero),
             ("NA_BatchEnableOutputStage", (), nonzero),
             ("NA_BatchSetStreamGain", (0, 0.5, 64), nonzero),
             ("NA_BatchGetStreamGain", (0,), negative),
             ("NA_BatchHandover", (0, 1, 1.0, 64), nonzero),
             ("NA_BatchHandoverRemaining", (0,), negative),
             ("NA_BatchEnableCabinetStage", (2048,), nonzero),
             ("NA_BatchGetCabinetInfo", (C.byref(cab_info),), nonzero),
             ("NA_BatchLoadIR", (taps, 4), negative),
             ("NA_BatchUnloadIR", (0,), nonzero),
             ("NA_BatchSetStreamIR", (0, 0, 64), nonzero),
             ("NA_BatchGetStreamIR", (0,), below_dry),
             ("NA_BatchStreamIRFadeRemaining", (0,), negative),
             ("NA_BatchEnableGateStage", (), nonzero),
             ("NA_BatchGetGateInfo", (C.byref(gate_info),), nonzero),
             ("NA_BatchSetStreamGate", (0, C.byref(gate), 1), nonzero),
             ("NA_BatchGetStreamGate", (0, C.byref(gate)), negative),
             ("NA_BatchStreamGateGain", (0,), negative),
             ("NA_BatchEnableEqStage", (), nonzero),
             ("NA_BatchGetEqInfo", (C.byref(eq_info),), nonzero),
             ("NA_BatchSetStreamEq", (0, sec, 1, 0), nonzero),
             ("NA_BatchGetStreamEq", (0, sec, 8), negative),
             ("NA_BatchStreamEqFadeRemaining", (0,), negative)]
    assert len(set(name for name, _, _ in calls)) == 25
    for name, args, failed in calls:
        rc =getattr(lib, name)(None, *args)
        assert failed(rc), (name, rc)
        assert capi.last_error().startswith(name + ": null batch"), (name, capi.last_error())


def test_cpp_api_is_exported_and_a_cpp_host_links(na, tmp_path):
    """The C++ boundary (NeuralModel.h:33-153 of the reference): NeuralModel / NeuralModelLoader are exported from the shared
    library, and a C++ translation unit written against include/NeuralAudio/NeuralModel.h alone links and runs."""
    from neuralaudio_amd import capi
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ("NeuralAudio::NeuralModelLoader::CreateFromFile(", "NeuralAudio::NeuralModelLoader::CreateFromStream(",
                "NeuralAudio::NeuralModelLoader::CreateFromString(", "NeuralAudio::NeuralModelLoader::SupportsWaveNetLoadMode(",
                "NeuralAudio::NeuralModelLoader::SupportsLSTMLoadMode(", "vtable for NeuralAudio::NeuralModel",
                "typeinfo for NeuralAudio::NeuralModel"):
        assert sym in out, sym
    src = tmp_path / "host.cpp"
    src.write_text(
        '#include <NeuralAudio/NeuralModel.h>\n#include <cstdio>\n'
        'int main(int argc, char** argv) {\n'
        '  NeuralAudio::NeuralModelLoader loader;\n'
        '  loader.SetDefaultMaxAudioBufferSize(128);\n'
        '  NeuralAudio::NeuralModel* m = loader.CreateFromFile(argv[1], false);\n'
        '  if (!m) return 3;\n'
        '  std::printf("%d %g %d %d\\n", (int)m->GetLoadMode(), m->GetSampleRate(), m->GetReceptiveFieldSize(), (int)m->IsStatic());\n'
        '  delete m;\n  return loader.CreateFromFile("/nonexistent.nam") == nullptr ? 0 : 4;\n}\n')
    exe = tmp_path / "host"
    libdir = os.path.dirname(capi.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir, "-lNeuralAudioCAPI",
                    "-Wl,-rpath," + libdir], check=True)
    r = subprocess.run([str(exe), os.path.join(O.MODELS_DIR, "BossWN-standard.nam")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["0", "48000", "4092", "1"]


# declaration order of the virtuals of the reference's class NeuralModel (NeuralAudio/NeuralModel.h:40-134; the two destructor entries
# take slots 0 and 1)
REFERENCE_VIRTUAL_ORDER = ["GetLoadMode", "HasQualityScaling", "GetQualityScaleFactor", "IsQualityChangeRealtimeSafe", "SetQualityScaleFactor",
                           "IsStatic", "SetMaxAudioBufferSize", "SetAudioInputLevelDBu", "GetAudioInputLevelDBu",
                           "GetRecommendedInputDBAdjustment", "GetRecommendedOutputDBAdjustment", "GetSampleRate", "GetReceptiveFieldSize",
                           "GetModelVersion", "GetMetadata", "Process", "Prewarm"]


def test_vtable_slots_follow_the_reference_header(na, tmp_path):
    """Binary-level drop-in of the C++ class: every virtual sits in the vtable slot a host compiled against the reference's
    NeuralModel.h expects (slots follow declaration order), and the object has the reference's data members
    (5 floats, a string, a vector: NeuralModel.h:139-145)."""
    exe = tmp_path / "vtable_slots"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "vtable_slots.cpp"), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    slots = {l.split()[0]: int(l.split()[1]) for l in lines if l and not l.startswith("sizeof")}
    assert [n for n, _ in sorted(slots.items(), key=lambda kv: kv[1])] == REFERENCE_VIRTUAL_ORDER
    assert sorted(slots.values()) == list(range(2, 2 + len(REFERENCE_VIRTUAL_ORDER)))
    # vptr + 5 floats (padded to 8) + std::string + std::vector
    assert int([l for l in lines if l.startswith("sizeof")][0].split()[1]) == 8 + 24 + 32 + 24
    ref = "/root/reference/NeuralAudio/NeuralModel.h"
    if os.path.exists(ref):  # (this container only: the list above against the header itself)
        text = open(ref).read()
        body = text[text.index("class NeuralModel"):text.index("class NeuralModelLoader")]
        assert re.findall(r"virtual\s+[\w:<>]+\s+(\w+)\s*\(", body) == REFERENCE_VIRTUAL_ORDER


def test_range_proof_decides_the_wavenet_kernel_family(na):
    """the f16-split kernels run a model only when the plan builder proves that no value leaves the f16 range for inputs
    within a limit >= 8 and that the weights fit the operand format; everything else runs on the f32 frame kernel (host-side decision,
    NA_ModelKernelInfo -- the GPU tests check the kernel that really runs and its parity)."""
    loader = na.NeuralModelLoader()
    std = loader.CreateFromFile(os.path.join(O.MODELS_DIR, "BossWN-standard.nam"), doPrewarm=False)
    info = std.KernelInfo(1.0, 1024)
    assert info["kernel"] == "f16-split" and info["range_proven"] and info["weights_ok"] and 8.0 <= info["input_limit"] <= 32752.0
    arrays = O.a1_arrays(16, 8)
    w = O.synth_wavenet_weights(arrays, seed=5)

    def info_of(weights, arr=arrays, streams=1024):
        m = loader.CreateFromString(O.nam_json_wavenet_generic(arr, weights), ".nam", doPrewarm=False)
        assert m is not None
        return m.KernelInfo(1.0, streams)

    assert info_of(w)["kernel"] == "f16-split"
    # tanh bounds what a layer adds to the residual stream by the row sums of its 1x1: x 4000 they sum past the f16 range
    big = info_of(O.scale_wavenet_tensors(arrays, w, {"1x1": 4000.0}))
    assert big["kernel"] == "frame" and not big["range_proven"] and big["weights_ok"] and big["input_limit"] == float("inf")
    # a moderate scale only lowers the input limit
    mid = info_of(O.scale_wavenet_tensors(arrays, w, {"1x1": 30.0}))
    assert mid["kernel"] == "f16-split" and mid["range_proven"] and 8.0 <= mid["input_limit"] < info_of(w)["input_limit"]
    # weights beyond half the f16 range / a weight matrix below 2^-12: not representable as (hi, lo) f16 pairs
    assert info_of(O.scale_wavenet_tensors(arrays, w, {"mixin": 1e5}))["weights_ok"] is False
    assert info_of(O.scale_wavenet_tensors(arrays, w, {"mixin": 1e5}))["kernel"] == "frame"
    tiny = info_of(O.scale_wavenet_tensors(arrays, w, {"rechannel": 1e-6}))
    assert tiny["kernel"] == "frame" and not tiny["weights_ok"]
    # narrow models: no packing without the proof (packing means the f16-split kernels)
    nano = O.a1_arrays(4, 2)
    wn = O.synth_wavenet_weights(nano, seed=6)
    assert info_of(wn, nano, 4096)["pack"] == 4 and info_of(wn, nano, 4096)["kernel"] == "f16-split"
    bad = info_of(O.scale_wavenet_tensors(nano, wn, {"1x1": 1e4}), nano, 4096)
    assert bad["pack"] == 1 and bad["kernel"] == "frame"
    # LeakyReLU: the worst case grows with the product of the layers' row sums.  The official A2 shapes stay on their chains
    # (saturating arithmetic + NA_BatchStreamRangeEvents); any other LeakyReLU model without a proof runs in f32
    a2 = loader.CreateFromFile(os.path.join(O.MODELS_DIR, "BossWN-a2.nam"), doPrewarm=False)
    for q in (0.0, 1.0):
        ia = a2.KernelInfo(q, 1024)
        assert ia["kernel"] == "f16-split" and not ia["range_proven"] and ia["weights_ok"] and 8.0 <= ia["input_limit"] <= 32752.0
    for layers, want in ((2, "f16-split"), (14, "frame")):
        leaky = [dict(input_size=1, condition_size=1, head_size=1, head_kernel_size=1, head_dilation=1, channels=16, has_head_bias=True,
                      activation=O.ACT_LEAKYRELU, kernel_sizes=[3] * layers, dilations=[1 << (i % 9) for i in range(layers)])]
        il = info_of(O.synth_wavenet_weights(leaky, seed=7), leaky)
        assert il["kernel"] == want and il["range_proven"] == (want == "f16-split"), (layers, il)


def test_rccl_is_bound_at_run_time_and_the_library_does_not_link_it(na):
    """The multi-GPU host's RCCL fan-out / fan-in (csrc/multi_gpu.cpp, rccl_dyn.cpp): librccl.so is loaded with dlopen when a multi
    batch asks for it -- every entry point resolves against the installed library (no GPU needed for that) -- and the product library
    itself still links only libamdhip64 (single-GPU hosts never load RCCL)."""
    from neuralaudio_amd import capi
    needed = subprocess.run(["readelf", "-d", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    libs = re.findall(r"Shared library: \[([^\]]+)\]", needed)
    assert any(l.startswith("libamdhip64") for l in libs) and not any("rccl" in l or "nccl" in l for l in libs), libs
    if not os.path.exists("/opt/rocm/lib/librccl.so.1"):
        pytest.skip("no RCCL in this image")
    assert na.rccl_available(), capi.last_error()
    # the fan-in mode is a property of a multi batch, fixed at Commit; without a device the batch itself cannot be created
    if na.device_count() == 0:
        with pytest.raises(na.NeuralAudioError):
            na.MultiBatch([0])


def test_modeltest_host_builds_and_reports_a_missing_gpu(na):
    """tools/ModelTest (the reference's Utils/ModelTest counterpart) is a C++ host of the exported API; without a device it must say so."""
    subprocess.run(["make", "-C", os.path.join(ROOT, "tools", "ModelTest")], check=True, capture_output=True)
    exe = os.path.join(ROOT, "tools", "bin", "ModelTest")
    assert subprocess.run([exe, "--bogus"], capture_output=True).returncode == 1
    if na.device_count() > 0:
        pytest.skip("a GPU is present: tests/test_gpu_modeltest.py runs it for real")
    r = subprocess.run([exe, "-b", "128", os.path.join(O.MODELS_DIR, "BossLSTM-1x16.nam")], capture_output=True, text=True)
    assert r.returncode == 2 and "no HIP device" in r.stdout and "Block size: 128  Quality Scale: 1" in r.stdout


def test_release_library_exports_the_documented_surface_and_nothing_else(na):
    """make release -> dist/libNeuralAudioCAPI.so (-DNA_RELEASE -DNA_NO_TUNING, no loopback RCCL table): its dynamic symbol table is the 15
    legacy symbols of the reference's NeuralAudioCApi.h:18-46 plus the NA_* set include/neuralaudio_amd.h declares outside its
    `#ifndef NA_RELEASE` block -- no NA_Debug* hook, no loopback table, no tuning environment reader."""
    import re
    from neuralaudio_amd import capi
    subprocess.run(["make", "-C", os.path.join(ROOT, "neuralaudio_amd", "csrc"), "-j8", "release"], check=True, capture_output=True)
    lib = os.path.join(ROOT, "dist", "libNeuralAudioCAPI.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] in "TWBDRV" and not l.split()[-1].startswith("_")}
    header = open(os.path.join(ROOT, "include", "neuralaudio_amd.h")).read()
    public, hooks = header.split("#ifndef NA_RELEASE")[0], header.split("#ifndef NA_RELEASE")[1].split("#endif /* NA_RELEASE */")[0]
    declared = set(re.findall(r"NA_EXTERN[^;(]*?\b(NA_[A-Za-z0-9]+)\(", public))
    debug = set(re.findall(r"NA_EXTERN[^;(]*?\b(NA_[A-Za-z0-9]+)\(", hooks))
    assert debug and all(n.startswith("NA_Debug") for n in debug)
    assert set(capi.NA_SYMBOLS) == declared | debug  # (the Python binding list and the header agree)
    assert exported == set(capi.LEGACY_SYMBOLS) | declared, (sorted(exported - set(capi.LEGACY_SYMBOLS) - declared), sorted((set(capi.LEGACY_SYMBOLS) | declared) - exported))
    data = open(lib, "rb").read()
    assert b"NA_WN_KERNEL" not in data and b"NA_LSTM_LANE_KERNEL" not in data  # no tuning knob is read
    assert b"gfx950" in data and b"WaveNetSpecKernel" in data


def test_no_kernel_feeds_a_loaded_register_to_a_packed_f32_instruction_through_op_sel(na):
    """gfx950 (profiles/r06_quad_race.txt, tools/microbench/pk_lds_opsel.hip): v_pk_fma_f32 with a non-default op_sel / op_sel_hi on a register
    that a 128-bit load (ds_read_b128, global_load_dwordx4) has just delivered is wrong in lanes 48 .. 63 now and then while another wave
    issues MFMAs on the SIMD.  The library's kernels have thousands of packed-f32 operands with op_sel -- on ALU / MFMA results -- and must
    have none on a loaded register: the hand-written ones go through pairs or copies, the compiler's own pairing (SLP) is off for the
    recurrent files (csrc/Makefile).  A scan of the disassembly of every code object in the built library."""
    import importlib.util
    from neuralaudio_amd import capi
    spec = importlib.util.spec_from_file_location("pk_opsel_sources", os.path.join(ROOT, "tools", "analysis", "pk_opsel_sources.py"))
    scan = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(scan)
    if not os.path.exists(scan.OBJDUMP):
        pytest.skip("no llvm-objdump under /opt/rocm")
    n, total, found = scan.scan_library(capi.LIB_PATH)
    assert n >= 10 and sum(total.values()) > 1000  # (the scan saw the kernels and their packed instructions)
    assert any("RecurrentQuadKernel" in k for k in total)
    assert not found, sorted(found.items())


def test_library_embeds_gfx950_code_object(na):
    from neuralaudio_amd import capi
    data = open(capi.LIB_PATH, "rb").read()
    assert b"gfx950" in data and b"WaveNetSplitKernel" in data and b"WaveNetFrameKernel" in data and b"LstmBlockKernel" in data


@pytest.mark.parametrize("name", ["BossWN-standard.nam", "BossWN-feather.nam", "BossWN-nano.nam", "BossWN-a2.nam",
                                  "BossLSTM-1x16.nam", "BossLSTM-2x8.nam", "tw40_blues_deluxe_deerinkstudios.json"])
def test_loader_reads_reference_sample_models(na, name):
    loader = na.NeuralModelLoader()
    for wide in (False, True):
        m = loader.CreateFromFile(os.path.join(O.MODELS_DIR, name), doPrewarm=False, use_wchar_entry=wide) if not wide else None
        if m is None:
            continue
        j = O.load_json(name)
        assert m.GetLoadMode() == na.EModelLoadMode.Internal
        assert m.GetSampleRate() == 48000.0
        if name.endswith(".nam"):
            assert m.GetModelVersion() == j["version"]
            loud = j["metadata"]["loudness"]
            assert m.GetRecommendedOutputDBAdjustment() == pytest.approx(-18.0 - loud, abs=1e-5)  # NeuralModel.h:92-95
            assert float(m.GetMetadata("loudness")) == pytest.approx(loud)
            assert m.GetMetadata("no_such_field") == ""
        else:
            assert m.GetRecommendedOutputDBAdjustment() == 0.0
        assert m.GetRecommendedInputDBAdjustment() == 0.0  # 12 dBu default on both sides
        arch = j.get("architecture")
        if arch == "WaveNet":
            assert m.GetReceptiveFieldSize() == 4092 and m.IsStatic() and not m.HasQualityScaling()
        elif arch == "SlimmableContainer":
            assert m.GetReceptiveFieldSize() == 6346 and m.IsStatic() and m.HasQualityScaling()
        else:
            assert m.GetReceptiveFieldSize() == -1 and not m.HasQualityScaling()


def test_quality_scaling_follows_reference_rule(na):
    loader = na.NeuralModelLoader()
    loader.SetDefaultQualityScaleFactor(0.25)
    m = loader.CreateFromFile(os.path.join(O.MODELS_DIR, "BossWN-a2.nam"), doPrewarm=False)
    assert m.HasQualityScaling() and m.GetQualityScaleFactor() == pytest.approx(0.25)
    m.SetQualityScaleFactor(0.9)
    assert m.GetQualityScaleFactor() == pytest.approx(0.9)
    plain = loader.CreateFromFile(os.path.join(O.MODELS_DIR, "BossWN-nano.nam"), doPrewarm=False)
    plain.SetQualityScaleFactor(0.1)
    assert plain.GetQualityScaleFactor() == 1.0  # NeuralModel.h:50-53 default


def test_input_level_calibration(na):
    loader = na.NeuralModelLoader()
    loader.SetAudioInputLevelDBu(18.0)
    m = loader.CreateFromFile(os.path.join(O.MODELS_DIR, "BossWN-nano.nam"), doPrewarm=False)
    assert m.GetRecommendedInputDBAdjustment() == pytest.approx(6.0)  # audioInputLevelDBu - modelInputLevelDBu(12)


def test_missing_and_malformed_files(na, tmp_path):
    loader = na.NeuralModelLoader()
    assert loader.CreateFromFile(str(tmp_path / "nope.nam")) is None  # NeuralModel.cpp:321-322
    bad = tmp_path / "bad.nam"
    bad.write_text("{ this is not json")
    with pytest.raises(na.NeuralAudioError):
        loader.CreateFromFile(str(bad))
    j = O.load_json("BossWN-nano.nam")
    j["weights"] = j["weights"][:-3]
    short = tmp_path / "short.nam"
    short.write_text(json.dumps(j))
    with pytest.raises(na.NeuralAudioError, match="Wrong number of weights. Expected 842 but got 839"):  # at LOAD, like WaveNet.h:704-709
        loader.CreateFromFile(str(short), doPrewarm=False)
    arr = [dict(O.a1_arrays(4, 2)[0], channels=20, head_size=1)]
    short.write_text(O.nam_json_wavenet_generic(arr, O.synth_wavenet_weights(arr, seed=2)))
    assert loader.CreateFromFile(str(short), doPrewarm=False) is not None  # > 16 channels: the runtime-shaped kernel (WaveNetDynamic.h)
    arr = [dict(O.a1_arrays(4, 2)[0], channels=80, head_size=1)]
    short.write_text(O.nam_json_wavenet_generic(arr, O.synth_wavenet_weights(arr, seed=2)))
    assert loader.CreateFromFile(str(short), doPrewarm=False) is not None  # 65 .. 128 channels: WaveNetWideKernel
    arr = [dict(O.a1_arrays(4, 2)[0], channels=144, head_size=1)]
    short.write_text(O.nam_json_wavenet_generic(arr, [0.0]))
    with pytest.raises(na.NeuralAudioError, match="channels > 128"):  # kernel limits are load-time errors too
        loader.CreateFromFile(str(short), doPrewarm=False)
    arr = [dict(O.a1_arrays(4, 2)[0], channels=80, head_size=1, head_kernel_size=4)]
    short.write_text(O.nam_json_wavenet_generic(arr, [0.0]))
    with pytest.raises(na.NeuralAudioError, match="conv head on a layer array wider than 64"):
        loader.CreateFromFile(str(short), doPrewarm=False)
    conv = tmp_path / "conv.json"
    conv.write_text(json.dumps({"in_shape": [None, None, 1], "layers": [{"type": "conv2d", "shape": [None, None, 8], "weights": []},
                                                                        {"type": "dense", "shape": [None, None, 1], "weights": []}]}))
    assert loader.CreateFromFile(str(conv)) is None  # keras layer types without a kernel: no model (the reference needs RTNeural for them)
    gru = tmp_path / "gru.json"
    gru.write_text(json.dumps(O.synth_keras_gru(1, 16, seed=3)))
    g = loader.CreateFromFile(str(gru), doPrewarm=False)  # keras GRU: RTNeural's arithmetic in the reference, restated here
    assert g is not None and g.GetSampleRate() == 48000.0 and g.GetReceptiveFieldSize() == -1
    wide = O.synth_keras_gru(1, 16, seed=3)
    wide["layers"][-1]["weights"] = [[[0.1, 0.2]] * 16, [0.0, 0.0]]  # dense head with 2 outputs: a generic stack (output = unit 0)
    wide["layers"][-1]["shape"] = [None, None, 2]
    gru.write_text(json.dumps(wide))
    assert loader.CreateFromFile(str(gru), doPrewarm=False) is not None
    wide["layers"][-1]["shape"] = [None, None, 1]  # ... but the declared shape must match the weights
    gru.write_text(json.dumps(wide))
    with pytest.raises(na.NeuralAudioError, match="unexpected weight shapes"):
        loader.CreateFromFile(str(gru), doPrewarm=False)


def test_lstm_shapes_accepted_or_rejected_at_load(na, tmp_path):
    """Any hidden size the reference's dynamic LSTM takes loads (runtime-shaped kernel); what has no kernel fails at load, with a reason."""
    loader = na.NeuralModelLoader()
    path = tmp_path / "m.nam"
    # (up to 1024 units whatever the weight size: streamed from L2, a workgroup of up to 16 waves per stream from 65 gate rows on)
    for layers, hidden in ((1, 3), (1, 18), (3, 16), (2, 64), (3, 128), (2, 192), (1, 512)):
        path.write_text(O.nam_json_lstm(layers, hidden, O.synth_lstm_weights(layers, hidden, seed=hidden)))
        assert loader.CreateFromFile(str(path), doPrewarm=False) is not None
    path.write_text(O.nam_json_lstm(1, 1030, O.synth_lstm_weights(1, 1030, seed=1)))
    with pytest.raises(na.NeuralAudioError, match="LSTM 1x1030 is not supported"):
        loader.CreateFromFile(str(path), doPrewarm=False)
    gru = tmp_path / "gru.json"
    for layers, hidden in ((3, 16), (1, 96), (2, 128), (1, 160)):
        gru.write_text(json.dumps(O.synth_keras_gru(layers, hidden, seed=3)))
        assert loader.CreateFromFile(str(gru), doPrewarm=False) is not None  # any shape up to 1024 units: runtime-shaped GRU kernel
    # a dense TAIL (more than the 1-unit head) behind a wide recurrent layer needs the [samples][units] buffer of the block in LDS:
    # 2 x 400 x 64 floats do not fit
    j = O.synth_keras_gru(1, 400, seed=3)
    j["layers"][-1] = {"type": "dense", "activation": "tanh", "shape": [None, None, 4], "weights": [[[0.01] * 4] * 400, [0.0] * 4]}
    j["layers"].append({"type": "dense", "activation": "", "shape": [None, None, 1], "weights": [[[0.5]] * 4, [0.0]]})
    gru.write_text(json.dumps(j))
    with pytest.raises(na.NeuralAudioError, match="GRU 1x400 is not supported"):
        loader.CreateFromFile(str(gru), doPrewarm=False)
    gru.write_text(json.dumps(O.synth_keras_gru(1, 1100, seed=3)))
    with pytest.raises(na.NeuralAudioError, match="GRU 1x1100 is not supported"):
        loader.CreateFromFile(str(gru), doPrewarm=False)


def test_generic_keras_stacks_accepted_or_rejected_at_load(na, tmp_path):
    """Stacks of lstm | gru and dense layers with activations -- what the reference hands to RTNeural (NeuralModel.cpp:565-572) -- load;
    layer types / activations / sizes without a kernel fail at load with a reason (no silent fallback)."""
    import ref_np as R
    loader = na.NeuralModelLoader()
    path = tmp_path / "m.json"
    for spec in ([("lstm", 8), ("dense", 6, "tanh"), ("dense", 1)], [("gru", 12), ("dense", 5, "relu"), ("dense", 3, "sigmoid"), ("dense", 1)],
                 [("dense", 8, "tanh"), ("dense", 4, "elu"), ("dense", 1)], [("gru", 8), ("dense", 2)], [("lstm", 16), ("dense", 1, "tanh")],
                 # the element-wise layers of RTNeural's parser, lowered to dense layers at load (model_loader.cpp AppendKerasTailLayer)
                 [("gru", 8), ("dense", 6), ("batchnorm", 6), ("activation", 6, "tanh"), ("dense", 1)],
                 [("lstm", 8), ("prelu", 8), ("dense", 4), ("prelu", 4, "scalar"), ("batchnorm", 4, "noaffine"), ("dense", 1)],
                 [("dense", 8), ("activation", 8, "relu"), ("batchnorm", 8), ("dense", 1)]):
        path.write_text(json.dumps(R.synth_keras_stack(spec, seed=5)))
        m = loader.CreateFromFile(str(path), doPrewarm=False)
        assert m is not None, spec
    bad = R.synth_keras_stack([("gru", 8), ("dense", 4, "tanh"), ("dense", 1)], seed=6)
    bad["layers"][1]["activation"] = "gelu"
    path.write_text(json.dumps(bad))
    with pytest.raises(na.NeuralAudioError, match="activation 'gelu' is not supported"):
        loader.CreateFromFile(str(path), doPrewarm=False)
    bad["layers"][1]["activation"] = "softmax"  # (round 5: across the units of its layer)
    path.write_text(json.dumps(bad))
    assert loader.CreateFromFile(str(path), doPrewarm=False) is not None
    path.write_text(json.dumps(R.synth_keras_stack([("gru", 8), ("dense", 100, "tanh"), ("dense", 1)], seed=6)))
    assert loader.CreateFromFile(str(path), doPrewarm=False) is not None  # (dense layers up to 256 units since round 4)
    path.write_text(json.dumps(R.synth_keras_stack([("gru", 8), ("dense", 300, "tanh"), ("dense", 1)], seed=6)))
    with pytest.raises(na.NeuralAudioError, match="wider than 256 units"):
        loader.CreateFromFile(str(path), doPrewarm=False)
    mixed = R.synth_keras_stack([("gru", 8), ("lstm", 8), ("dense", 1)], seed=7)  # two kinds of recurrent layers: no kernel
    path.write_text(json.dumps(mixed))
    assert loader.CreateFromFile(str(path), doPrewarm=False) is None
    wide = R.synth_keras_stack([("gru", 8), ("dense", 140), ("prelu", 140), ("dense", 1)], seed=9)  # relu(x) - alpha relu(-x): twice the width in between
    path.write_text(json.dumps(wide))
    with pytest.raises(na.NeuralAudioError, match="prelu layer wider than 128 units"):
        loader.CreateFromFile(str(path), doPrewarm=False)
    # conv1d layers (round 5): causal, dilated, behind the recurrent layers or in a stack without any; their limits are load errors
    for spec in ([("conv1d", 8, 3, 1, "tanh"), ("conv1d", 4, 2, 4, "relu"), ("dense", 1)], [("lstm", 8), ("conv1d", 6, 5, 3), ("prelu", 6), ("batchnorm", 6), ("dense", 1)],
                 [("gru", 12), ("conv1d", 16, 4, 64, "elu"), ("dense", 5, "softmax"), ("dense", 1)]):
        path.write_text(json.dumps(R.synth_keras_stack(spec, seed=8)))
        assert loader.CreateFromFile(str(path), doPrewarm=False) is not None, spec
    conv = R.synth_keras_stack([("conv1d", 4, 3, 1, "tanh"), ("dense", 1)], seed=8)
    conv["layers"][0]["strides"] = [2]
    path.write_text(json.dumps(conv))
    with pytest.raises(na.NeuralAudioError, match="stride or groups"):
        loader.CreateFromFile(str(path), doPrewarm=False)
    path.write_text(json.dumps(R.synth_keras_stack([("conv1d", 4, 3, 600), ("dense", 1)], seed=8)))
    with pytest.raises(na.NeuralAudioError, match="more than 1024 samples of history"):
        loader.CreateFromFile(str(path), doPrewarm=False)
    path.write_text(json.dumps(R.synth_keras_stack([("conv1d", 200, 3, 400), ("dense", 1)], seed=8)))  # two [200][800 + 128] buffers: beyond the LDS
    with pytest.raises(na.NeuralAudioError, match="conv1d layers with its two"):
        loader.CreateFromFile(str(path), doPrewarm=False)
    front = R.synth_keras_stack([("conv1d", 4, 3, 1, "tanh"), ("dense", 1)], seed=8)  # a conv1d layer in FRONT of a recurrent one: no kernel
    front["layers"].insert(1, R.synth_keras_stack([("dense", 4), ("gru", 8)], seed=8)["layers"][1])
    path.write_text(json.dumps(front))
    assert loader.CreateFromFile(str(path), doPrewarm=False) is None


def test_stream_packing_builds_a_block_diagonal_virtual_model(na):
    """Stream packing, host side (no GPU): Nano packs 4 streams, Feather 2, Standard / A2 none; the virtual model's flat weights hold
    the real model's tensors on the block diagonal, replicated vectors, zeros elsewhere, in the reference's weight order.  Nano's pack
    is dense: 16 / 8 virtual channels (wavenet_plan.cpp WaveNetPackCanBeDense)."""
    import ctypes as C
    from neuralaudio_amd import capi
    lib = capi.load_library()
    loader = na.NeuralModelLoader()
    mdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "models")

    def packed(name):
        m = loader.CreateFromFile(os.path.join(mdir, name), doPrewarm=False)
        pf = C.c_int(0)
        n = lib.NA_DebugPackedWeights(m._h, C.byref(pf), None, 0)
        assert n >= 0, capi.last_error()
        out = np.zeros(n, np.float32)
        if n:
            assert lib.NA_DebugPackedWeights(m._h, C.byref(pf), out.ctypes.data_as(C.POINTER(C.c_float)), n) == n
        return pf.value, out

    assert packed("BossWN-standard.nam")[0] == 1 and packed("BossWN-a2.nam")[0] == 1
    for name, P in (("BossWN-nano.nam", 4), ("BossWN-feather.nam", 2)):
        pf, v = packed(name)
        assert pf == P
        j = O.load_json(name)
        w = np.array(j["weights"], np.float32)
        arrays = O.wavenet_arrays_from_nam(j)
        pad = [4 * ((a["channels"] + 3) // 4) for a in arrays]
        if P == 4 and [a["channels"] for a in arrays] == [4, 2] and os.environ.get("NA_WN_DENSE") != "0":
            pad[1] = 2  # dense pack (round 5): the 2-channel arrays of the four streams side by side, two streams per channel group
        pos = vpos = 0
        for ai, a in enumerate(arrays):
            C_, Cp = a["channels"], pad[ai]
            Cv = P * Cp
            In = a["input_size"]
            Inv = 1 if ai == 0 else P * pad[ai - 1]
            Inp = 1 if ai == 0 else pad[ai - 1]
            re_ = w[pos:pos + C_ * In].reshape(C_, In); pos += C_ * In
            vre = v[vpos:vpos + Cv * Inv].reshape(Cv, Inv); vpos += Cv * Inv
            for q in range(P):
                blk = vre[q * Cp:q * Cp + C_, (0 if ai == 0 else q * Inp):(1 if ai == 0 else q * Inp + In)]
                assert np.array_equal(blk, re_)
            assert np.count_nonzero(vre) == P * np.count_nonzero(re_)
            for K in a["kernel_sizes"]:
                conv = w[pos:pos + C_ * C_ * K].reshape(C_, C_, K); pos += C_ * C_ * K
                vec = [w[pos + i * C_:pos + (i + 1) * C_] for i in range(2)]; pos += 2 * C_
                w1 = w[pos:pos + C_ * C_].reshape(C_, C_); pos += C_ * C_
                b1 = w[pos:pos + C_]; pos += C_
                vconv = v[vpos:vpos + Cv * Cv * K].reshape(Cv, Cv, K); vpos += Cv * Cv * K
                vvec = [v[vpos + i * Cv:vpos + (i + 1) * Cv] for i in range(2)]; vpos += 2 * Cv
                vw1 = v[vpos:vpos + Cv * Cv].reshape(Cv, Cv); vpos += Cv * Cv
                vb1 = v[vpos:vpos + Cv]; vpos += Cv
                for q in range(P):
                    s_ = slice(q * Cp, q * Cp + C_)
                    assert np.array_equal(vconv[s_, s_], conv) and np.array_equal(vw1[s_, s_], w1) and np.array_equal(vb1[s_], b1)
                    assert np.array_equal(vvec[0][s_], vec[0]) and np.array_equal(vvec[1][s_], vec[1])
                assert np.count_nonzero(vconv) == P * np.count_nonzero(conv) and np.count_nonzero(vw1) == P * np.count_nonzero(w1)
            Hs = a["head_size"]
            last = ai == len(arrays) - 1
            Hp = 1 if last else pad[ai + 1]
            head = w[pos:pos + Hs * C_].reshape(Hs, C_); pos += Hs * C_
            vhead = v[vpos:vpos + P * Hp * Cv].reshape(P * Hp, Cv); vpos += P * Hp * Cv
            for q in range(P):
                assert np.array_equal(vhead[q * Hp:q * Hp + Hs, q * Cp:q * Cp + C_], head)
            assert np.count_nonzero(vhead) == P * np.count_nonzero(head)
            if a["has_head_bias"]:
                hb = w[pos:pos + Hs]; pos += Hs
                vhb = v[vpos:vpos + P * Hp]; vpos += P * Hp
                for q in range(P):
                    assert np.array_equal(vhb[q * Hp:q * Hp + Hs], hb)
        assert v[vpos] == w[pos] and vpos + 1 == v.size and pos + 1 == w.size  # head scale


def test_number_parsing_ignores_the_c_locale(na, tmp_path):
    """A host that called setlocale(LC_ALL, "") under a comma-decimal locale must still read "0.1234" as 0.1234."""
    import locale
    import subprocess
    import sys
    code = (
        "import locale, sys, os\n"
        "sys.path.insert(0, %r)\n"
        "ok = False\n"
        "for name in ('de_DE.UTF-8', 'fr_FR.UTF-8', 'de_DE', 'fr_FR', 'nl_NL.UTF-8', 'ru_RU.UTF-8'):\n"
        "    try:\n"
        "        locale.setlocale(locale.LC_ALL, name); ok = True; break\n"
        "    except locale.Error:\n"
        "        pass\n"
        "import neuralaudio_amd as na\n"
        "m = na.NeuralModelLoader().CreateFromFile(%r, doPrewarm=False)\n"
        "print('LOCALE' if ok else 'NOLOCALE', m.GetMetadata('loudness'), m.GetRecommendedOutputDBAdjustment())\n"
    ) % (ROOT, os.path.join(O.MODELS_DIR, "BossWN-nano.nam"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True).stdout.split()
    ref = json.load(open(os.path.join(O.MODELS_DIR, "BossWN-nano.nam")))["metadata"]["loudness"]
    assert float(out[1]) == ref and abs(float(out[2]) - (-18 - ref)) < 1e-5
    # the image may carry no comma-decimal locale: the in-process check below covers the parser either way
    loader = na.NeuralModelLoader()
    j = O.load_json("BossWN-nano.nam")
    j["metadata"]["gain"] = 0.1234
    j["metadata"]["loudness"] = -20.5
    p = tmp_path / "m.nam"
    p.write_text(json.dumps(j))
    m = loader.CreateFromFile(str(p), doPrewarm=False)
    assert m.GetMetadata("gain") == "0.1234" and abs(m.GetRecommendedOutputDBAdjustment() - 2.5) < 1e-6


def test_metadata_values_are_dumped_like_nlohmann(na, tmp_path):
    """GetMetadata returns json.dump() text (NeuralModelImpl.h:85-94): shortest round-trip floats, "3.0" stays "3.0", sorted keys."""
    loader = na.NeuralModelLoader()
    j = O.load_json("BossWN-nano.nam")
    j["metadata"].update({"a_tenth": 0.1, "three": 3.0, "int": 3, "tiny": 1e-05, "big": 1.5e+20, "neg": -0.25,
                          "nested": {"zeta": 1, "alpha": [1.5, 2, "x"], "mid": None}})
    p = tmp_path / "m.nam"
    p.write_text(json.dumps(j))
    m = loader.CreateFromFile(str(p), doPrewarm=False)
    assert m.GetMetadata("a_tenth") == "0.1"
    assert m.GetMetadata("three") == "3.0"
    assert m.GetMetadata("int") == "3"
    assert m.GetMetadata("tiny") == "1e-05"
    assert m.GetMetadata("big") == "1.5e+20"
    assert m.GetMetadata("neg") == "-0.25"
    assert m.GetMetadata("nested") == '{"alpha":[1.5,2,"x"],"mid":null,"zeta":1}'


def test_numbers_beyond_the_double_range_follow_the_literal_not_its_spelling(na, tmp_path):
    """Out-of-range literals: underflow -> 0 whatever the spelling (plain decimals and positive exponents with many leading
    zeros included), overflow -> +-inf, subnormals keep their value (libstdc++'s from_chars reports them as out of range)."""
    loader = na.NeuralModelLoader()
    j = O.load_json("BossWN-nano.nam")
    text = json.dumps(j)
    extra = ('"u1": 1e-400, "u2": 0.' + "0" * 400 + '1, "u3": 0.' + "0" * 400 + '1e+20, "o1": 1e400, "o2": -1' + "0" * 400 + '.0, '
             '"sub": 4.9406564584124654e-324, "sub2": 2.5e-310, "edge": 1.7976931348623157e308, ')
    text = text.replace('"metadata": {', '"metadata": {' + extra, 1)
    p = tmp_path / "m.nam"
    p.write_text(text)
    m = loader.CreateFromFile(str(p), doPrewarm=False)
    assert m is not None
    assert float(m.GetMetadata("u1")) == 0.0 and float(m.GetMetadata("u2")) == 0.0 and float(m.GetMetadata("u3")) == 0.0
    assert m.GetMetadata("o1") in ("null", "inf", "Infinity") or float(m.GetMetadata("o1")) == float("inf")
    assert m.GetMetadata("o2") in ("null", "-inf", "-Infinity") or float(m.GetMetadata("o2")) == float("-inf")
    assert float(m.GetMetadata("sub")) == 5e-324 and float(m.GetMetadata("sub2")) == 2.5e-310
    assert float(m.GetMetadata("edge")) == 1.7976931348623157e308


def test_a2_features_outside_the_internal_path_are_rejected(na, tmp_path):
    """NAMIsA2Standard (NeuralModel.cpp:188-317) sends such files to NAM Core; without that back-end they must not load silently."""
    loader = na.NeuralModelLoader()
    base = O.load_json("BossWN-a2.nam")["config"]["submodels"][1]["model"]  # a plain A2 WaveNet (ch8)

    def variant(edit):
        j = copy.deepcopy(base)
        edit(j["config"]["layers"][0], j["config"])
        path = tmp_path / "v.nam"
        path.write_text(json.dumps(j))
        return str(path)

    assert loader.CreateFromFile(variant(lambda lc, c: None), doPrewarm=False) is not None
    # optional blocks that are simply absent are fine (they have no weights either)
    assert loader.CreateFromFile(variant(lambda lc, c: [lc.pop(k) for k in ("conv_pre_film", "head1x1", "slimmable")]), doPrewarm=False) is not None
    edits = {
        "head1x1": lambda lc, c: lc["head1x1"].update(active=True),
        "conv_post_film": lambda lc, c: lc["conv_post_film"].update(active=True),
        "gating_mode": lambda lc, c: lc.update(gating_mode=["gated"] * len(lc["dilations"])),
        "secondary_activation": lambda lc, c: lc.update(secondary_activation=[{"type": "Sigmoid"}] * len(lc["dilations"])),
        "bottleneck": lambda lc, c: lc.update(bottleneck=4),
        "layer1x1": lambda lc, c: lc["layer1x1"].update(active=False),
        "groups_input": lambda lc, c: lc.update(groups_input=2),
        "negative_slope": lambda lc, c: lc["activation"][3].update(negative_slope=0.2),
        "slimmable": lambda lc, c: lc.update(slimmable={"method": "slice_channels_uniform"}),
        "model-level head": lambda lc, c: c.update(head={"channels": 8}),
        "condition_dsp": lambda lc, c: c.update(condition_dsp={"architecture": "WaveNet"}),
        "in_channels": lambda lc, c: c.update(in_channels=2),
    }
    for what, edit in edits.items():
        with pytest.raises(na.NeuralAudioError, match="NAM Core"):
            loader.CreateFromFile(variant(edit), doPrewarm=False)


def test_unicode_path_through_wchar_entry(na, tmp_path):
    src = os.path.join(O.MODELS_DIR, "BossWN-nano.nam")
    dst = tmp_path / "mödel-音.nam"
    dst.write_bytes(open(src, "rb").read())
    loader = na.NeuralModelLoader()
    assert loader.CreateFromFile(str(tmp_path / "absent.nam"), use_wchar_entry=True) is None
    if na.device_count() == 0:
        # CreateModelFromFile prewarms (reference semantics); without a GPU the model stays a host-side template
        m = loader.CreateFromFile(str(dst), use_wchar_entry=True)
        assert m is not None and m.GetReceptiveFieldSize() == 4092


def test_load_modes_other_than_internal_are_rejected(na):
    from neuralaudio_amd import capi
    loader = na.NeuralModelLoader()
    loader.SetWaveNetLoadMode(na.EModelLoadMode.NAMCore)   # ignored like the reference without BUILD_NAMCORE
    loader.SetLSTMLoadMode(na.EModelLoadMode.RTNeural)
    m = loader.CreateFromFile(os.path.join(O.MODELS_DIR, "BossLSTM-1x16.nam"), doPrewarm=False)
    assert m.GetLoadMode() == na.EModelLoadMode.Internal
    assert capi.load_library().NA_GetVersion().decode().startswith("neuralaudio_amd")


def test_process_without_gpu_fails_loudly(na):
    """No CPU fallback: on a box without a HIP device Process must report an error, not return numbers."""
    if na.device_count() > 0:
        pytest.skip("a GPU is present")
    from neuralaudio_amd import capi
    loader = na.NeuralModelLoader()
    m = loader.CreateFromFile(os.path.join(O.MODELS_DIR, "BossWN-nano.nam"), doPrewarm=False)
    x = np.ones(16, np.float32)
    y = np.full(16, 123.0, np.float32)
    fp = C.POINTER(C.c_float)
    capi.load_library().Process(m._h, x.ctypes.data_as(fp), y.ctypes.data_as(fp), 16)
    assert "no HIP device" in capi.last_error()
    assert np.all(y == 0.0)  # silence, never uninitialised memory (and never numbers from some fallback)
    # a second call must fail the same way (no half-built device state left behind by the first)
    y[:] = 123.0
    assert capi.load_library().NA_ProcessChecked(m._h, x.ctypes.data_as(fp), y.ctypes.data_as(fp), 16) != 0
    assert np.all(y == 0.0)
    with pytest.raises(na.NeuralAudioError):
        m.Process(x)
    with pytest.raises(na.NeuralAudioError):
        na.Batch(0)


def test_product_never_references_the_oracle():
    """oracle/ is test infrastructure: nothing under neuralaudio_amd/ or include/ may mention it."""
    bad = []
    for base in ("neuralaudio_amd", "include"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, base)):
            if "build" in dirpath or "__pycache__" in dirpath:
                continue
            for f in files:
                if f.endswith((".so", ".o", ".pyc")):
                    continue
                text = open(os.path.join(dirpath, f), errors="replace").read()
                if "na_oracle" in text or "oracle/" in text or "ref_np" in text:
                    bad.append(os.path.join(dirpath, f))
    assert not bad, bad


def test_shard_ranges_partition_and_balance(na):
    from neuralaudio_amd.sharding import shard_ranges
    for n, w in [(8192, 8), (16384, 8), (10, 3), (3, 8), (1, 1), (0, 2)]:
        r = shard_ranges([1.0] * n, w)
        assert len(r) == w and r[0][0] == 0 and r[-1][1] == n
        for (a, b), (c, d) in zip(r, r[1:]):
            assert b == c and a <= b
        if n >= w:
            sizes = [b - a for a, b in r]
            assert max(sizes) - min(sizes) <= 1
    # config 5: half the streams cost 2434 B/sample (A2 Full), half 917.8 (A2 Lite), sorted by arch
    costs = [917.8] * 8192 + [2434.0] * 8192
    r = shard_ranges(costs, 8)
    loads = [sum(costs[a:b]) for a, b in r]
    assert max(loads) / (sum(loads) / 8) < 1.01


def test_a2_engine_selection_predicates(na):
    """NAMIsA2 (NeuralModel.cpp:159-168) and NAMIsA2Standard (:188-317), rule for rule, on accept / reject fixtures made from the
    reference's own A2 sample file."""
    from neuralaudio_amd import capi
    lib = capi.load_library()

    def classify(j):
        return lib.NA_DebugClassifyNam(json.dumps(j).encode())

    for v, want in (("0.5.4", 0), ("0.5.5", 1), ("0.6.0", 1), ("0.7.0", 1), ("1.0.0", 1), ("0.5.1", 0), ("0.4.9", 0)):
        assert classify({"version": v}) & 1 == want, v
    for sub in O.load_json("BossWN-a2.nam")["config"]["submodels"]:
        base = sub["model"]
        assert classify(base) == 3  # A2 version, standard architecture

        def variant(edit):
            j = copy.deepcopy(base)
            edit(j["config"]["layers"][0], j["config"], j)
            return classify(j) & 2

        assert variant(lambda lc, c, j: None) == 2
        rejects = [
            lambda lc, c, j: j.update(architecture="LSTM"),
            lambda lc, c, j: c.update(head={"x": 1}),
            lambda lc, c, j: c.update(condition_dsp=None),  # mere presence counts
            lambda lc, c, j: c.update(in_channels=2),
            lambda lc, c, j: c["layers"].append(copy.deepcopy(lc)),
            lambda lc, c, j: lc.update(input_size=2),
            lambda lc, c, j: lc.update(condition_size=2),
            lambda lc, c, j: lc.update(channels=4),
            lambda lc, c, j: lc.update(bottleneck=lc["channels"] + 1),
            lambda lc, c, j: lc["kernel_sizes"].__setitem__(3, 5),
            lambda lc, c, j: lc["dilations"].__setitem__(0, 2),
            lambda lc, c, j: lc["dilations"].append(1),
            lambda lc, c, j: lc["activation"].__setitem__(2, {"type": "Tanh"}),
            lambda lc, c, j: lc["activation"].__setitem__(2, {"type": "LeakyReLU", "negative_slope": 0.2}),
            lambda lc, c, j: lc["secondary_activation"].__setitem__(1, {"type": "Sigmoid"}),
            lambda lc, c, j: lc["gating_mode"].__setitem__(1, "gated"),
            lambda lc, c, j: lc["head"].update(out_channels=2),
            lambda lc, c, j: lc["head"].update(kernel_size=8),
            lambda lc, c, j: lc["head"].update(head_dilation=2),
            lambda lc, c, j: lc["head"].update(bias=False),
            lambda lc, c, j: lc["layer1x1"].update(active=False),
            lambda lc, c, j: lc["layer1x1"].update(groups=2),
            lambda lc, c, j: lc["head1x1"].update(active=True),
            lambda lc, c, j: lc["conv_pre_film"].update(active=True),
            lambda lc, c, j: lc["head1x1_post_film"].update(active=True),
            lambda lc, c, j: lc.pop("activation_pre_film"),  # the reference's IsActive(): a missing block counts as active
            lambda lc, c, j: lc.update(groups_input=2),
            lambda lc, c, j: lc.update(groups_input_mixin=4),
            lambda lc, c, j: lc.update(slimmable={"method": "x"}),
            lambda lc, c, j: lc.pop("head"),
        ]
        for k, edit in enumerate(rejects):
            assert variant(edit) == 0, k
        accepts = [
            lambda lc, c, j: lc["gating_mode"].__setitem__(1, None),
            lambda lc, c, j: lc["activation"].__setitem__(2, {"type": "LeakyReLU"}),  # default slope 0.01
            lambda lc, c, j: lc.pop("secondary_activation"),
            lambda lc, c, j: lc.pop("bottleneck"),
            lambda lc, c, j: lc.update(slimmable=None),
        ]
        for k, edit in enumerate(accepts):
            assert variant(edit) == 2, k
    for a1 in ("BossWN-standard.nam", "BossWN-nano.nam", "BossLSTM-1x16.nam"):
        assert classify(O.load_json(a1)) == 0


def _shard_ranges_in_python(costs, world_size):
    """NA_ShardByCost (csrc/multi_gpu.cpp) once more in plain Python: the test below compares the two."""
    n = len(costs)
    if world_size < 1:
        raise ValueError("world_size must be >= 1")
    total = float(sum(costs))
    ranges = []
    begin = 0
    acc = 0.0
    for rank in range(world_size):
        if rank == world_size - 1:
            end = n
        else:
            target = total * (rank + 1) / world_size
            end = begin
            while end < n and acc + costs[end] <= target + 1e-9:
                acc += costs[end]
                end += 1
            # at least one stream per rank while streams remain: take one even if it alone overshoots the share,
            # and leave one for each remaining rank
            cap = max(begin, n - (world_size - rank - 1))
            if end == begin and end < cap:
                end += 1
            end = min(end, cap)
            acc = float(sum(costs[:end]))
        ranges.append((begin, end))
        begin = end
    return ranges



def test_shard_by_cost_matches_the_python_restatement_and_covers_everything():
    """NA_ShardByCost (csrc/multi_gpu.cpp) is the partition both multi-GPU hosts use (the C++ NA_Multi* host and bench.py's
    one-process-per-GPU ranks through neuralaudio_amd.sharding): contiguous, ordered, disjoint, complete, near-equal cost, at least one
    item per range while items remain -- and identical to the plain-Python restatement."""
    import numpy as np
    from neuralaudio_amd.sharding import shard_ranges
    rng = np.random.default_rng(0)
    cases = [([1.0] * 8192, 8), ([41.6] * 4096 + [20.2] * 4096, 8), ([46.6] * 8192 + [71.4] * 8192, 8), ([1.0, 3.0, 1.0, 1.0, 2.0, 1.0, 1.0], 2),
             ([5.0], 4), ([], 3), ([0.0] * 10, 3), ([1.0] * 3, 8)]
    for _ in range(40):
        n = int(rng.integers(1, 400))
        cases.append((list(rng.choice([20.2, 33.7, 41.6, 71.4], size=n) * rng.uniform(0.5, 2.0)), int(rng.integers(1, 9))))
    for costs, parts in cases:
        got = shard_ranges(costs, parts)
        assert got == _shard_ranges_in_python(costs, parts), (costs[:8], parts, got)
        assert len(got) == parts and got[0][0] == 0 and got[-1][1] == len(costs)
        assert all(a <= b for a, b in got) and all(got[i][1] == got[i + 1][0] for i in range(parts - 1))
        if len(costs) >= parts:
            assert all(b > a for a, b in got), (parts, got)
    # balance: 8 ranks over config 5's global list (A2 ch3 then ch8): the ranks holding the expensive half get fewer streams
    costs = [46.6] * 8192 + [71.4] * 8192
    r = shard_ranges(costs, 8)
    loads = [sum(costs[a:b]) for a, b in r]
    assert max(loads) / min(loads) < 1.01 and (r[0][1] - r[0][0]) > (r[-1][1] - r[-1][0])


def test_stream_cost_estimates_rank_the_official_models(models_dir):
    import ctypes as C
    from neuralaudio_amd import capi
    lib = capi.load_library()
    loader = lib.CreateLoader()
    cost = {}
    for name in ("BossWN-standard.nam", "BossWN-feather.nam", "BossWN-nano.nam", "BossLSTM-1x16.nam", "BossLSTM-2x8.nam", "BossWN-a2.nam"):
        m = lib.NA_CreateModelFromFileUtf8(loader, os.path.join(models_dir, name).encode(), 0)
        assert m
        cost[name] = lib.NA_ModelStreamCost(m, C.c_float(1.0))
        if "a2" in name:
            cost["a2-lite"] = lib.NA_ModelStreamCost(m, C.c_float(0.0))
    assert cost["BossWN-standard.nam"] > cost["BossWN-feather.nam"] > cost["BossWN-nano.nam"] > 0
    assert cost["BossWN-a2.nam"] > cost["a2-lite"] > cost["BossLSTM-1x16.nam"] > 0
    assert 35.0 < cost["BossWN-standard.nam"] < 50.0 and 15.0 < cost["BossLSTM-1x16.nam"] < 25.0  # (us per 1024 streams x 128 frames)


def test_bench_cpu_baseline_legs_run(na):
    """bench.py's cpu_baseline leg (the oracle timed on the host cores: the only place outside tests / smoke() that may call it) for
    every kind of workload the bench line carries one for -- single models, the mixed batches, config 4's seeded recurrent models."""
    sys.path.insert(0, ROOT)
    import bench
    import numpy as np
    r = bench.cpu_baseline("standard", 0.2)
    assert r["value"] > 0 and r["kind"] == "port" and r["cores"] >= 1 and "MULTIFRAME_8X8" in r["sample"]
    assert bench.mixed_cpu_baseline(["a2lite", "a2full"], 0.3)["value"] > 0
    rng = np.random.default_rng(4)
    H, a = 8, 0.25
    lw = np.concatenate([rng.uniform(-a, a, 4 * H * (1 + H) + 4 * H + 2 * H), rng.uniform(-a, a, H + 1)])
    lstm = {"architecture": "LSTM", "config": {"input_size": 1, "hidden_size": H, "num_layers": 1}, "weights": [float(v) for v in lw]}
    gru = {"layers": [{"type": "gru", "shape": [None, None, H], "weights": [rng.uniform(-a, a, (1, 3 * H)).tolist(), rng.uniform(-a, a, (H, 3 * H)).tolist(),
                                                                              rng.uniform(-a, a, (2, 3 * H)).tolist()]},
                      {"type": "dense", "shape": [None, None, 1], "weights": [rng.uniform(-a, a, (H, 1)).tolist(), [0.0]]}]}
    assert bench.mixed_cpu_baseline([("lstm", lstm), ("gru", gru)], 0.3)["value"] > 0


def test_every_wide_fuzz_seed_loads(na):
    """tests/test_gpu_wide.py runs every seed of its architecture fuzz and every fixed case without a skip, so the generator must produce
    loadable shapes only -- proven here without a GPU -- and must reach what it is for: every channel count of the edge list, both
    orders of a wide array beside a narrower one, one to three arrays, both activations, conv heads, every kernel on both sides of 64."""
    loader = na.NeuralModelLoader()
    assert WC.NUM_FUZZ_SEEDS >= len(WC.EDGE_CHANNELS)
    seen, orders, counts, acts, kernels, conv_heads, ks, ds = set(), set(), set(), set(), set(), 0, set(), set()
    cases = [WC.fuzz_case(seed) for seed in range(WC.NUM_FUZZ_SEEDS)] + [(WC.fixed_case(c, act), None) for c, act in WC.FIXED_CASES]
    for arrays, sizes in cases:
        ch = [a["channels"] for a in arrays]
        assert max(ch) > 16 and 1 <= len(arrays) <= 3, ch
        for i, a in enumerate(arrays):
            assert a["head_size"] == (arrays[i + 1]["channels"] if i + 1 < len(arrays) else 1)
        w = O.synth_wavenet_weights(arrays, seed=1)
        m = loader.CreateFromString(O.nam_json_wavenet_generic(arrays, w), ".nam", doPrewarm=False)
        assert m is not None, arrays
        info = m.KernelInfo(1.0, 1)
        assert info["kernel"] == "generic" and info["weights_ok"] and 8.0 <= info["input_limit"] <= 32752.0, (arrays, info)
        assert m.GetReceptiveFieldSize() == sum((k - 1) * d for a in arrays for k, d in zip(a["kernel_sizes"], a["dilations"])) + \
            (arrays[-1]["head_kernel_size"] - 1) * arrays[-1]["head_dilation"]
        if sizes is None:
            continue
        assert sizes[:3] == [1, 1, 17] and sum(sizes) == WC.FUZZ_SAMPLES and WC.fuzz_work(arrays) <= WC.FUZZ_WORK_CAP
        seen.update(ch)
        counts.add(len(arrays))
        acts.add(arrays[0]["activation"])
        kernels.add(WC.max_channels(arrays) > 64)
        conv_heads += arrays[-1]["head_kernel_size"] > 1
        for a in arrays:
            ks.update(a["kernel_sizes"])
            ds.update(a["dilations"])
        for a, b in zip(ch, ch[1:]):
            if max(a, b) > 16 and a != b:
                orders.add("wide->narrow" if a > b else "narrow->wide")
    assert seen >= set(WC.EDGE_CHANNELS), sorted(set(WC.EDGE_CHANNELS) - seen)
    assert orders == {"wide->narrow", "narrow->wide"} and counts == {1, 2, 3} and acts == {O.ACT_TANH, O.ACT_LEAKYRELU}
    assert kernels == {False, True} and conv_heads >= 1 and ks == set(WC.KERNEL_SIZES) and ds == set(WC.DILATIONS)


def test_wide_range_tests_stand_on_the_side_of_the_f16_boundary_they_claim(na):
    """The range-contract tests of tests/test_gpu_wide.py call some inputs "inside" and some "outside" the f16 range of the split
    operands.  A float64 evaluation (ref_np.wavenet_forward, peaks of the residual stream h, the activations z and the head accumulator)
    says which is which: the hot inputs stay under 32 752 (half the range: what the static proof allows), the loud ones exceed 65 504
    -- also after the kernel's own clamp at the model's input limit, which is what the chain then sees -- and the reference's output
    is finite either way (its f32 chain holds 3e38)."""
    loader = na.NeuralModelLoader()
    noise = O.signal_noise(1024, 5)
    for name in ("32/8 tanh", "128/64 tanh", "24/12 leaky", "128/128 leaky"):
        arrays, w = WC.range_model(name)
        limit = loader.CreateFromString(O.nam_json_wavenet_generic(arrays, w), ".nam", doPrewarm=False).KernelInfo(1.0, 1)["input_limit"]
        for amp in (30.0, 1000.0, 10000.0):
            x = (amp * noise).astype(np.float32)
            assert np.abs(x).max() < limit, (name, amp, limit)  # nothing is clamped
            peaks = {}
            y, _ = ref_np.wavenet_forward(arrays, w, x, peaks=peaks)
            assert max(peaks.values()) < WC.SPLIT_SAFE and np.all(np.isfinite(y)), (name, amp, peaks)
        loud = 1e5 if "tanh" in name else 6e4
        for clamp in (np.inf, limit):
            peaks = {}
            y, _ = ref_np.wavenet_forward(arrays, w, (loud * noise).astype(np.float32).clip(-clamp, clamp), peaks=peaks)
            assert np.all(np.isfinite(y)), name
            if clamp == np.inf or "leaky" in name:  # (a proven tanh model is inside the range once its input is clamped: that is the proof)
                assert max(peaks.values()) > WC.F16_MAX, (name, loud, clamp, peaks)
            else:
                assert max(peaks.values()) < WC.SPLIT_SAFE, (name, loud, clamp, peaks)


@pytest.mark.parametrize("name", ["32/8 tanh", "80/72 tanh"])
def test_wide_models_outside_the_operand_format_fail_at_load(na, name):
    """Layer arrays wider than 16 channels have no f32 kernel: a model whose weights do not fit the (hi, lo) f16 operands, or whose tanh
    layers can add more than the f16 range holds, is a load error that names the reason (narrow models with the same weights load and
    run on the f32 frame kernel: test_models_without_a_range_proof_run_on_the_f32_kernel)."""
    loader = na.NeuralModelLoader()
    arrays, w = WC.range_model(name)
    m = loader.CreateFromString(O.nam_json_wavenet_generic(arrays, w), ".nam", doPrewarm=False)
    info = m.KernelInfo(1.0, 1)
    assert info["kernel"] == "generic" and info["range_proven"] and info["weights_ok"] and 8.0 <= info["input_limit"] <= 32752.0
    expect = {"mix-in x 1e5": "weights do not fit", "1x1 x 4000": "no input limit of at least 8", "all x 1e-3": "weights do not fit"}
    for case, factors in WC.WEIGHT_SCALINGS.items():
        ws = O.scale_wavenet_tensors(arrays, w, factors)
        with pytest.raises(na.NeuralAudioError, match=expect[case]):
            loader.CreateFromString(O.nam_json_wavenet_generic(arrays, ws), ".nam", doPrewarm=False)


# ---- the runtime-shaped recurrent kernel's test shapes (tests/recurrent_cases.py, run by tests/test_gpu_recurrent_rt.py) --------------

def _recurrent_knob_free():
    if RC.knob_set():
        pytest.skip("a recurrent tuning knob is set: the plan is not the default one")


@pytest.mark.parametrize("c", RC.edge_cases(), ids=RC.case_id)
def test_every_recurrent_case_loads_and_sits_in_the_regime_it_is_named_for(na, c):
    """Without a GPU: the loader takes the case, and NA_DebugRecurrentPlan -- the plan the launcher reads -- says that it runs on the
    runtime-shaped kernel with the wave count, rows per lane, weight path and head placement the case was generated for; at an edge
    h - 1 | h the named field differs between the two sides."""
    _recurrent_knob_free()
    m = RC.Built(c).load(na)
    p = m.RecurrentPlan()
    assert p["runs"] and {f: int(p[f]) for f in RC.FIELDS} == c["regime"], (RC.case_id(c), p)
    assert p["lds_bytes"] <= 160 * 1024
    gate_rows = (3 if c["kind"] == "gru" else 4) * c["hidden"]
    assert p["rows_per_lane"] == -(-gate_rows // (64 * p["waves"])) and (p["waves"] == 16 or p["rows_per_lane"] == 1)
    assert p["head_in_loop"] == (c["hidden"] >= 129)
    if " edge " in c["why"]:
        field, _, pair = c["why"].split(" ")
        lo, hi = (int(v) for v in pair.split("|"))
        assert RC.regime(c["kind"], lo, c["layers"])[field] != RC.regime(c["kind"], hi, c["layers"])[field], c["why"]
    m.close()


def test_recurrent_cases_reach_every_regime_of_the_kernel(na):
    """The set of cases (the keras stacks with tails included) reaches every wave count, every rows-per-lane count a cell type can have
    (a GRU has 3 x 1024 gate rows at most: three per lane), both weight paths on one and on several waves, both head placements and
    every H % 4 on both weight paths, for both cell types; the tail stacks load and sit where tests/test_gpu_recurrent_rt.py expects."""
    _recurrent_knob_free()
    import json
    regimes = [(c["kind"], c["hidden"], c["regime"]) for c in RC.edge_cases()]
    for spec in RC.TAIL_STACKS:
        kind, hidden = RC.stack_dims(spec)[:2]
        regimes.append((kind, hidden, RC.stack_regime(spec)))
        m = na.NeuralModelLoader().CreateFromString(json.dumps(ref_np.synth_keras_stack(spec, seed=40 + len(spec))), ".json", doPrewarm=False)
        assert m is not None and m.RecurrentPlan()["runs"], spec
        assert {f: int(m.RecurrentPlan()[f]) for f in RC.FIELDS} == RC.stack_regime(spec), spec
    for kind in ("lstm", "gru"):
        mine = [(h, r) for k, h, r in regimes if k == kind]
        assert {r["waves"] for _, r in mine} == {1, 2, 4, 8, 16}, kind
        assert {r["rows_per_lane"] for _, r in mine} == ({1, 2, 3, 4} if kind == "lstm" else {1, 2, 3}), kind
        assert {r["head_in_loop"] for _, r in mine} == {0, 1}, kind
        for l2w in (0, 1):
            assert {h % 4 for h, r in mine if r["l2w"] == l2w} == {0, 1, 2, 3}, (kind, l2w)
            assert any(r["waves"] > 1 and r["l2w"] == l2w for _, r in mine), (kind, l2w)
    both = [r for _, _, r in regimes]
    assert {(r["waves"] == 1, r["l2w"]) for r in both} == {(True, 0), (True, 1), (False, 0), (False, 1)}
    # the shapes of the batch / snapshot / pool / level tests are multi-wave shapes of this kernel
    for kind, layers, hidden in RC.BATCH_SHAPES + RC.SNAPSHOT_SHAPES + RC.POOL_SHAPES + RC.LEVEL_SHAPES + [("lstm", 1, 40)]:
        p = RC.shape_plan(kind, hidden, layers)
        assert p["runs"] and p["waves"] > 1, (kind, layers, hidden)
    assert RC.shape_plan("lstm", 64, 2)["l2w"] and RC.shape_plan("lstm", 257, 1)["rows_per_lane"] == 2
    # call sizes: n = 1 and a call above LSTM_MAX_FRAMES in every partition
    for samples in (150, 300):
        sizes = RC.call_sizes(samples, 1)
        assert sum(sizes) == samples and sizes[0] == 1 and max(sizes) > 128 and set(sizes) <= set(RC.CALL_SIZES) | {sizes[-1]}
    # eight rows per lane forced: the LSTMs of 613, 769 and 1024 units reach dispatch cases 5, 7 and 8
    assert [na.recurrent_shape_plan("lstm", h, 1, rpl=8, force_l2w=0)["rows_per_lane"] for h in (613, 769, 1024)] == [5, 7, 8]
    # the widest recurrent layer with a dense tail: admitted, and the next one up is not
    for kind in ("lstm", "gru"):
        h = RC.widest_with_dense_tail(kind)
        assert RC.shape_plan(kind, h, 1, 2, RC.TAIL_DENSE, 0)["admitted"] and not RC.shape_plan(kind, h + 1, 1, 2, RC.TAIL_DENSE, 0)["admitted"]


HEADROOM_CASES = [c for c in RC.edge_cases() if c["hidden"] <= 256 or (c["kind"], c["hidden"]) in (("lstm", 513), ("gru", 342))]


@pytest.mark.parametrize("c", HEADROOM_CASES, ids=RC.case_id)
def test_recurrent_oracle_keeps_its_headroom_under_the_gpu_bound(c):
    """The GPU tests hold the kernel to 5e-6 * max(1, rms(want)) against the C oracle: the oracle (float32) itself is within a tenth of
    that bound of the float64 restatement at unit amplitude and within a quarter at amplitude 1000, so the bound measures the kernel.
    (Above 256 units: one LSTM and one GRU, to keep CPU time down.)"""
    b = RC.Built(c)
    for amp, share in ((1.0, 0.1), (1000.0, 0.25)):
        x = RC.signal(c, amp)
        got, want = b.oracle().process(x), b.f64(x)
        err = O.rms(got - want)
        print("%s amplitude %g: oracle-float64 rms %.3g, bound %.3g" % (RC.case_id(c), amp, err, RC.bound(want)))
        assert np.all(np.isfinite(got)) and err <= share * RC.bound(want), (RC.case_id(c), amp, err, RC.bound(want))


# ---- the keras-stack tails' test shapes (tests/tail_cases.py, run by tests/test_gpu_tails.py) -------------------------------------------
# These checks are what makes the GPU bound of that file mean something: a case's output depends on its input, float32 arithmetic alone
# stays far below the bound, and a checker with a wrong tap, a wrong dilation or no softmax would be off by a hundred bounds.

_tail_walks = {}


def _tail_walk(c, amp=1.0, zero=False, dtype=np.float64):
    """The restatement's walk of a case (its own signal at `amp`, or zeros of that length): computed once, shared, never changed."""
    key = (c["name"], amp, zero, dtype)
    if key not in _tail_walks:
        x = TC.signal(c, amp)
        w = TC.Built(c).f64(np.zeros_like(x) if zero else x, dtype=dtype)
        w.setflags(write=False)
        _tail_walks[key] = w
    return _tail_walks[key]


@pytest.mark.parametrize("c", TC.cases(), ids=TC.case_id)
def test_every_tail_case_loads_and_runs_where_it_is_listed(na, c):
    """Without a GPU: the loader takes the case, the plan of the loaded model is the plan of the dimensions tests/tail_cases.py lowers
    the stack to (so the sizes read from the shape predicate mean what the table says), the decision function names the kernel and the
    plan the regime the case is listed for, and the call partition holds every size it must."""
    _recurrent_knob_free()
    m = TC.Built(c).load(na, prewarm=False)
    p, sp, runs = m.RecurrentPlan(), TC.plan(c["spec"]), c["runs"]
    assert sp["admitted"] and {k: p[k] for k in p} == {k: sp[k] for k in p}, (c["name"], p, sp)
    assert p["lds_bytes"] <= 160 * 1024
    assert na.recurrent_kernel(*TC.dims(c["spec"])) == runs["kernel"] == "RecurrentWaveRtKernel" and p["runs"], (c["name"], p)
    assert not p["head_in_loop"], "a tail is evaluated behind the block"
    if "waves" in runs:
        assert (p["waves"] == 1) == (runs["waves"] == "one"), (c["name"], p)
    if "l2w" in runs:
        assert int(p["l2w"]) == runs["l2w"], (c["name"], p)
    if "tail_layers" in runs:
        assert len(TC.lowered(c["spec"])) == runs["tail_layers"], c["name"]
    assert (TC.history(c["spec"]) > 0) == (c["form"] == "conv") and c["hist"] == TC.history(c["spec"])
    # under the knobs that force the lane = stream kernels a conv1d tail stays where it is, a dense tail moves or has no kernel
    for knob in ("NA_LSTM_NO_WAVE_RT", "NA_LSTM_LANE_KERNEL"):
        forced = na.recurrent_kernel(*TC.dims(c["spec"]), knobs=(knob,))
        if c["form"] == "conv":
            assert forced == "RecurrentWaveRtKernel", (c["name"], knob, forced)
        elif knob == "NA_LSTM_NO_WAVE_RT" or TC.dims(c["spec"])[0] == "lstm":
            assert forced in ("", "LstmGenericKernel", "GruGenericKernel"), (c["name"], knob, forced)
    sizes = TC.Built(c).sizes()
    assert sum(sizes) == c["samples"] >= 3 * c["hist"] + 300 and sizes[:4] == [1, 1, 2, 3] and max(sizes) > TC.MAX_FRAMES
    assert set(TC.FIXED_CALLS) <= set(sizes)
    if c["form"] == "conv":
        assert {h for h in (c["hist"] - 1, c["hist"], c["hist"] + 1) if 1 <= h <= 300} <= set(sizes), (c["name"], sizes)
    m.close()


@pytest.mark.parametrize("c", TC.refused_cases(), ids=TC.case_id)
def test_every_tail_shape_beyond_a_limit_is_refused_by_name(na, c):
    with pytest.raises(na.NeuralAudioError, match=c["refused"]):
        na.NeuralModelLoader().CreateFromString(TC.Built(c).doc, ".json", doPrewarm=False)


def test_tail_cases_reach_every_path_of_the_tails(na):
    """The set of cases reaches both tail forms, a tail without and behind recurrent layers, conv1d histories below, at and above
    LSTM_MAX_FRAMES and at the limit, one-wave and multi-wave shapes, gate weights in LDS and streamed from L2, every activation code in
    both forms, and the sizes read from the shape predicate are edges of it."""
    _recurrent_knob_free()
    cs = TC.cases()
    plans = {c["name"]: TC.plan(c["spec"]) for c in cs}
    for form in ("conv", "dense"):
        mine = [c for c in cs if c["form"] == form]
        assert {len(TC.recurrent(c["spec"])) > 0 for c in mine} == {False, True}, form                 # Hin == 0 and Hin > 0
        assert {TC.dims(c["spec"])[0] for c in mine if TC.recurrent(c["spec"])} == {"lstm", "gru"}, form
        assert {plans[c["name"]]["waves"] == 1 for c in mine} == {False, True}, form
        assert {bool(plans[c["name"]]["l2w"]) for c in mine} == {False, True}, form
        acts = set()
        for c in mine:
            for l in TC.scaled_stack(c["spec"], c["seed"])["layers"]:
                if l["type"] in ("dense", "conv1d", "activation"):
                    acts.add(l.get("activation") or "linear")
        assert acts >= {"linear", "tanh", "relu", "sigmoid", "elu", "softmax"}, (form, acts)
    hists = {c["hist"] for c in cs if c["form"] == "conv"}
    assert {TC.MAX_FRAMES - 1, TC.MAX_FRAMES, TC.MAX_FRAMES + 1, TC.max_history()} <= hists and min(hists) < 64
    assert (True, 1) in {(plans[c["name"]]["waves"] == 1, int(plans[c["name"]]["l2w"])) for c in cs if c["form"] == "conv"}  # one wave, streamed
    widths = set()
    for c in cs:
        if c["form"] == "dense":
            widths |= {t[1] for t in TC.lowered(c["spec"])}
    assert widths >= {1, 63, 64, 65, 256}
    assert any(len(TC.lowered(c["spec"])) == 8 for c in cs)
    # a layer whose history is shorter than the longest of its tail, in front of and behind the longest
    orders = [[(t[2] - 1) * t[3] for t in TC.lowered(c["spec"]) if t[2] > 1] for c in cs if c["form"] == "conv"]
    assert any(len(o) == 3 and o[1] < o[2] < o[0] for o in orders) and any(len(o) == 3 and o[1] < o[0] < o[2] for o in orders)
    assert any(TC.lowered(c["spec"])[0][2] == 1 and TC.history(c["spec"]) > 0 and not TC.recurrent(c["spec"]) for c in cs)  # dense first, conv behind
    # the sizes read from the shape predicate are its edges
    assert TC.max_history() == 1024 and not RC.shape_plan("lstm", 1, 0, 1, 1, TC.max_history() + 1)["admitted"]
    for kind in ("lstm", "gru"):
        w = TC.widest_conv_input(kind)
        assert plans["conv-widest-" + kind]["waves"] > 1 and not TC.plan(TC._conv_probe(kind, w + 1, 2, 1))["admitted"]
    wh = TC.dims(TC.by_name("conv-hist-limit")["spec"])[1]
    assert TC.plan(TC._conv_probe("lstm", wh, 3, 512))["admitted"] and not TC.plan(TC._conv_probe("lstm", wh + 1, 3, 512))["admitted"]
    # the cases of the batch tests: a short history for the growth test, conv1d tails where one is asked for, softmax in the lane cases
    assert [TC.by_name(n)["form"] for n in TC.GROWTH_CASES] == ["conv", "dense"] and TC.by_name(TC.GROWTH_CASES[0])["hist"] <= 64
    assert TC.by_name(TC.LEAVE_JOIN_CASE)["form"] == "conv"
    assert [TC.by_name(n)["form"] for n in TC.MIXED_CASES] == ["conv", "conv", "dense"]
    assert [TC.by_name(n)["form"] for n in TC.IN_PLACE_CASES] == ["conv", "dense"] and not TC.recurrent(TC.by_name(TC.IN_PLACE_CASES[0])["spec"])
    for n in TC.LANE_CASES:
        c = TC.by_name(n)
        assert c["form"] == "dense" and any(len(l) > 2 and l[2] == "softmax" for l in c["spec"])
        assert na.recurrent_kernel(*TC.dims(c["spec"]), knobs=("NA_LSTM_NO_WAVE_RT",)) in ("LstmGenericKernel", "GruGenericKernel"), n
    assert {TC.dims(TC.by_name(n)["spec"])[0] for n in TC.LANE_CASES} == {"lstm", "gru"}


@pytest.mark.parametrize("c", TC.cases(), ids=TC.case_id)
def test_tail_case_output_depends_on_its_input(c):
    """The signal path: rms(want - want for a zero input) is at least 0.1 and at least a fifth of rms(want).  A condition, not a
    measurement: a case that misses it gets another gain in tests/tail_cases.py."""
    want, zero = _tail_walk(c), _tail_walk(c, zero=True)
    path = O.rms(want - zero)
    print("%-28s rms(want) %.3g, rms(want - zero-input want) %.3g" % (c["name"], O.rms(want), path))
    assert path >= 0.1 and path >= 0.2 * O.rms(want), (c["name"], path, O.rms(want))


@pytest.mark.parametrize("c", TC.cases(), ids=TC.case_id)
def test_float32_walk_of_a_tail_case_keeps_its_headroom_under_the_gpu_bound(c):
    """The restatement walked in float32 (weights, state, input and constants) is within a quarter of the GPU bound of the float64 walk at
    amplitudes 1 and 1000: the bound measures the kernel, not the number format."""
    for amp in (1.0, 1000.0):
        want, got = _tail_walk(c, amp), _tail_walk(c, amp, dtype=np.float32)
        err = O.rms(got - want)
        print("%-28s amplitude %g: float32-float64 rms %.3g, bound %.3g (%.3f of it)" % (c["name"], amp, err, TC.bound(want), err / TC.bound(want)))
        assert got.dtype == np.float32 and np.all(np.isfinite(got)) and err <= 0.25 * TC.bound(want), (c["name"], amp, err, TC.bound(want))


@pytest.mark.parametrize("c", TC.cases(), ids=TC.case_id)
def test_a_wrong_tap_dilation_or_softmax_would_be_noticed_on_a_tail_case(c):
    """Each mutant of the restatement, one at a time -- the oldest tap of a conv1d layer reads zeros, its dilation is one larger, softmax
    is the identity -- is off by at least 100 bounds on every case it applies to."""
    b, x, want = TC.Built(c), TC.signal(c), _tail_walk(c)
    muts = TC.mutants(b.mj)
    assert muts or c["form"] == "dense"
    for name, mj in muts:
        off = O.rms(b.f64(x, mj=mj) - want) / TC.bound(want)
        print("%-28s %-32s off by %.0f bounds" % (c["name"], name, off))
        assert off >= 100.0, (c["name"], name, off)


def test_keras_stack_walk_is_in_float64_unless_asked_otherwise():
    """The walk's default type is float64 -- asking for it by name changes no bit -- and float32 is held all the way through."""
    mj = ref_np.synth_keras_stack([("gru", 12), ("conv1d", 16, 4, 64, "elu"), ("batchnorm", 16, "noaffine"), ("dense", 5, "softmax"), ("dense", 1)], seed=8)
    x = O.signal_noise(200, 3)
    a, b = ref_np.keras_stack_forward(mj, x, prewarm=64), ref_np.keras_stack_forward(mj, x, prewarm=64, dtype=np.float64)
    assert a.dtype == np.float64 and np.array_equal(a, b)
    assert ref_np.keras_stack_forward(mj, x, prewarm=64, dtype=np.float32).dtype == np.float32


# ---- the f32 frame kernel's test shapes (tests/frame_cases.py, run by tests/test_gpu_frame.py) -------------------------------------------

def _frame_cases():
    fuzz = [FC.fuzz_case(seed) for seed in range(FC.NUM_FUZZ_SEEDS)]
    batch = [FC.small_k2_model()] + FC.table_models() + FC.fused_models() + [FC.lds_model(k) for k in (62, 63, 70)]
    return FC.named_cases(), fuzz, batch


def test_every_frame_case_loads_and_is_predicted_on_the_frame_kernel(na):
    """tests/test_gpu_frame.py runs every case without a skip and asserts the kernel's name before it trusts a comparison, so every
    generated shape must load and land on the f32 frame kernel by default -- at one stream and at 600, so neither packing nor padding
    takes it away -- with no input limit, and with the receptive field its layers add up to."""
    loader = na.NeuralModelLoader()
    named, fuzz, batch = _frame_cases()
    names = [c["name"] for c in named + [c for c, _ in fuzz] + batch]
    assert len(set(names)) == len(names)
    for case in named + [c for c, _ in fuzz] + batch:
        arrays = case["arrays"]
        assert max(max(a["channels"], a["head_size"], a["input_size"]) for a in arrays) <= 16 and 1 <= len(arrays) <= 2, case["name"]
        assert all(1 <= len(a["kernel_sizes"]) <= (4 if case["family"] != "no range proof" else 13) for a in arrays), case["name"]
        assert case["rule"] in (FC.RULE_F32, FC.RULE_F64) and (case["rule"] == FC.RULE_F64) == bool(case["scale"]), case["name"]
        m = loader.CreateFromString(O.nam_json_wavenet_generic(arrays, FC.weights(case)), ".nam", doPrewarm=False)
        assert m is not None, case["name"]
        for streams in (1, 600):
            info = m.KernelInfo(1.0, streams)
            assert info["kernel"] == "frame" and info["pack"] == 1 and info["input_limit"] == float("inf"), (case["name"], streams, info)
        assert m.GetReceptiveFieldSize() == FC.receptive_field(arrays), case["name"]
        assert FC.work(arrays, case["samples"]) <= FC.WORK_CAP, case["name"]
    for case, sizes in fuzz:
        assert sizes[:3] == [1, 1, 17] and sum(sizes) == FC.SAMPLES == case["samples"], case["name"]
        assert set(sizes) & {31, 63, 64, 65, 127, 128} and max(sizes) > FC.BLOCK, (case["name"], sizes)
    for case in named + [c for c, _ in fuzz]:  # every ring wraps at least twice
        longest = max(FC.ring_frames((k - 1) * d) for a in case["arrays"] for k, d in zip(a["kernel_sizes"], a["dilations"]))
        assert case["samples"] >= 2 * max(longest, FC.ring_frames(case["arrays"][-1]["head_kernel_size"] - 1)), (case["name"], longest)


def test_frame_cases_reach_every_path_of_the_kernel_they_name():
    """The named cases alone -- and the seeded draw once more -- reach: every channel-group count, partially filled groups, both
    activations, one and two arrays with equal and with different G across the link, conv heads on both sides of the reach that picks
    HeadConvLds or HeadConvPk (with and without a bias, every head G), staged blocks on both sides of the stager's 384 and 512 float4,
    kernel sizes on both sides of the wide prefetch depth at G <= 2 and at G >= 3, tap shifts on both sides of 64 and of 128 frames, a
    K = 1 layer, and a model without the range proof."""
    named, fuzz, _ = _frame_cases()

    def reach(cases):
        r = dict(G=set(), partial=set(), acts=set(), arrays=set(), link=set(), head=set(), blocks=set(), taps=set(), shifts=set(), ks=set(), rules=set())
        for c in cases:
            arrays = c["arrays"]
            r["arrays"].add(len(arrays))
            r["rules"].add(c["rule"])
            if len(arrays) == 2:
                r["link"].add(FC.groups(arrays[0]["channels"]) == FC.groups(arrays[1]["channels"]))
            last = arrays[-1]
            if last["head_kernel_size"] > 1:
                r["head"].add((last["head_kernel_size"] - 1 <= FC.HEAD_SHORT_REACH, FC.groups(last["channels"]), bool(last["has_head_bias"])))
            maxk = max(k for a in arrays for k in a["kernel_sizes"])
            for a in arrays:
                g = FC.groups(a["channels"])
                r["G"].add(g)
                r["partial"].add((g, a["channels"] % 4 != 0))
                r["acts"].add(a["activation"])
                for k in a["kernel_sizes"]:
                    r["ks"].add(k)
                    f4 = FC.layer_block_f4(k, a["channels"])
                    r["blocks"].add((f4 > FC.STAGER_F4, f4 > FC.STAGER_F4_SPB))
                    if maxk > 3:  # (the kernel's `wide`: a model with a K > 3 requests five taps ahead in its G <= 2 runs)
                        r["taps"].add((g <= 2, (k - 1 > FC.HPF_WIDE) - (k - 1 < FC.HPF_WIDE)))
            r["shifts"].update(FC.layer_shifts(arrays))
        return r

    for what, r in (("named", reach(named)), ("fuzz", reach([c for c, _ in fuzz]))):
        assert r["G"] == {1, 2, 3, 4} and r["acts"] == {O.ACT_TANH, O.ACT_LEAKYRELU} and r["arrays"] == {1, 2} and r["link"] == {True, False}, (what, r)
        assert {p for p in r["partial"] if p[1]} == {(g, True) for g in (1, 2, 3, 4)}, (what, r["partial"])
        assert {h[0] for h in r["head"]} == {True, False}, (what, r["head"])
        assert {(False, False), (True, False), (True, True)} <= r["blocks"], (what, r["blocks"])
        assert {(wide, side) for wide in (True, False) for side in (-1, 0, 1)} <= r["taps"], (what, r["taps"])
        for edge in (64, 128):
            assert any(s < edge for s in r["shifts"]) and edge in r["shifts"] and any(edge < s < edge + 64 for s in r["shifts"]), (what, edge, r["shifts"])
        assert 1 in r["ks"], (what, r["ks"])
    r = reach(named)
    assert r["rules"] == {FC.RULE_F32, FC.RULE_F64}
    assert {h[:2] for h in r["head"]} == {(s, g) for s in (True, False) for g in (1, 2, 3, 4)}, r["head"]  # both head kernels at every head G ...
    assert {(h[0], h[2]) for h in r["head"]} == {(s, b) for s in (True, False) for b in (True, False)}, r["head"]  # ... with and without bias
    assert {c["arrays"][0]["channels"] for c in named if c["family"] == "g sweep" and len(c["arrays"]) == 1} == set(FC.CHANNELS)
    assert set(FC.layer_shifts([a for c in named if c["family"] == "tap shifts" for a in c["arrays"]])) >= {d * m for d in FC.SHIFT_DILATIONS for m in (1, 2, 3)}


def test_frame_kernel_lds_limit_is_decided_at_load(na, tmp_path):
    """frame_lds.h is the one place that sizes the LDS of a frame-kernel launch (block images + two staged weight blocks of the launch's
    largest layer + the optional history buffers, against the 160 KB of a gfx950 workgroup).  16 channels: K = 62 fits two streams per
    workgroup (162 176 bytes) and K = 63 does not (164 224) -- the launcher then takes one; K = 70 fits one stream with 128-frame blocks
    (162 176) and K = 71 only 64-frame blocks (156 032 against 164 224): such a model could not run a buffer of more than 64 frames, and
    is refused when it loads, with the layer and its kernel size in the message."""
    exe = tmp_path / "frame_lds_cases"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "neuralaudio_amd", "csrc"),
                    os.path.join(ROOT, "tests", "frame_lds_cases.cpp"), "-o", str(exe)], check=True)
    rows = [(16, 62, 2, 2, 1), (16, 63, 2, 2, 1), (16, 63, 2, 1, 1), (16, 70, 2, 1, 1), (16, 71, 2, 1, 1), (16, 71, 1, 1, 0), (16, 70, 2, 1, 2),
            (16, 3, 2, 4, 1), (16, 3, 1, 1, 0), (4, 23, 2, 1, 1)]
    text = "".join(" ".join(map(str, r)) + "\n" for r in rows)
    out = [tuple(int(v) for v in line.split()) for line in subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.splitlines()]
    assert len(out) == len(rows)
    got = {r: o for r, o in zip(rows, out)}
    for r, o in got.items():  # the formula of the issue, restated: images + two weight buffers (at least what the stager writes) + history buffers
        c, k, wps, spb, pf = r
        g = (c + 3) // 4
        floats = (k + 1) * 64 * g + 12 * g
        stride = max((floats + 3) // 4, 384 if wps * spb <= 2 else 512)
        lds = spb * 2 * wps * 4 * 64 * 16 + 2 * stride * 16 + (wps * spb * 2 * 4 * 64 * 16 if pf == 2 else 0)
        assert o[:4] == (floats, stride, lds, int(lds <= 160 * 1024)), (r, o)
    assert got[(16, 62, 2, 2, 1)][2:4] == (162176, 1) and got[(16, 63, 2, 2, 1)][2:4] == (164224, 0) and got[(16, 63, 2, 1, 1)][3] == 1
    assert got[(16, 70, 2, 1, 1)][2:5] == (162176, 1, 1) and got[(16, 71, 2, 1, 1)][2:5] == (164224, 0, 0) and got[(16, 71, 1, 1, 0)][2:4] == (156032, 1)
    assert got[(16, 70, 2, 1, 2)][3] == 0  # (the LDS history buffers of NA_FR_PF=2 give way: the launcher falls back to registers)
    assert got[(16, 70, 2, 1, 1)][5] == 70 and got[(16, 3, 2, 4, 1)][2:4] == (4 * 16384 + 2 * 512 * 16, 1) and got[(16, 3, 1, 1, 0)][2] == 8192 + 2 * 384 * 16
    loader = na.NeuralModelLoader()
    for k in (62, 63, 70):
        case = FC.lds_model(k)
        assert loader.CreateFromString(O.nam_json_wavenet_generic(case["arrays"], FC.weights(case)), ".nam", doPrewarm=False) is not None
    case = FC.lds_model(71)
    with pytest.raises(na.NeuralAudioError, match=r"layer array 0, layer 0: kernel size 71 at 16 channels needs 164224 bytes of LDS.*largest kernel size at this width is 70"):
        loader.CreateFromString(O.nam_json_wavenet_generic(case["arrays"], FC.weights(case)), ".nam", doPrewarm=False)
    # the limit follows the width: a second array of 4 channels may use a kernel size no 16-channel array may
    arrays = FC.chain([16, 4], [([2], [1]), ([71], [1])], O.ACT_TANH)
    assert loader.CreateFromString(O.nam_json_wavenet_generic(arrays, O.synth_wavenet_weights(arrays, seed=3)), ".nam", doPrewarm=False) is not None


# ---- the f16-split interpreter's test shapes (tests/split_cases.py, run by tests/test_gpu_split.py) --------------------------------------

def _split_cases():
    return SC.named_cases(), [SC.fuzz_case(seed) for seed in range(SC.NUM_FUZZ_SEEDS)], SC.batch_models()


def test_every_split_case_loads_and_is_predicted_on_the_split_kernel_in_the_layout_it_claims(na):
    """tests/test_gpu_split.py runs every case without a skip and asserts kernel name and pack factor before it trusts a comparison, so
    every generated shape must load and land on the f16-split kernels by default, at one stream and at 600, with the pack factor it
    claims, a proven range, weights that fit the operand format, a finite input limit above the +-1 the signals are clipped to, and the
    receptive field its layers add up to.  NA_ModelKernelInfo does not name the layout: the claim is split_cases.layout_of, the Python
    restatement of the plan's rule, and what the library adds is that such a model runs on the split kernels at all -- a model that
    neither fills its lane modes nor is padded or packed has no fast plan and runs on the frame kernel.  The decision edges next to the
    table land there."""
    loader = na.NeuralModelLoader()
    named, fuzz, batch = _split_cases()
    every = named + [c for c, _ in fuzz] + batch
    names = [c["name"] for c in every]
    assert len(set(names)) == len(names)
    for case in every:
        arrays = case["arrays"]
        assert max(max(a["channels"], a["head_size"], a["input_size"]) for a in arrays) <= 16 and 1 <= len(arrays) <= 3, case["name"]
        assert all(1 <= len(a["kernel_sizes"]) <= (4 if case["name"] != "rings-63" else 63) for a in arrays), case["name"]
        assert case["layout"] in ("plain", "padded", "packed") and (case["pack"] > 1) == (case["layout"] == "packed"), case["name"]
        m = loader.CreateFromString(O.nam_json_wavenet_generic(arrays, SC.weights(case)), ".nam", doPrewarm=False)
        assert m is not None, case["name"]
        for streams in (1, 600):
            info = m.KernelInfo(1.0, streams)
            assert info["kernel"] == "f16-split" and info["pack"] == case["pack"] and info["range_proven"] and info["weights_ok"], (case["name"], streams, info)
            assert 1.0 < info["input_limit"] < float("inf"), (case["name"], info)
        assert m.GetReceptiveFieldSize() == SC.receptive_field(arrays), case["name"]
        assert SC.work(arrays, case["samples"]) <= SC.WORK_CAP, case["name"]
        assert SC.num_rings(arrays) <= SC.MAX_SPLIT_RINGS, case["name"]
        firsts = [(d, i == 0) for a in arrays for i, d in enumerate(a["dilations"])]
        assert case["samples"] >= 2 * max(SC.ring_frames(d, f) for d, f in firsts), case["name"]  # every ring wraps at least twice
    for case, sizes in fuzz:
        assert sizes[:3] == [1, 1, 17] and sum(sizes) == SC.SAMPLES == case["samples"], case["name"]
        assert set(sizes) & {31, 63, 64, 65, 127, 128} and max(sizes) > SC.BLOCK, (case["name"], sizes)
    by_name = {c["name"]: c for c in named}
    assert by_name["padded-13-8"]["layout"] == "padded" and by_name["packed4-4-2"]["dense"] and not by_name["packed4-4-4"]["dense"]
    assert SC.num_rings(by_name["rings-63"]["arrays"]) == 63
    edges = SC.decision_edges()
    assert {n for n, _, _ in edges} >= {"16-4", "12-4", "rings-64", "k2", "padded-last-head-2", "packed-last-head-2"}
    for name, arrays, seed in edges:
        m = loader.CreateFromString(O.nam_json_wavenet_generic(arrays, O.synth_wavenet_weights(arrays, seed=seed)), ".nam", doPrewarm=False)
        assert m is not None, name
        for streams in (1, 600):
            info = m.KernelInfo(1.0, streams)
            assert info["kernel"] == "frame" and info["pack"] == 1 and info["input_limit"] == float("inf"), (name, streams, info)
        assert m.KernelInfo(1.0, 1)["range_proven"] == (not name.startswith("leaky")), name


def test_split_cases_reach_every_path_of_the_interpreter_they_name():
    """The named cases alone -- and the seeded draw once more -- reach: every layout; pack factors 1, 2 and 4, dense and not; kernel-level
    channel groups 2 and 4 and single-group real streams inside a pack; one, two and three arrays; models whose rings are all compact,
    none compact, and mixed; exact and roomy long rings; tap shifts on both sides of 16, 32, 64 and 128 frames; both activations; a
    first array with and without head bias."""
    named, fuzz, _ = _split_cases()

    def reach(cases):
        r = dict(layouts=set(), packs=set(), G=set(), real_g=set(), arrays=set(), rings=set(), kinds=set(), shifts=set(), acts=set(), bias0=set())
        for c in cases:
            arrays = c["arrays"]
            r["layouts"].add(c["layout"])
            r["packs"].add((c["pack"], c["dense"]))
            r["G"].update(SC.kernel_groups(arrays))
            if c["pack"] > 1:
                r["real_g"].update((a["channels"] + 3) // 4 for a in arrays)
            r["arrays"].add(len(arrays))
            kinds = {SC.ring_kind(d, i == 0) for a in arrays for i, d in enumerate(a["dilations"])}
            r["kinds"].update(kinds)
            r["rings"].add("compact" if kinds == {"compact"} else ("mixed" if "compact" in kinds else "long"))
            r["shifts"].update(SC.shifts(arrays))
            r["acts"].update(a["activation"] for a in arrays)
            if len(arrays) > 1:
                r["bias0"].add(bool(arrays[0]["has_head_bias"]))
        return r

    for what, r in (("named", reach(named)), ("fuzz", reach([c for c, _ in fuzz]))):
        assert r["layouts"] == {"plain", "padded", "packed"} and r["packs"] == {(1, False), (2, False), (4, False), (4, True)}, (what, r)
        assert r["G"] == {2, 4} and 1 in r["real_g"] and r["arrays"] == {1, 2, 3}, (what, r)
        assert r["rings"] == {"compact", "mixed", "long"} and r["kinds"] == {"compact", "roomy", "exact"}, (what, r)
        assert r["acts"] == {O.ACT_TANH, O.ACT_LEAKYRELU} and r["bias0"] == {True, False}, (what, r)
        for edge in SC.EDGES:
            assert any(edge // 2 <= s < edge for s in r["shifts"]) and edge in r["shifts"] and any(edge < s <= edge + edge // 2 for s in r["shifts"]), (what, edge, r["shifts"])
    shift = [c for c in named if c["family"] == "tap shifts"]
    for pick in ({"plain"}, {"packed"}):  # every dilation of the list at kernel G = 4 and 2 (plain 16 / 8, P = 2) and at one real group (P = 4)
        for p in (1, 2, 4):
            got = {d for c in shift if c["layout"] in pick and c["pack"] == p for a in c["arrays"] for d in a["dilations"]}
            assert not got or got == set(SC.DILATIONS), (pick, p, got)
    assert {(c["layout"], c["pack"]) for c in shift} == {("plain", 1), ("packed", 2), ("packed", 4)}
    # the layouts and widths the issue names
    widths = {tuple(a["channels"] for a in c["arrays"]): c["layout"] for c in named if c["family"] == "widths"}
    for cs in [(16, 8), (16, 16), (16,), (16, 8, 8)]:
        assert widths[cs] == "plain", cs
    for cs in [(13, 8), (12, 6), (13, 5), (9, 7), (16, 5), (10,), (6, 16)]:
        assert widths[cs] == "padded", cs
    for cs in [(8, 4), (7, 3), (5, 5), (8,), (6, 8), (8, 1), (8, 4, 2), (4, 2), (4, 4), (4, 3), (3, 1), (2, 2), (2, 4), (1,)]:
        assert widths[cs] == "packed", cs
    assert {c["layout"] for c in named if c["family"] == "activation"} == {"plain", "padded", "packed"}


@pytest.mark.parametrize("part", range(4))
def test_split_cases_are_well_conditioned(part):
    """Keeps the GPU parity rule honest without a GPU: for every case the f32 oracle's worst 32-frame window stays within 1 / 16 of
    the GPU bound -- 1.25e-7 RMS relative to the level above 1 -- of a float64 evaluation.  The project states the split arithmetic at
    no more than 8 times the f32 oracle's error, so a correct kernel stays under the bound on every case here.  A case that fails gets
    another seed, never a looser bound."""
    named, fuzz, batch = _split_cases()
    every = named + [c for c, _ in fuzz] + batch
    for case in every[part::4]:
        w = SC.weights(case)
        x = O.signal_noise(case["samples"], seed=case["seed"])
        yo = O.OracleWaveNet(case["arrays"], w).process(x)
        y64, _ = ref_np.wavenet_forward(case["arrays"], w, x)
        assert O.rms(y64) > 1e-5, (case["name"], O.rms(y64))
        for a in range(0, x.size, 32):
            err, level = O.rms(yo[a:a + 32] - y64[a:a + 32]), O.rms(y64[a:a + 32])
            assert err <= 1.25e-7 * max(1.0, level), (case["name"], a, err, level)
