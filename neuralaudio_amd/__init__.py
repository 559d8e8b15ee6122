"""neuralaudio_amd -- MI355X-native NeuralAudio hot path (NAM WaveNet / LSTM per-sample inference).

Thin, pythonic mirror of the reference's host interface for this path:
  NeuralModelLoader / NeuralModel  <->  NeuralAudio/NeuralModel.h:33-231 (same method names and meaning)
  Batch                            <->  new: many independent streams per GPU (include/neuralaudio_amd.h)
All compute happens in libNeuralAudioCAPI.so (C++ host code + hand-written gfx950 HIP kernels) through
its C ABI; numpy arrays are only the host-side containers.
"""
import ctypes as C
import os

import numpy as np

from . import capi

__all__ = ["NeuralModelLoader", "NeuralModel", "Batch", "MultiBatch", "EModelLoadMode", "EMathMode", "ECompositeModelLoadMode", "device_count",
           "NeuralAudioError", "render_offline", "render_plan", "debug_render_tap", "snapshot_bytes", "snapshot_fingerprint", "resample_plan", "resample_prototype",
           "resample_model_frames", "db_to_gain", "gate_params_from_db", "compressor_params_from_db", "mod_params_from_ms", "MOD_TRIANGLE", "MOD_SINE", "delay_params_from_ms", "eq_section", "tuner_params_from_range", "tuner_pitch", "mix_gains_from_pan"]


class NeuralAudioError(RuntimeError):
    pass


class EModelLoadMode:
    Internal = 0
    RTNeural = 1
    NAMCore = 2


class EMathMode:
    FastMath = 0
    StdMath = 1


class ECompositeModelLoadMode:
    LoadAll = 0
    OnDemand = 1


def device_count():
    return capi.device_count()


def db_to_gain(db):
    """Decibels as the linear gain Batch.SetStreamGain takes: 10 ** (db / 20), 0.0 at -inf (GetRecommendedOutputDBAdjustment is in dB)."""
    db = float(db)
    return 0.0 if db == float("-inf") else 10.0 ** (db / 20.0)


GATE_FIELDS = ("openPower", "closePower", "floorGain", "detectorCoeff", "attackSamples", "holdSamples", "releaseSamples")


def _gate_dict(p):
    return {name: (float if name in GATE_FIELDS[:4] else int)(getattr(p, name)) for name in GATE_FIELDS}


def _gate_params(d):
    if isinstance(d, capi.NA_GateParams):
        return d
    p = capi.NA_GateParams()
    for name in GATE_FIELDS:
        setattr(p, name, d[name])
    return p


def gate_params_from_db(sample_rate, open_db, close_db, floor_db=float("-inf"), detector_ms=1.0, attack_ms=1.0, hold_ms=50.0, release_ms=100.0):
    """The constants Batch.SetStreamGate takes, from decibels and milliseconds (NA_GateParamsFromDb): thresholds are dBFS of a sine's peak,
    floor_db = -inf closes the gate to silence.  Host arithmetic: needs no device."""
    out = capi.NA_GateParams()
    if capi.load_library().NA_GateParamsFromDb(int(sample_rate), float(open_db), float(close_db), float(floor_db), float(detector_ms),
                                               float(attack_ms), float(hold_ms), float(release_ms), C.byref(out)) != 0:
        raise NeuralAudioError(capi.last_error())
    return _gate_dict(out)


def _compressor_dict(p):
    return {"attackCoeff": float(p.attackCoeff), "releaseCoeff": float(p.releaseCoeff), "curve": np.ctypeslib.as_array(p.curve).astype(np.float32)}


def _compressor_params(d):
    if isinstance(d, capi.NA_CompressorParams):
        return d
    curve = np.ascontiguousarray(d["curve"], np.float32)
    if curve.shape != (capi.NA_COMPRESSOR_CURVE_POINTS,):
        raise NeuralAudioError("a compressor curve has %d values" % capi.NA_COMPRESSOR_CURVE_POINTS)
    p = capi.NA_CompressorParams()
    p.attackCoeff, p.releaseCoeff = d["attackCoeff"], d["releaseCoeff"]
    C.memmove(p.curve, curve.ctypes.data, curve.nbytes)
    return p


def compressor_params_from_db(sample_rate, threshold_db, ratio, knee_db=0.0, makeup_db=0.0, attack_ms=5.0, release_ms=100.0):
    """The constants Batch.SetStreamCompressor takes, from decibels and milliseconds (NA_CompressorParamsFromDb): attackCoeff,
    releaseCoeff and the curve of 513 gains as a float32 array.  ratio = inf, knee_db = 0, attack_ms = 0 is a limiter.  Host arithmetic:
    needs no device."""
    out = capi.NA_CompressorParams()
    if capi.load_library().NA_CompressorParamsFromDb(int(sample_rate), float(threshold_db), float(ratio), float(knee_db), float(makeup_db),
                                                     float(attack_ms), float(release_ms), C.byref(out)) != 0:
        raise NeuralAudioError(capi.last_error())
    return _compressor_dict(out)


MOD_TRIANGLE, MOD_SINE = 0, 1
MOD_SCALARS = (("baseSamples", float), ("depthSamples", float), ("phaseInc", int), ("shape", int), ("numVoices", int), ("feedback", float),
               ("wet", float), ("dry", float), ("tremoloDepth", float))


def _mod_dict(p):
    d = {name: kind(getattr(p, name)) for name, kind in MOD_SCALARS}
    d["voicePhase"] = [int(v) for v in p.voicePhase]
    d["voiceGain"] = [float(v) for v in p.voiceGain]
    return d


def _mod_params(d):
    if isinstance(d, capi.NA_ModParams):
        return d
    p = capi.NA_ModParams()
    for name, _ in MOD_SCALARS:
        setattr(p, name, d[name])
    if len(d["voicePhase"]) != 4 or len(d["voiceGain"]) != 4:
        raise NeuralAudioError("a modulation has four voicePhase and four voiceGain values")
    for v in range(4):
        p.voicePhase[v] = int(d["voicePhase"][v])
        p.voiceGain[v] = d["voiceGain"][v]
    return p


def mod_params_from_ms(sample_rate, base_ms, depth_ms, rate_hz, shape=MOD_SINE, voices=1, feedback=0.0, wet_db=0.0, dry_db=0.0, tremolo_depth=0.0):
    """The constants Batch.SetStreamMod takes, from milliseconds, hertz and decibels (NA_ModParamsFromMs): the voices lie 1 / voices of a
    cycle apart with gain 1 / voices each; -inf dB is 0.  Host arithmetic: needs no device."""
    out = capi.NA_ModParams()
    if capi.load_library().NA_ModParamsFromMs(int(sample_rate), float(base_ms), float(depth_ms), float(rate_hz), int(shape), int(voices), float(feedback),
                                              float(wet_db), float(dry_db), float(tremolo_depth), C.byref(out)) != 0:
        raise NeuralAudioError(capi.last_error())
    return _mod_dict(out)


DELAY_FIELDS = ("delaySamples", "feedback", "lowpassCoeff", "highpassCoeff", "wet", "dry")


def _delay_dict(p):
    return {name: (int if name == "delaySamples" else float)(getattr(p, name)) for name in DELAY_FIELDS}


def _delay_params(d):
    if isinstance(d, capi.NA_DelayParams):
        return d
    p = capi.NA_DelayParams()
    for name in DELAY_FIELDS:
        setattr(p, name, d[name])
    return p


def delay_params_from_ms(sample_rate, delay_ms, feedback=0.35, low_cut_hz=0.0, high_cut_hz=0.0, wet_db=-6.0, dry_db=0.0):
    """The constants Batch.SetStreamDelay takes, from milliseconds, hertz and decibels (NA_DelayParamsFromMs): low_cut_hz <= 0 leaves the
    high-pass out, high_cut_hz <= 0 or >= rate / 2 the low-pass; -inf dB is 0.  Host arithmetic: needs no device."""
    out = capi.NA_DelayParams()
    if capi.load_library().NA_DelayParamsFromMs(int(sample_rate), float(delay_ms), float(feedback), float(low_cut_hz), float(high_cut_hz),
                                                float(wet_db), float(dry_db), C.byref(out)) != 0:
        raise NeuralAudioError(capi.last_error())
    return _delay_dict(out)


METER_FIELDS = ("windowSamples", "clipLevelIn", "clipLevelOut")
METER_TAP_FIELDS = ("energy", "oversTotal", "peak", "peakHold", "overs")


def _meter_params(d):
    if isinstance(d, capi.NA_MeterParams):
        return d
    p = capi.NA_MeterParams()
    for name in METER_FIELDS:
        setattr(p, name, d[name])
    return p


def _meter_reading(r):
    tap = lambda t: {name: (float if name in ("peak", "peakHold") else int)(getattr(t, name)) for name in METER_TAP_FIELDS}
    return {"windows": int(r.windows), "in": tap(r.in_), "out": tap(r.out), "gateGainMin": float(r.gateGainMin), "gateGainLast": float(r.gateGainLast),
            "windowSamples": int(r.windowSamples)}


TUNER_FIELDS = ("decimation", "windowSamples", "minLag", "maxLag", "hopSamples", "phase", "thresholdQ10", "minEnergy")


def _tuner_params(d):
    if isinstance(d, capi.NA_TunerParams):
        return d
    p = capi.NA_TunerParams()
    for name in TUNER_FIELDS:
        setattr(p, name, int(d[name]))
    return p


def _tuner_dict(p):
    return {name: int(getattr(p, name)) for name in TUNER_FIELDS}


def _tuner_reading(r):
    return {"evaluations": int(r.evaluations), "position": int(r.position), "r": [int(v) for v in r.r], "e0": int(r.e0), "e": [int(v) for v in r.e],
            "lag": int(r.lag), "decimation": int(r.decimation)}


def _tuner_reading_struct(d):
    if isinstance(d, capi.NA_TunerReading):
        return d
    r = capi.NA_TunerReading()
    r.evaluations, r.position, r.e0, r.lag, r.decimation = d["evaluations"], d["position"], d["e0"], d["lag"], d["decimation"]
    for i in range(3):
        r.r[i], r.e[i] = d["r"][i], d["e"][i]
    return r


def tuner_params_from_range(sampleRate, lowestHz, highestHz, evaluationsPerSecond):
    """The NA_TunerParams fields, as a dict, for notes from lowestHz to highestHz (NA_TunerParamsFromRange)."""
    out = capi.NA_TunerParams()
    if capi.load_library().NA_TunerParamsFromRange(float(sampleRate), float(lowestHz), float(highestHz), float(evaluationsPerSecond), C.byref(out)) != 0:
        raise NeuralAudioError(capi.last_error())
    return _tuner_dict(out)


def tuner_pitch(reading, sampleRate):
    """(hz, clarity) of a ReadStreamTuner dict; None when it holds no pitch (lag == 0) (NA_TunerPitch)."""
    hz, clarity = C.c_double(0.0), C.c_double(0.0)
    rc = int(capi.load_library().NA_TunerPitch(C.byref(_tuner_reading_struct(reading)), float(sampleRate), C.byref(hz), C.byref(clarity)))
    if rc < 0:
        raise NeuralAudioError(capi.last_error())
    return (hz.value, clarity.value) if rc else None


def mix_gains_from_pan(levelDb, pan):
    """(left, right) float32 gains of one member of a stereo mix group (Batch.SetMixGroup): equal power, level = 10^(levelDb / 20),
    pan in [-1, 1]; pan = -1 is exactly (level, 0), pan = +1 exactly (0, level) (NA_MixGainsFromPan)."""
    left, right = C.c_float(0.0), C.c_float(0.0)
    if capi.load_library().NA_MixGainsFromPan(float(levelDb), float(pan), C.byref(left), C.byref(right)) != 0:
        raise NeuralAudioError(capi.last_error())
    return left.value, right.value


EQ_FIELDS = ("b0", "b1", "b2", "a1", "a2")
EQ_KINDS = {"lowpass": 0, "highpass": 1, "lowshelf": 2, "highshelf": 3, "peaking": 4}


def _eq_dict(s):
    return {name: float(getattr(s, name)) for name in EQ_FIELDS}


def _eq_section(d):
    if isinstance(d, capi.NA_EqSection):
        return d
    s = capi.NA_EqSection()
    for name in EQ_FIELDS:
        setattr(s, name, d[name])
    return s


def eq_section(kind, sample_rate, freq_hz, q=0.7071067811865476, gain_db=0.0):
    """One biquad section for Batch.SetStreamEq from a design (NA_EqSectionFromDesign, the RBJ cookbook in double): kind 0 / "lowpass",
    1 / "highpass", 2 / "lowshelf", 3 / "highshelf", 4 / "peaking"; gain_db matters for the shelves and the peak.  Host arithmetic: needs
    no device."""
    out = capi.NA_EqSection()
    kind = EQ_KINDS[kind] if isinstance(kind, str) else int(kind)
    if capi.load_library().NA_EqSectionFromDesign(kind, float(sample_rate), float(freq_hz), float(q), float(gain_db), C.byref(out)) != 0:
        raise NeuralAudioError(capi.last_error())
    return _eq_dict(out)


def rccl_available():
    """librccl.so loads and exports what the multi-GPU host binds (no GPU needed)."""
    return bool(capi.load_library().NA_RcclAvailable())


def debug_set_rccl_api(mode, fail_send_at=0, rendezvous_ms=0):
    """Tests: 1 = the multi-GPU host binds the in-library loopback table (ranks may share a device) instead of librccl.so; 0 = back."""
    capi.load_library().NA_DebugSetRcclApi(int(mode), int(fail_send_at), int(rendezvous_ms))


def _recurrent_plan_dict(out):
    return {"runs": bool(out[0]), "waves": int(out[1]), "rows_per_lane": int(out[2]), "l2w": bool(out[3]), "head_in_loop": bool(out[4]),
            "lds_bytes": int(out[5])}


def recurrent_shape_plan(kind, hidden, layers=1, tail_layers=0, tail_width=0, tail_history=0, rpl=0, force_l2w=-1):
    """Test hook, host side only (NA_DebugRecurrentShapePlan): how the runtime-shaped recurrent kernel would run an "lstm" / "gru" of this
    shape; rpl > 0 / force_l2w >= 0 stand in for the tuning knobs.  "admitted": the loader's shape predicate of that kernel takes it."""
    out = (C.c_int * 6)()
    r = capi.load_library().NA_DebugRecurrentShapePlan(1 if kind == "gru" else 0, int(hidden), int(layers), int(tail_layers), int(tail_width),
                                                       int(tail_history), int(rpl), int(force_l2w), out)
    if r < 0:
        raise NeuralAudioError("NA_DebugRecurrentShapePlan: bad argument")
    return dict(_recurrent_plan_dict(out), admitted=bool(r))


RECURRENT_KNOB_BITS = {"NA_LSTM_NO_DPP": 1, "NA_GRU_NO_DPP": 2, "NA_LSTM_LANE_KERNEL": 4, "NA_LSTM_NO_WAVE_RT": 8, "NA_REC_NO_DPP32": 16, "NA_REC_L2W": 32}


def recurrent_kernel(kind, hidden, layers=1, tail_layers=0, tail_width=0, tail_history=0, have_wt=True, knobs=(), rpl=0):
    """Test hook, host side only (NA_DebugRecurrentKernel): the name of the kernel that runs an "lstm" / "gru" of this shape ("": none).
    knobs: names from RECURRENT_KNOB_BITS (the environment is not read), or None for the process's own tuning knobs; rpl: NA_REC_RPL."""
    mask = -1 if knobs is None else sum(RECURRENT_KNOB_BITS[k] for k in knobs)
    name = C.create_string_buffer(64)
    r = capi.load_library().NA_DebugRecurrentKernel(1 if kind == "gru" else 0, int(hidden), int(layers), int(tail_layers), int(tail_width),
                                                    int(tail_history), int(bool(have_wt)), mask, int(rpl), name, 64)
    if r < 0:
        raise NeuralAudioError("NA_DebugRecurrentKernel: bad argument")
    return name.value.decode()


# the knobs of the WaveNet decisions in the order of NA_DebugWaveNetKernel / NA_DebugWaveNetLaunch, by their environment names
# ("NA_WN_KERNEL": "split" | "frame" | "generic" or 1 | 2 | 3; "NA_WN_PAD": 0 turns padding off; "NA_WN_SPEC": 0 turns the chains off;
# NA_SP_T and NA_SP_GEN imply NA_WN_SPEC=0, as in the library's own parsing of the environment)
WAVENET_KNOBS = ("NA_WN_KERNEL", "NA_WN_PACK", "NA_WN_PAD", "NA_WN_DENSE", "NA_SP_T", "NA_SP_SPB", "NA_SP_GEN", "NA_SP_NO_T1", "NA_FR_PF", "NA_FR_SPB",
                 "NA_WN_SPEC")
WAVENET_FAMILIES = {1: "f16-split", 2: "frame", 3: "generic"}
WAVENET_LAUNCH_KERNELS = ("none", "chain", "chain table", "interpreter", "frame", "pieces")
WAVENET_CHAINS = ("Std", "Lite", "LitePacked", "Lite16T1", "A2")
# csrc/host_route.h HostRoute, in its order: what Batch.DebugLastHostRoute() indexes (tests/test_host_route_cpu.py pins the names)
HOST_ROUTES = ("RegisteredInPlace", "StagedHalves", "StagedInPlace", "StagedCopies", "SubmitHalves", "SubmitInPlace", "SubmitOwnStream",
               "SubmitCopyStreams", "DeviceResident", "DeviceHalves", "DeviceOrdered", "ToDeviceInPlace", "ToDeviceCopies")


def _wavenet_knob_args(knobs):
    if knobs is None:
        return -1, None
    vals = (C.c_int * len(WAVENET_KNOBS))()
    mask = 0
    knobs = dict(knobs)
    if ("NA_SP_T" in knobs or "NA_SP_GEN" in knobs) and "NA_WN_SPEC" not in knobs:
        knobs["NA_WN_SPEC"] = 0
    for name, v in knobs.items():
        i = WAVENET_KNOBS.index(name)
        if name == "NA_WN_KERNEL":
            v = {"split": 1, "frame": 2, "generic": 3}.get(v, v)
        elif name == "NA_WN_PAD":
            v = int(int(v) == 0)  # (the knob of the decision is "padding off")
        elif name in ("NA_SP_GEN", "NA_SP_NO_T1"):
            v = 1  # (set at all: on)
        vals[i] = int(v)
        mask |= 1 << i
    return mask, vals


def wavenet_kernel(model, streams=1, quality=1.0, knobs=()):
    """Test hook, host side only (NA_DebugWaveNetKernel): what a batch's model group decides once for `streams` streams of a WaveNet `model`
    (csrc/wavenet_choice.h WaveNetKernelFor).  knobs: a dict of names from WAVENET_KNOBS (the environment is not read), or None for the
    process's own tuning knobs."""
    mask, vals = _wavenet_knob_args(knobs)
    out = (C.c_int * 8)()
    lim = C.c_float()
    name = C.create_string_buffer(64)
    if capi.load_library().NA_DebugWaveNetKernel(model._h, float(quality), int(streams), mask, vals, out, C.byref(lim), name, 64) != 0:
        raise NeuralAudioError(capi.last_error() or "NA_DebugWaveNetKernel: bad argument")
    return {"family": WAVENET_FAMILIES[out[0]], "pack": int(out[1]), "dense": bool(out[2]), "virtual": bool(out[3]), "spec_arch": int(out[4]),
            "launch_kind": int(out[5]), "range_proven": bool(out[6]), "weights_ok": bool(out[7]), "input_limit": float(lim.value),
            "kernel_name": name.value.decode()}


def wavenet_launch(groups, n, frame=False, sharing=1, beyond_cache=False, cus=256, knobs=()):
    """Test hook, host side only (NA_DebugWaveNetLaunch): the one kernel instantiation a launch of `n` frames of `groups` lands on
    (csrc/wavenet_choice.h WaveNetLaunchFor).  groups: per group (spec_arch, pack, split_fast_T, streams, has_lists, max_a4_floats[, max_G,
    max_split_ops]).  Returns (kernel, error, chain, NF, SPB, NT, T, WPS, GEN, PK, PF) as ints."""
    mask, vals = _wavenet_knob_args(knobs)
    flat = (C.c_int * (8 * max(len(groups), 1)))()
    for i, g in enumerate(groups):
        g = tuple(g) + (1, 16)[len(g) - 6:]
        flat[8 * i:8 * i + 8] = [int(v) for v in g]
    out = (C.c_int * 11)()
    if capi.load_library().NA_DebugWaveNetLaunch(int(bool(frame)), int(n), len(groups), flat, int(sharing), int(bool(beyond_cache)), int(cus), mask, vals, out) != 0:
        raise NeuralAudioError("NA_DebugWaveNetLaunch: bad argument")
    return tuple(out)


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class NeuralModel:
    """One mono audio stream (NeuralAudio::NeuralModel). Created by NeuralModelLoader."""

    def __init__(self, handle):
        self._lib = capi.load_library()
        self._h = handle

    # -- reference API -------------------------------------------------------------------------
    def GetLoadMode(self):
        return self._lib.GetLoadMode(self._h)

    def IsStatic(self):
        return bool(self._lib.IsStatic(self._h))

    def SetMaxAudioBufferSize(self, max_size):
        self._lib.SetMaxAudioBufferSize(self._h, int(max_size))

    def GetRecommendedInputDBAdjustment(self):
        return float(self._lib.GetRecommendedInputDBAdjustment(self._h))

    def GetRecommendedOutputDBAdjustment(self):
        return float(self._lib.GetRecommendedOutputDBAdjustment(self._h))

    def GetSampleRate(self):
        return float(self._lib.GetSampleRate(self._h))

    def GetReceptiveFieldSize(self):
        return int(self._lib.NA_GetReceptiveFieldSize(self._h))

    def HasQualityScaling(self):
        return bool(self._lib.NA_HasQualityScaling(self._h))

    def GetQualityScaleFactor(self):
        return float(self._lib.NA_GetQualityScaleFactor(self._h))

    def SetQualityScaleFactor(self, q):
        self._lib.NA_SetQualityScaleFactor(self._h, float(q))

    def GetModelVersion(self):
        buf = C.create_string_buffer(256)
        self._lib.NA_GetModelVersion(self._h, buf, 256)
        return buf.value.decode()

    def GetMetadata(self, field):
        buf = C.create_string_buffer(65536)
        self._lib.NA_GetMetadata(self._h, field.encode(), buf, 65536)
        return buf.value.decode()

    def Prewarm(self):
        if self._lib.NA_Prewarm(self._h) != 0:
            raise NeuralAudioError(capi.last_error())

    def Process(self, x):
        """input -> output (same length), any number of samples; runs on the GPU."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.empty_like(x)
        if self._lib.NA_ProcessChecked(self._h, _fptr(x), _fptr(y), x.size) != 0:
            raise NeuralAudioError(capi.last_error())
        return y

    def IsQualityChangeRealtimeSafe(self, q):
        return bool(self._lib.NA_IsQualityChangeRealtimeSafe(self._h, float(q)))

    def GetProcessLatencySamples(self):
        """External samples by which Process delays its output: 0 unless the loader's resampling opt-in applies to this model."""
        return int(self._lib.NA_GetProcessLatencySamples(self._h))

    def GetModelProcessRate(self):
        """The model-side rate as loaded: the file's rate times the oversampling factor the loader applied (0: not a whole number)."""
        return int(self._lib.NA_GetModelProcessRate(self._h))

    def KernelInfo(self, quality=1.0, streams=1):
        """Host side only: the kernel family a batch of `streams` streams would run on and the f16-split range proof behind the choice."""
        name = C.create_string_buffer(64)
        lim = C.c_float(0.0)
        proven, wok, pack = C.c_int(0), C.c_int(0), C.c_int(0)
        if self._lib.NA_ModelKernelInfo(self._h, float(quality), int(streams), name, 64, C.byref(lim), C.byref(proven), C.byref(wok), C.byref(pack)) != 0:
            raise NeuralAudioError(capi.last_error())
        return {"kernel": name.value.decode(), "input_limit": float(lim.value), "range_proven": bool(proven.value), "weights_ok": bool(wok.value),
                "pack": int(pack.value)}

    def RecurrentPlan(self):
        """Test hook, host side only (NA_DebugRecurrentPlan): how the runtime-shaped recurrent kernel runs this LSTM / GRU / keras stack."""
        out = (C.c_int * 6)()
        if self._lib.NA_DebugRecurrentPlan(self._h, out) != 0:
            raise NeuralAudioError(capi.last_error())
        return _recurrent_plan_dict(out)

    # -- stream snapshots (include/neuralaudio_amd.h) --------------------------------
    def SnapshotBytes(self):
        return snapshot_bytes(self)

    def SaveState(self):
        """This stream's state as a relocatable blob (bytes); LoadState on a model of the same file continues from it."""
        buf = C.create_string_buffer(max(self.SnapshotBytes(), 1))
        written = C.c_size_t(0)
        if self._lib.NA_SaveModelState(self._h, buf, len(buf), C.byref(written)) != 0:
            raise NeuralAudioError(capi.last_error())
        return buf.raw[:written.value]

    def LoadState(self, blob):
        blob = bytes(blob)
        if self._lib.NA_LoadModelState(self._h, blob, len(blob)) != 0:
            raise NeuralAudioError(capi.last_error())

    def close(self):
        if self._h:
            self._lib.DeleteModel(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NeuralModelLoader:
    """NeuralAudio::NeuralModelLoader (settings + factories)."""

    def __init__(self):
        self._lib = capi.load_library()
        self._h = self._lib.CreateLoader()
        if not self._h:
            raise NeuralAudioError(capi.last_error())

    def SetLSTMLoadMode(self, mode):
        self._lib.SetLSTMLoadMode(self._h, int(mode))

    def SetWaveNetLoadMode(self, mode):
        self._lib.SetWaveNetLoadMode(self._h, int(mode))

    def SetAudioInputLevelDBu(self, dbu):
        self._lib.SetAudioInputLevelDBu(self._h, float(dbu))

    def SetDefaultMaxAudioBufferSize(self, n):
        self._lib.SetDefaultMaxAudioBufferSize(self._h, int(n))

    def SetDefaultQualityScaleFactor(self, q):
        self._lib.NA_SetDefaultQualityScaleFactor(self._h, float(q))

    def SetExternalSampleRate(self, sr):
        self._lib.NA_SetExternalSampleRate(self._h, int(sr))

    def SetResampleToExternalRate(self, on=True):
        """Opt-in: models created at an external rate that is neither their rate nor a whole multiple of it resample inside Process."""
        self._lib.NA_SetResampleToExternalRate(self._h, 1 if on else 0)

    def SetDevice(self, device):
        self._lib.NA_SetDevice(self._h, int(device))

    def SetWaveNetMathMode(self, mode):
        self._lib.NA_SetWaveNetMathMode(self._h, int(mode))

    def SetLSTMMathMode(self, mode):
        self._lib.NA_SetLSTMMathMode(self._h, int(mode))

    def SetCompositeModelLoadMode(self, mode):
        self._lib.NA_SetCompositeModelLoadMode(self._h, int(mode))

    def CreateFromFile(self, path, doPrewarm=True, use_wchar_entry=False):
        """Returns None when the file is missing / unsupported (reference: nullptr); raises on malformed files."""
        if use_wchar_entry:
            h = self._lib.CreateModelFromFile(self._h, str(path))
        else:
            h = self._lib.NA_CreateModelFromFileUtf8(self._h, str(path).encode(), 1 if doPrewarm else 0)
        if not h:
            err = capi.last_error()
            if "not found or not supported" in err or "model not supported" in err:
                return None
            raise NeuralAudioError(err)
        return NeuralModel(h)

    def CreateFromString(self, text, extension, doPrewarm=True):
        h = self._lib.NA_CreateModelFromString(self._h, text.encode(), extension.encode(), 1 if doPrewarm else 0)
        if not h:
            err = capi.last_error()
            if "model not supported" in err:
                return None
            raise NeuralAudioError(err)
        return NeuralModel(h)

    def close(self):
        if self._h:
            self._lib.DeleteLoader(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch:
    """Many independent streams on one GPU; row s of the [streams][n] arrays is stream s."""

    def __init__(self, device=0, hip_stream=None):
        self._lib = capi.load_library()
        self._h = self._lib.NA_BatchCreate(int(device), C.c_void_p(hip_stream) if hip_stream else None)
        if not self._h:
            raise NeuralAudioError(capi.last_error())

    def AddStreams(self, model, count=1, quality=1.0, doPrewarm=True):
        first = self._lib.NA_BatchAddStreams(self._h, model._h, float(quality), int(count), 1 if doPrewarm else 0)
        if first < 0:
            raise NeuralAudioError(capi.last_error())
        return first

    def NumStreams(self):
        return int(self._lib.NA_BatchNumStreams(self._h))

    def NumLiveStreams(self):
        return int(self._lib.NA_BatchNumLiveStreams(self._h))

    def IsLive(self, stream):
        return bool(self._lib.NA_BatchIsLive(self._h, int(stream)))

    def RemoveStreams(self, first, count=1):
        if self._lib.NA_BatchRemoveStreams(self._h, int(first), int(count)) != 0:
            raise NeuralAudioError(capi.last_error())

    # -- the stream pool: ReserveStreams is set-up side; ActivateStream / ParkStream are real-time safe (include/neuralaudio_amd.h) ----
    def ReserveStreams(self, model, count=1, doPrewarm=True):
        """`count` parked, armed streams of `model`; returns the first id."""
        first = self._lib.NA_BatchReserveStreams(self._h, model._h, int(count), 1 if doPrewarm else 0)
        if first < 0:
            raise NeuralAudioError(capi.last_error())
        return first

    def ActivateStream(self, stream, quality=1.0):
        if self._lib.NA_BatchActivateStream(self._h, int(stream), float(quality)) != 0:
            raise NeuralAudioError(capi.last_error())

    def ParkStream(self, stream):
        if self._lib.NA_BatchParkStream(self._h, int(stream)) != 0:
            raise NeuralAudioError(capi.last_error())

    def IsParked(self, stream):
        return bool(self._lib.NA_BatchIsParked(self._h, int(stream)))

    def FindParked(self, model):
        return int(self._lib.NA_BatchFindParked(self._h, model._h))

    def NumParked(self):
        return int(self._lib.NA_BatchNumParked(self._h))

    # -- the output stage: EnableOutputStage is set-up side; SetStreamGain / Handover are real-time safe (include/neuralaudio_amd.h) ----
    def EnableOutputStage(self):
        if self._lib.NA_BatchEnableOutputStage(self._h) != 0:
            raise NeuralAudioError(capi.last_error())

    def SetStreamGain(self, stream, gain, rampSamples=0):
        """Linear output gain of a live stream, reached over `rampSamples` samples (db_to_gain turns decibels into it)."""
        if self._lib.NA_BatchSetStreamGain(self._h, int(stream), float(gain), int(rampSamples)) != 0:
            raise NeuralAudioError(capi.last_error())

    def GetStreamGain(self, stream):
        gain = float(self._lib.NA_BatchGetStreamGain(self._h, int(stream)))
        if gain < 0:
            raise NeuralAudioError(capi.last_error())
        return gain

    def Handover(self, src, dst, quality=1.0, fadeSamples=0):
        """Activates the parked stream `dst`; from the next buffer on its row carries the cross-fade from `src`'s output to its own."""
        if self._lib.NA_BatchHandover(self._h, int(src), int(dst), float(quality), int(fadeSamples)) != 0:
            raise NeuralAudioError(capi.last_error())

    def HandoverRemaining(self, stream):
        left = int(self._lib.NA_BatchHandoverRemaining(self._h, int(stream)))
        if left < 0:
            raise NeuralAudioError(capi.last_error())
        return left

    # -- the cabinet stage: EnableCabinetStage / LoadIR / UnloadIR are set-up side; SetStreamIR is real-time safe (include/neuralaudio_amd.h) ----
    def EnableCabinetStage(self, maxTaps):
        if self._lib.NA_BatchEnableCabinetStage(self._h, int(maxTaps)) != 0:
            raise NeuralAudioError(capi.last_error())

    def CabinetInfo(self):
        info = capi.NA_CabinetInfo()
        if self._lib.NA_BatchGetCabinetInfo(self._h, C.byref(info)) != 0:
            raise NeuralAudioError(capi.last_error())
        return {name: int(getattr(info, name)) for name, _ in capi.NA_CabinetInfo._fields_}

    def LoadIR(self, taps):
        """Copies an impulse response (1-D, at the rate of the rows the caller sees) to the device; returns its id."""
        taps = np.ascontiguousarray(taps, np.float32).reshape(-1)
        ir = int(self._lib.NA_BatchLoadIR(self._h, _fptr(taps), int(taps.size)))
        if ir < 0:
            raise NeuralAudioError(capi.last_error())
        return ir

    def UnloadIR(self, ir):
        if self._lib.NA_BatchUnloadIR(self._h, int(ir)) != 0:
            raise NeuralAudioError(capi.last_error())

    def SetStreamIR(self, stream, ir, fadeSamples=0):
        """The stream's row is convolved with IR `ir` from the next sample on (-1: dry), cross-faded over `fadeSamples` samples."""
        if self._lib.NA_BatchSetStreamIR(self._h, int(stream), int(ir), int(fadeSamples)) != 0:
            raise NeuralAudioError(capi.last_error())

    def GetStreamIR(self, stream):
        ir = int(self._lib.NA_BatchGetStreamIR(self._h, int(stream)))
        if ir <= -2:
            raise NeuralAudioError(capi.last_error())
        return ir

    def IRFadeRemaining(self, stream):
        left = int(self._lib.NA_BatchStreamIRFadeRemaining(self._h, int(stream)))
        if left < 0:
            raise NeuralAudioError(capi.last_error())
        return left

    def _debug_run_stage(self, hook, rows, n):
        assert rows.dtype == np.float32 and rows.flags["C_CONTIGUOUS"] and rows.ndim == 2 and rows.shape[0] == self.NumStreams()
        n = rows.shape[1] if n is None else int(n)
        if hook(self._h, _fptr(rows), int(rows.shape[1]), n) != 0:
            raise NeuralAudioError(capi.last_error())
        return rows

    def DebugRunCabinetStage(self, rows, n=None):
        """Test hook: the stage of a call of n samples, in place on the float32 array rows[NumStreams, stride] (NA_DebugRunCabinetStage)."""
        return self._debug_run_stage(self._lib.NA_DebugRunCabinetStage, rows, n)

    # -- the reverb stage: EnableReverbStage / LoadReverbIR / UnloadReverbIR are set-up side; SetStreamReverb is real-time safe (include/neuralaudio_amd.h) ----
    def EnableReverbStage(self, maxTaps):
        if self._lib.NA_BatchEnableReverbStage(self._h, int(maxTaps)) != 0:
            raise NeuralAudioError(capi.last_error())

    def ReverbInfo(self):
        info = capi.NA_ReverbInfo()
        if self._lib.NA_BatchGetReverbInfo(self._h, C.byref(info)) != 0:
            raise NeuralAudioError(capi.last_error())
        return {name: int(getattr(info, name)) for name, _ in capi.NA_ReverbInfo._fields_}

    def LoadReverbIR(self, taps):
        """Puts a long impulse response (1-D, at the rate of the rows the caller sees) on the device -- its first 128 taps and the spectra
        of the partitions behind them; returns its id."""
        taps = np.ascontiguousarray(taps, np.float32).reshape(-1)
        ir = int(self._lib.NA_BatchLoadReverbIR(self._h, _fptr(taps), int(taps.size)))
        if ir < 0:
            raise NeuralAudioError(capi.last_error())
        return ir

    def UnloadReverbIR(self, ir):
        if self._lib.NA_BatchUnloadReverbIR(self._h, int(ir)) != 0:
            raise NeuralAudioError(capi.last_error())

    def SetStreamReverb(self, stream, ir, wet, dry, fadeSamples=0):
        """The stream's row x becomes dry * x + wet * (x convolved with IR `ir`) from the next sample on (-1: no reverb), cross-faded
        over `fadeSamples` samples."""
        if self._lib.NA_BatchSetStreamReverb(self._h, int(stream), int(ir), float(wet), float(dry), int(fadeSamples)) != 0:
            raise NeuralAudioError(capi.last_error())

    def GetStreamReverb(self, stream):
        """(ir, wet, dry) of the stream's target setting; ir = -1: no reverb."""
        wet, dry = C.c_float(0.0), C.c_float(0.0)
        ir = int(self._lib.NA_BatchGetStreamReverb(self._h, int(stream), C.byref(wet), C.byref(dry)))
        if ir <= -2:
            raise NeuralAudioError(capi.last_error())
        return ir, float(wet.value), float(dry.value)

    def ReverbFadeRemaining(self, stream):
        left = int(self._lib.NA_BatchStreamReverbFadeRemaining(self._h, int(stream)))
        if left < 0:
            raise NeuralAudioError(capi.last_error())
        return left

    def DebugRunReverbStage(self, rows, n=None):
        """Test hook: the stage of a call of n samples, in place on the float32 array rows[NumStreams, stride] (NA_DebugRunReverbStage)."""
        return self._debug_run_stage(self._lib.NA_DebugRunReverbStage, rows, n)

    # -- the delay stage: EnableDelayStage is set-up side; SetStreamDelay is real-time safe (include/neuralaudio_amd.h) ----
    def EnableDelayStage(self, maxDelaySamples):
        if self._lib.NA_BatchEnableDelayStage(self._h, int(maxDelaySamples)) != 0:
            raise NeuralAudioError(capi.last_error())

    def GetDelayInfo(self):
        info = capi.NA_DelayInfo()
        if self._lib.NA_BatchGetDelayInfo(self._h, C.byref(info)) != 0:
            raise NeuralAudioError(capi.last_error())
        return {name: int(getattr(info, name)) for name, _ in capi.NA_DelayInfo._fields_}

    def SetStreamDelay(self, stream, params, fadeSamples=0):
        """An echo on the stream from the next sample on: `params` a dict of the NA_DelayParams fields (delay_params_from_ms makes one);
        None: no delay.  The change runs over `fadeSamples` samples."""
        p = None if params is None else C.byref(_delay_params(params))
        if self._lib.NA_BatchSetStreamDelay(self._h, int(stream), p, int(fadeSamples)) != 0:
            raise NeuralAudioError(capi.last_error())

    def GetStreamDelay(self, stream):
        """The target setting as a dict; None: no delay (or one that fades to none)."""
        out = capi.NA_DelayParams()
        rc = int(self._lib.NA_BatchGetStreamDelay(self._h, int(stream), C.byref(out)))
        if rc < 0:
            raise NeuralAudioError(capi.last_error())
        return _delay_dict(out) if rc else None

    def StreamDelayFadeRemaining(self, stream):
        left = int(self._lib.NA_BatchStreamDelayFadeRemaining(self._h, int(stream)))
        if left < 0:
            raise NeuralAudioError(capi.last_error())
        return left

    def DebugRunDelayStage(self, rows, n=None):
        """Test hook: the stage of a call of n samples, in place on the float32 array rows[NumStreams, stride] (NA_DebugRunDelayStage)."""
        return self._debug_run_stage(self._lib.NA_DebugRunDelayStage, rows, n)

    # -- the modulation stage: EnableModStage is set-up side; SetStreamMod is real-time safe (include/neuralaudio_amd.h) ----
    def EnableModStage(self, maxDelaySamples):
        if self._lib.NA_BatchEnableModStage(self._h, int(maxDelaySamples)) != 0:
            raise NeuralAudioError(capi.last_error())

    def GetModInfo(self):
        info = capi.NA_ModInfo()
        if self._lib.NA_BatchGetModInfo(self._h, C.byref(info)) != 0:
            raise NeuralAudioError(capi.last_error())
        return {name: int(getattr(info, name)) for name, _ in capi.NA_ModInfo._fields_}

    def SetStreamMod(self, stream, params, fadeSamples=0):
        """A chorus, flanger, vibrato or tremolo on the stream from the next sample on: `params` a dict of the NA_ModParams fields
        (mod_params_from_ms makes one) or the struct itself; None: the effect goes.  The change runs over `fadeSamples` samples."""
        p = None if params is None else C.byref(_mod_params(params))
        if self._lib.NA_BatchSetStreamMod(self._h, int(stream), p, int(fadeSamples)) != 0:
            raise NeuralAudioError(capi.last_error())

    def GetStreamMod(self, stream):
        """The target setting as a dict; None: no modulation (or one that fades to none)."""
        out = capi.NA_ModParams()
        rc = int(self._lib.NA_BatchGetStreamMod(self._h, int(stream), C.byref(out)))
        if rc < 0:
            raise NeuralAudioError(capi.last_error())
        return _mod_dict(out) if rc else None

    def StreamModFadeRemaining(self, stream):
        left = int(self._lib.NA_BatchStreamModFadeRemaining(self._h, int(stream)))
        if left < 0:
            raise NeuralAudioError(capi.last_error())
        return left

    def DebugRunModStage(self, rows, n=None):
        """Test hook: the stage of a call of n samples, in place on the float32 array rows[NumStreams, stride] (NA_DebugRunModStage)."""
        return self._debug_run_stage(self._lib.NA_DebugRunModStage, rows, n)

    # -- the compressor stage: EnableCompressorStage is set-up side; SetStreamCompressor is real-time safe (include/neuralaudio_amd.h) ----
    def EnableCompressorStage(self):
        if self._lib.NA_BatchEnableCompressorStage(self._h) != 0:
            raise NeuralAudioError(capi.last_error())

    def GetCompressorInfo(self):
        info = capi.NA_CompressorInfo()
        if self._lib.NA_BatchGetCompressorInfo(self._h, C.byref(info)) != 0:
            raise NeuralAudioError(capi.last_error())
        return {name: int(getattr(info, name)) for name, _ in capi.NA_CompressorInfo._fields_}

    def SetStreamCompressor(self, stream, params, fadeSamples=0):
        """A compressor on the stream from the next sample on: `params` a dict of the NA_CompressorParams fields
        (compressor_params_from_db makes one) or the struct itself; None: the compressor goes.  The curve fades in over `fadeSamples`
        samples; the coefficients act at once."""
        p = None if params is None else C.byref(_compressor_params(params))
        if self._lib.NA_BatchSetStreamCompressor(self._h, int(stream), p, int(fadeSamples)) != 0:
            raise NeuralAudioError(capi.last_error())

    def GetStreamCompressor(self, stream):
        """The target as a dict; None: no compressor (or one that fades to none)."""
        out = capi.NA_CompressorParams()
        rc = int(self._lib.NA_BatchGetStreamCompressor(self._h, int(stream), C.byref(out)))
        if rc < 0:
            raise NeuralAudioError(capi.last_error())
        return _compressor_dict(out) if rc else None

    def StreamCompressorFadeRemaining(self, stream):
        left = int(self._lib.NA_BatchStreamCompressorFadeRemaining(self._h, int(stream)))
        if left < 0:
            raise NeuralAudioError(capi.last_error())
        return left

    def StreamCompressorGain(self, stream):
        """The compressor's gain at the last sample produced (1 without a compressor).  Synchronises the batch: a diagnostic."""
        gain = float(self._lib.NA_BatchStreamCompressorGain(self._h, int(stream)))
        if gain < 0:
            raise NeuralAudioError(capi.last_error())
        return gain

    def DebugRunCompressorStage(self, rows, n=None):
        """Test hook: the stage of a call of n samples, in place on the float32 array rows[NumStreams, stride] (NA_DebugRunCompressorStage)."""
        return self._debug_run_stage(self._lib.NA_DebugRunCompressorStage, rows, n)

    # -- the gate stage: EnableGateStage is set-up side; SetStreamGate is real-time safe (include/neuralaudio_amd.h) ----
    def EnableGateStage(self):
        if self._lib.NA_BatchEnableGateStage(self._h) != 0:
            raise NeuralAudioError(capi.last_error())

    def GetGateInfo(self):
        info = capi.NA_GateInfo()
        if self._lib.NA_BatchGetGateInfo(self._h, C.byref(info)) != 0:
            raise NeuralAudioError(capi.last_error())
        return {name: int(getattr(info, name)) for name, _ in capi.NA_GateInfo._fields_}

    def SetStreamGate(self, stream, params, startOpen=True):
        """A noise gate on the stream from the next sample on: `params` a dict of the NA_GateParams fields (gate_params_from_db makes one
        from decibels and milliseconds); None takes the gate away, click-free.  A stream that has a gate keeps its state."""
        p = None if params is None else C.byref(_gate_params(params))
        if self._lib.NA_BatchSetStreamGate(self._h, int(stream), p, 1 if startOpen else 0) != 0:
            raise NeuralAudioError(capi.last_error())

    def GetStreamGate(self, stream):
        """The constants in effect as a dict; None: no gate (or one that is being taken away)."""
        out = capi.NA_GateParams()
        rc = int(self._lib.NA_BatchGetStreamGate(self._h, int(stream), C.byref(out)))
        if rc < 0:
            raise NeuralAudioError(capi.last_error())
        return _gate_dict(out) if rc else None

    def StreamGateGain(self, stream):
        """The gate's gain at the last sample produced (1 without a gate).  Synchronises the batch: a diagnostic."""
        gain = float(self._lib.NA_BatchStreamGateGain(self._h, int(stream)))
        if gain < 0:
            raise NeuralAudioError(capi.last_error())
        return gain

    # -- the meter stage: EnableMeterStage is set-up side; SetStreamMeter and ReadStreamMeter are real-time safe (include/neuralaudio_amd.h) ----
    def EnableMeterStage(self):
        if self._lib.NA_BatchEnableMeterStage(self._h) != 0:
            raise NeuralAudioError(capi.last_error())

    def GetMeterInfo(self):
        info = capi.NA_MeterInfo()
        if self._lib.NA_BatchGetMeterInfo(self._h, C.byref(info)) != 0:
            raise NeuralAudioError(capi.last_error())
        return {name: int(getattr(info, name)) for name, _ in capi.NA_MeterInfo._fields_}

    def SetStreamMeter(self, stream, params):
        """Level and gain-reduction meters on the stream from the next sample on: `params` a dict of the NA_MeterParams fields
        (windowSamples, clipLevelIn, clipLevelOut); None takes the meter away at once.  A stream that has a meter restarts it."""
        p = None if params is None else C.byref(_meter_params(params))
        if self._lib.NA_BatchSetStreamMeter(self._h, int(stream), p) != 0:
            raise NeuralAudioError(capi.last_error())

    def GetStreamMeter(self, stream):
        """The constants in effect as a dict; None: no meter."""
        out = capi.NA_MeterParams()
        rc = int(self._lib.NA_BatchGetStreamMeter(self._h, int(stream), C.byref(out)))
        if rc < 0:
            raise NeuralAudioError(capi.last_error())
        return {"windowSamples": int(out.windowSamples), "clipLevelIn": float(out.clipLevelIn), "clipLevelOut": float(out.clipLevelOut)} if rc else None

    def ReadStreamMeter(self, stream):
        """The newest reading that has arrived on the host, as a dict (windows, in, out, gateGainMin, gateGainLast, windowSamples; the
        taps: energy, oversTotal, peak, peakHold, overs); None: no meter, or no completed window has arrived yet.  Never waits."""
        out = capi.NA_MeterReading()
        rc = int(self._lib.NA_BatchReadStreamMeter(self._h, int(stream), C.byref(out)))
        if rc < 0:
            raise NeuralAudioError(capi.last_error())
        return _meter_reading(out) if rc else None

    # -- the tuner stage: EnableTunerStage is set-up side; SetStreamTuner and ReadStreamTuner are real-time safe (include/neuralaudio_amd.h) ----
    def EnableTunerStage(self):
        if self._lib.NA_BatchEnableTunerStage(self._h) != 0:
            raise NeuralAudioError(capi.last_error())

    def GetTunerInfo(self):
        info = capi.NA_TunerInfo()
        if self._lib.NA_BatchGetTunerInfo(self._h, C.byref(info)) != 0:
            raise NeuralAudioError(capi.last_error())
        return {name: int(getattr(info, name)) for name, _ in capi.NA_TunerInfo._fields_}

    def SetStreamTuner(self, stream, params):
        """A pitch reading of the stream's input row every hopSamples from the next sample on: `params` a dict of the NA_TunerParams
        fields (tuner_params_from_range makes one); None takes the tuner away at once.  A stream that has a tuner restarts it."""
        p = None if params is None else C.byref(_tuner_params(params))
        if self._lib.NA_BatchSetStreamTuner(self._h, int(stream), p) != 0:
            raise NeuralAudioError(capi.last_error())

    def GetStreamTuner(self, stream):
        """The constants in effect as a dict; None: no tuner."""
        out = capi.NA_TunerParams()
        rc = int(self._lib.NA_BatchGetStreamTuner(self._h, int(stream), C.byref(out)))
        if rc < 0:
            raise NeuralAudioError(capi.last_error())
        return _tuner_dict(out) if rc else None

    def ReadStreamTuner(self, stream):
        """The newest reading that has arrived on the host, as a dict (evaluations, position, r, e0, e, lag, decimation; tuner_pitch turns
        it into Hz); None: no tuner, or no evaluation has arrived yet.  Never waits."""
        out = capi.NA_TunerReading()
        rc = int(self._lib.NA_BatchReadStreamTuner(self._h, int(stream), C.byref(out)))
        if rc < 0:
            raise NeuralAudioError(capi.last_error())
        return _tuner_reading(out) if rc else None

    # -- the mix stage: EnableMixStage is set-up side; SetMixGroup and ClearMixGroup are real-time safe (include/neuralaudio_amd.h) ----
    def EnableMixStage(self):
        if self._lib.NA_BatchEnableMixStage(self._h) != 0:
            raise NeuralAudioError(capi.last_error())

    def GetMixInfo(self):
        info = capi.NA_MixInfo()
        if self._lib.NA_BatchGetMixInfo(self._h, C.byref(info)) != 0:
            raise NeuralAudioError(capi.last_error())
        return {name: int(getattr(info, name)) for name, _ in capi.NA_MixInfo._fields_}

    def SetMixGroup(self, streams, gains, numOutputs=None, taps=None, rampSamples=0):
        """A mix group of the members `streams` (`taps`: 0 OUT / 1 DRY per member, None: all OUT) whose first numOutputs rows (default:
        the rows of `gains`) become the sums `gains` [numOutputs][numMembers] says, ramped over rampSamples.  The member list of an
        existing group: a gain change from the gains reached."""
        streams = [int(s) for s in streams]
        g = np.ascontiguousarray(np.asarray(gains, dtype=np.float32))
        M = len(streams)
        D = int(numOutputs) if numOutputs is not None else (g.shape[0] if g.ndim == 2 else 1)
        if g.size != D * M:
            raise ValueError("gains must be [numOutputs][numMembers]")
        ids = (C.c_int * max(M, 1))(*streams)
        t = None if taps is None else (C.c_int * max(M, 1))(*[int(x) for x in taps])
        if taps is not None and len(taps) != M:
            raise ValueError("taps must name a tap per member")
        if self._lib.NA_BatchSetMixGroup(self._h, ids, t, M, D, g.ctypes.data_as(C.POINTER(C.c_float)), int(rampSamples)) != 0:
            raise NeuralAudioError(capi.last_error())

    def ClearMixGroup(self, stream):
        if self._lib.NA_BatchClearMixGroup(self._h, int(stream)) != 0:
            raise NeuralAudioError(capi.last_error())

    def GetStreamMix(self, stream):
        """The group that names the stream as a dict (streams, taps, numOutputs, gains [numOutputs][numMembers]: the target); None: no group."""
        cap = capi.NA_MIX_MAX_MEMBERS
        ids, taps, D = (C.c_int * cap)(), (C.c_int * cap)(), C.c_int(0)
        g = (C.c_float * (cap * cap))()
        M = int(self._lib.NA_BatchGetStreamMix(self._h, int(stream), ids, taps, cap, C.byref(D), g))
        if M < 0:
            raise NeuralAudioError(capi.last_error())
        if M == 0:
            return None
        return {"streams": list(ids[:M]), "taps": list(taps[:M]), "numOutputs": int(D.value),
                "gains": np.array(g[:D.value * M], dtype=np.float32).reshape(D.value, M)}

    def MixRampRemaining(self, stream):
        rc = int(self._lib.NA_BatchMixRampRemaining(self._h, int(stream)))
        if rc < 0:
            raise NeuralAudioError(capi.last_error())
        return rc

    # -- the EQ stage: EnableEqStage is set-up side; SetStreamEq is real-time safe (include/neuralaudio_amd.h) ----
    def EnableEqStage(self):
        if self._lib.NA_BatchEnableEqStage(self._h) != 0:
            raise NeuralAudioError(capi.last_error())

    def GetEqInfo(self):
        info = capi.NA_EqInfo()
        if self._lib.NA_BatchGetEqInfo(self._h, C.byref(info)) != 0:
            raise NeuralAudioError(capi.last_error())
        return {name: int(getattr(info, name)) for name, _ in capi.NA_EqInfo._fields_}

    def SetStreamEq(self, stream, sections, fadeSamples=0):
        """A cascade of up to 8 biquad sections on the stream from the next sample on, faded in over fadeSamples samples: `sections` a
        list of dicts of the NA_EqSection fields (eq_section designs one); None or an empty list is the flat cascade.  The new cascade
        starts from the state of the one the stream has."""
        sections = [] if sections is None else list(sections)
        arr = (capi.NA_EqSection * max(len(sections), 1))(*[_eq_section(s) for s in sections])
        if self._lib.NA_BatchSetStreamEq(self._h, int(stream), arr if sections else None, len(sections), int(fadeSamples)) != 0:
            raise NeuralAudioError(capi.last_error())

    def GetStreamEq(self, stream):
        """The sections of the target cascade as a list of dicts; an empty list: flat."""
        out = (capi.NA_EqSection * capi.NA_EQ_MAX_SECTIONS)()
        count = int(self._lib.NA_BatchGetStreamEq(self._h, int(stream), out, capi.NA_EQ_MAX_SECTIONS))
        if count < 0:
            raise NeuralAudioError(capi.last_error())
        return [_eq_dict(out[i]) for i in range(count)]

    def StreamEqFadeRemaining(self, stream):
        left = int(self._lib.NA_BatchStreamEqFadeRemaining(self._h, int(stream)))
        if left < 0:
            raise NeuralAudioError(capi.last_error())
        return left

    def DebugRunEqStage(self, rows, n=None):
        """Test hook: the stage of a call of n samples, in place on the float32 array rows[NumStreams, stride] (NA_DebugRunEqStage)."""
        return self._debug_run_stage(self._lib.NA_DebugRunEqStage, rows, n)

    def SetQuality(self, stream, q):
        if self._lib.NA_BatchSetQuality(self._h, int(stream), float(q)) != 0:
            raise NeuralAudioError(capi.last_error())

    # -- batch resampling (include/neuralaudio_amd.h) ------------------------------------------------------------
    def SetResampling(self, external_rate, model_rate=48000, quantum=0, max_frames=512):
        """Set-up call before the first AddStreams: every n of the processing entry points now counts samples at `external_rate`."""
        if self._lib.NA_BatchSetResampling(self._h, int(external_rate), int(model_rate), int(quantum), int(max_frames)) != 0:
            raise NeuralAudioError(capi.last_error())

    def ResampleInfo(self):
        """The resampling plan in effect (see resample_plan); raises if SetResampling was never called."""
        info = capi.NA_ResampleInfo()
        if self._lib.NA_BatchGetResampleInfo(self._h, C.byref(info)) != 0:
            raise NeuralAudioError(capi.last_error())
        return _resample_info(info)

    def DebugResampleTap(self, capacity=4096):
        """Test hook: (model_in, model_out), the model-rate rows [streams, frames] of the last processing call (NA_DebugResampleTap)."""
        rows = self.NumStreams()
        u = np.zeros((rows, int(capacity)), np.float32)
        v = np.zeros((rows, int(capacity)), np.float32)
        frames = C.c_int(0)
        if self._lib.NA_DebugResampleTap(self._h, _fptr(u), _fptr(v), int(capacity), C.byref(frames)) != 0:
            raise NeuralAudioError(capi.last_error())
        f = int(frames.value)
        return (u.reshape(-1)[:rows * f].reshape(rows, f).copy(), v.reshape(-1)[:rows * f].reshape(rows, f).copy())

    # -- stream snapshots: not real-time safe (they wait for everything in flight), call between buffers ---------------------------
    def StreamSnapshotBytes(self, stream):
        n = int(self._lib.NA_BatchStreamSnapshotBytes(self._h, int(stream)))
        if n < 0:
            raise NeuralAudioError(capi.last_error())
        return n

    def SaveStreams(self, streams):
        """The snapshots of `streams` (an id or a sequence of ids) back to back as bytes: one launch per model, one download."""
        ids = np.atleast_1d(np.asarray(streams, dtype=np.int32))
        idp = ids.ctypes.data_as(C.POINTER(C.c_int))
        need = sum(self.StreamSnapshotBytes(int(s)) for s in ids)
        buf = C.create_string_buffer(max(need, 1))
        written = C.c_size_t(0)
        if self._lib.NA_BatchSaveStreams(self._h, idp, ids.size, buf, need, C.byref(written)) != 0:
            raise NeuralAudioError(capi.last_error())
        return buf.raw[:written.value]

    def LoadStreams(self, streams, blob):
        """The inverse: snapshot i of `blob` goes to streams[i].  All or nothing: raises (naming the reason) before any stream changed."""
        ids = np.atleast_1d(np.asarray(streams, dtype=np.int32))
        blob = bytes(blob)
        if self._lib.NA_BatchLoadStreams(self._h, ids.ctypes.data_as(C.POINTER(C.c_int)), ids.size, blob, len(blob)) != 0:
            raise NeuralAudioError(capi.last_error())

    def IsQualityChangeRealtimeSafe(self, stream, q):
        return bool(self._lib.NA_BatchIsQualityChangeRealtimeSafe(self._h, int(stream), float(q)))

    def GetActiveSubModel(self, stream):
        return int(self._lib.NA_BatchGetActiveSubModel(self._h, int(stream)))

    def Prewarm(self, stream=-1):
        if self._lib.NA_BatchPrewarm(self._h, int(stream)) != 0:
            raise NeuralAudioError(capi.last_error())

    def Process(self, x):
        """x: host array [streams, n] -> host array [streams, n] (synchronous)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert x.ndim == 2 and x.shape[0] == self.NumStreams(), "expected [streams, n]"
        y = np.empty_like(x)
        if self._lib.NA_BatchProcess(self._h, _fptr(x), _fptr(y), x.shape[1]) != 0:
            raise NeuralAudioError(capi.last_error())
        return y

    def Submit(self, x):
        """Pipelined variant of Process: returns a ticket for Collect(); up to 3 buffers may be in flight."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert x.ndim == 2 and x.shape[0] == self.NumStreams(), "expected [streams, n]"
        t = self._lib.NA_BatchSubmit(self._h, _fptr(x), x.shape[1])
        if t < 0:
            raise NeuralAudioError(capi.last_error())
        return t, x.shape

    def Collect(self, ticket):
        t, shape = ticket
        y = np.empty(shape, np.float32)
        if self._lib.NA_BatchCollect(self._h, int(t), _fptr(y)) != 0:
            raise NeuralAudioError(capi.last_error())
        return y

    def NextInput(self, n):
        """Zero-copy: a numpy view [streams, n] of the pinned staging buffer of the next submission; fill it, then SubmitInput(n)."""
        p = self._lib.NA_BatchNextInput(self._h, int(n))
        if not p:
            raise NeuralAudioError(capi.last_error())
        return np.ctypeslib.as_array(p, shape=(self.NumStreams(), int(n)))

    def SubmitInput(self, n):
        t = self._lib.NA_BatchSubmit(self._h, None, int(n))
        if t < 0:
            raise NeuralAudioError(capi.last_error())
        return t, (self.NumStreams(), int(n))

    def CollectView(self, ticket):
        """Zero-copy: waits for the buffer and returns a numpy view of the pinned result (valid for the next 2 submissions)."""
        t, shape = ticket
        if self._lib.NA_BatchCollect(self._h, int(t), None) != 0:
            raise NeuralAudioError(capi.last_error())
        return np.ctypeslib.as_array(self._lib.NA_BatchOutputView(self._h, int(t)), shape=shape)

    def ProcessDevice(self, d_in, d_out, n, in_stride=None, out_stride=None):
        """d_in / d_out: raw device pointers (ints); asynchronous on the batch's HIP stream."""
        rc = self._lib.NA_BatchProcessDevice(self._h, C.c_void_p(d_in), C.c_void_p(d_out), int(n),
                                             int(in_stride if in_stride is not None else n),
                                             int(out_stride if out_stride is not None else n))
        if rc != 0:
            raise NeuralAudioError(capi.last_error())

    def Synchronize(self):
        if self._lib.NA_BatchSynchronize(self._h) != 0:
            raise NeuralAudioError(capi.last_error())

    def WaitOutputs(self):
        """Host-side wait until every buffer handed to ProcessDevice so far has been processed (the resident launch stays up)."""
        if self._lib.NA_BatchWaitOutputs(self._h) != 0:
            raise NeuralAudioError(capi.last_error())

    def SetWaitLimitMs(self, ms):
        """Wall-clock limit of every host-side wait of this batch (NA_BatchSetWaitLimitMs; <= 0: none).  A wait that runs into it breaks the batch."""
        self._lib.NA_BatchSetWaitLimitMs(self._h, float(ms))

    def GetWaitLimitMs(self):
        return float(self._lib.NA_BatchGetWaitLimitMs(self._h))

    def IsBroken(self):
        return bool(self._lib.NA_BatchIsBroken(self._h))

    def DebugStallDevice(self, ms):
        """Test hook: keep the batch's streams busy for `ms` milliseconds (NA_DebugStallDevice)."""
        if self._lib.NA_DebugStallDevice(self._h, float(ms)) != 0:
            raise NeuralAudioError(capi.last_error())

    def DebugLastHostRoute(self):
        """Test hook: the route the last processing call took, a value of HOST_ROUTES (NA_DebugLastHostRoute); -1 before any call."""
        return int(self._lib.NA_DebugLastHostRoute(self._h))

    def SetResidentLaunch(self, on=True):
        """Opt in to (or out of) the resident launch for device-pointer buffers of this batch (NA_BatchSetResidentLaunch)."""
        if self._lib.NA_BatchSetResidentLaunch(self._h, 1 if on else 0) != 0:
            raise NeuralAudioError(capi.last_error())

    def UsesResidentLaunch(self):
        """True when the last ProcessDevice call was a command to the resident launch (own stream, >= 512 A1 Standard streams)."""
        return bool(self._lib.NA_BatchUsesResidentLaunch(self._h))

    def GetHipStream(self):
        """The batch's HIP stream handle (int).  From the first call on every launch is ordered on it (see NA_BatchGetHipStream)."""
        return self._lib.NA_BatchGetHipStream(self._h)

    def MarkTime(self, which):
        """HIP events on every stream the batch launches on (0: start, 1: end); see ElapsedMs."""
        if self._lib.NA_BatchMarkTime(self._h, int(which)) != 0:
            raise NeuralAudioError(capi.last_error())

    def WaitMarks(self):
        """Polls until the marks of MarkTime(1) are reached on every stream the batch launches on."""
        if self._lib.NA_BatchWaitMarks(self._h) != 0:
            raise NeuralAudioError(capi.last_error())

    def ElapsedMs(self):
        ms = float(self._lib.NA_BatchElapsedMs(self._h))
        if ms < 0:
            raise NeuralAudioError(capi.last_error())
        return ms

    def UsesHalfLaunches(self):
        """True when the last ProcessDevice call ran as two free-running half-batch launches (own stream, one WaveNet group)."""
        return bool(self._lib.NA_BatchUsesHalfLaunches(self._h))

    def AlgorithmicBytesPerSample(self, block_frames=128):
        return float(self._lib.NA_BatchAlgorithmicBytesPerSample(self._h, int(block_frames)))

    def MacsPerSample(self):
        return float(self._lib.NA_BatchMacsPerSample(self._h))

    def StateBytes(self):
        return float(self._lib.NA_BatchStateBytes(self._h))

    def StreamKernelName(self, stream):
        return self._lib.NA_BatchStreamKernelName(self._h, int(stream)).decode()

    def StreamInputLimit(self, stream):
        return float(self._lib.NA_BatchStreamInputLimit(self._h, int(stream)))

    def StreamPackFactor(self, stream):
        return int(self._lib.NA_BatchStreamPackFactor(self._h, int(stream)))

    def StreamRangeEvents(self, stream):
        r = int(self._lib.NA_BatchStreamRangeEvents(self._h, int(stream)))
        if r < 0:
            raise NeuralAudioError(capi.last_error())
        return r

    def close(self):
        if self._h:
            self._lib.NA_BatchDestroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiBatch:
    """The C++ multi-GPU host (csrc/multi_gpu.cpp): one batch + one host thread per entry of `devices`, the global stream list sharded
    across them by cost.  Rows of the [streams][n] arrays are global stream ids."""

    def __init__(self, devices):
        self._lib = capi.load_library()
        arr = (C.c_int * len(devices))(*[int(d) for d in devices])
        self._h = self._lib.NA_MultiCreate(arr, len(devices))
        if not self._h:
            raise NeuralAudioError(capi.last_error())

    def AddStreams(self, model, count=1, quality=1.0, doPrewarm=True):
        first = self._lib.NA_MultiAddStreams(self._h, model._h, float(quality), int(count), 1 if doPrewarm else 0)
        if first < 0:
            raise NeuralAudioError(capi.last_error())
        return first

    def SetFanIn(self, mode):
        """"host" (default): every shard serves its own rows of the host arrays; "rccl": weights replicated and outputs gathered over RCCL."""
        if self._lib.NA_MultiSetFanIn(self._h, {"host": 0, "rccl": 1}[mode]) != 0:
            raise NeuralAudioError(capi.last_error())

    def Commit(self):
        if self._lib.NA_MultiCommit(self._h) != 0:
            raise NeuralAudioError(capi.last_error())

    def NumStreams(self):
        return int(self._lib.NA_MultiNumStreams(self._h))

    def ShardRanges(self):
        out = []
        for s in range(int(self._lib.NA_MultiNumShards(self._h))):
            b, e, d = C.c_int(), C.c_int(), C.c_int()
            if self._lib.NA_MultiShardRange(self._h, s, C.byref(b), C.byref(e), C.byref(d)) != 0:
                raise NeuralAudioError(capi.last_error())
            out.append((b.value, e.value, d.value))
        return out

    def Process(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert x.ndim == 2 and x.shape[0] == self.NumStreams(), "expected [streams, n]"
        y = np.empty_like(x)
        if self._lib.NA_MultiProcess(self._h, _fptr(x), _fptr(y), x.shape[1]) != 0:
            raise NeuralAudioError(capi.last_error())
        return y

    def SetResampling(self, external_rate, model_rate=48000, quantum=0, max_frames=512):
        """Before Commit: every shard's batch becomes a resampling batch of this plan; every n then counts samples at `external_rate`."""
        if self._lib.NA_MultiSetResampling(self._h, int(external_rate), int(model_rate), int(quantum), int(max_frames)) != 0:
            raise NeuralAudioError(capi.last_error())

    def ResampleInfo(self):
        """The resampling plan in effect (see resample_plan); raises if SetResampling was never called."""
        info = capi.NA_ResampleInfo()
        if self._lib.NA_MultiGetResampleInfo(self._h, C.byref(info)) != 0:
            raise NeuralAudioError(capi.last_error())
        return _resample_info(info)

    def Submit(self, x):
        """Pipelined variant of Process (NA_MultiSubmit, host-rows fan-in): returns a ticket for Collect()."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert x.ndim == 2 and x.shape[0] == self.NumStreams(), "expected [streams, n]"
        t = self._lib.NA_MultiSubmit(self._h, _fptr(x), x.shape[1])
        if t < 0:
            raise NeuralAudioError(capi.last_error())
        return t, x.shape

    def Collect(self, ticket):
        t, shape = ticket
        y = np.empty(shape, np.float32)
        if self._lib.NA_MultiCollect(self._h, int(t), _fptr(y)) != 0:
            raise NeuralAudioError(capi.last_error())
        return y

    def DebugLastHostRoute(self, shard):
        """Test hook: Batch.DebugLastHostRoute of the batch of `shard` (NA_DebugMultiLastHostRoute)."""
        return int(self._lib.NA_DebugMultiLastHostRoute(self._h, int(shard)))

    def GatheredOutput(self, shard, n):
        """RCCL fan-in: the [streams][n] device buffer of the last Process() on `shard`'s GPU, copied to the host (tests)."""
        ptr = self._lib.NA_MultiGatheredOutput(self._h, int(shard))
        if not ptr:
            raise NeuralAudioError("no gathered output (RCCL fan-in only, after Process)")
        out = np.empty((self.NumStreams(), int(n)), dtype=np.float32)
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        if hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes, 2) != 0:  # hipMemcpyDeviceToHost
            raise NeuralAudioError("hipMemcpy of the gathered output failed")
        return out

    def SetQuality(self, stream, q):
        if self._lib.NA_MultiSetQuality(self._h, int(stream), float(q)) != 0:
            raise NeuralAudioError(capi.last_error())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.NA_MultiDestroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _resample_info(info):
    return {"external_rate": info.externalRate, "model_rate": info.modelRate, "te": info.ticksExternal, "tm": info.ticksModel,
            "taps_up": info.tapsUp, "taps_down": info.tapsDown, "quantum": info.quantum, "latency_samples": info.latencySamples,
            "prototype_length": info.prototypeLength}


def resample_plan(external_rate, model_rate=48000, quantum=0):
    """The resampling plan of a rate pair (NA_ResamplePlan; host arithmetic, no device): te, tm, taps, quantum, latency, K."""
    info = capi.NA_ResampleInfo()
    if capi.load_library().NA_ResamplePlan(int(external_rate), int(model_rate), int(quantum), C.byref(info)) != 0:
        raise NeuralAudioError(capi.last_error())
    return _resample_info(info)


def resample_prototype(external_rate, model_rate=48000):
    """The f32 prototype low-pass of a rate pair at the common rate (NA_ResamplePrototype), as a numpy array of length K."""
    lib = capi.load_library()
    k = int(lib.NA_ResamplePrototype(int(external_rate), int(model_rate), None, 0))
    if k < 0:
        raise NeuralAudioError(capi.last_error())
    h = np.zeros(k, np.float32)
    lib.NA_ResamplePrototype(int(external_rate), int(model_rate), _fptr(h), k)
    return h


def resample_model_frames(external_rate, model_rate, quantum, external_samples):
    """Model frames P(E) a resampling batch has run after E external samples (NA_ResampleModelFrames)."""
    f = int(capi.load_library().NA_ResampleModelFrames(int(external_rate), int(model_rate), int(quantum), int(external_samples)))
    if f < 0:
        raise NeuralAudioError(capi.last_error())
    return f


def snapshot_bytes(model):
    """Bytes of one stream snapshot of `model` (host arithmetic: no batch, no device)."""
    n = int(capi.load_library().NA_ModelSnapshotBytes(model._h))
    if n < 0:
        raise NeuralAudioError(capi.last_error())
    return n


def snapshot_fingerprint(model):
    """The model fingerprint a snapshot carries: architecture + weights of every submodel, nothing kernel-specific."""
    return int(capi.load_library().NA_ModelSnapshotFingerprint(model._h))


def _render_jobs(model, x, quality):
    """(model, x, quality) or a list of (model, x[, quality]) -> (ctypes job array, [input arrays], [output arrays], list form?)"""
    many = isinstance(model, (list, tuple))
    specs = model if many else [(model, x, quality)]
    if not specs:
        raise NeuralAudioError("render_offline: no jobs")
    jobs = (capi.NA_RenderJob * len(specs))()
    xs, ys = [], []
    for i, spec in enumerate(specs):
        m, xi = spec[0], spec[1]
        q = float(spec[2]) if len(spec) > 2 else 1.0
        xi = np.ascontiguousarray(xi, dtype=np.float32).reshape(-1)
        yi = np.empty_like(xi)
        xs.append(xi)
        ys.append(yi)
        jobs[i].model = m._h if m is not None else None
        jobs[i].quality = q
        jobs[i].input = _fptr(xi)
        jobs[i].output = _fptr(yi)
        jobs[i].numSamples = xi.size
    return jobs, xs, ys, many


def _render_options(segment_samples, max_samples_per_pass, wait_limit_ms):
    return capi.NA_RenderOptions(int(segment_samples), int(max_samples_per_pass), float(wait_limit_ms))


def render_offline(model, x=None, quality=1.0, segment_samples=0, max_samples_per_pass=0, wait_limit_ms=0.0, external_rate=None):
    """Renders a whole signal through `model` as a fresh, prewarmed instance would (NA_RenderOffline: time-parallel segments for WaveNet
    models, one sequential stream per recurrent job).  float32 in, float32 out, same length.  List form: render_offline([(model, x,
    quality), ...]) renders every job in one call and returns the list of outputs.  The model's own stream state is not touched.
    external_rate: the signals are at this sample rate, whatever rate each model runs at (NA_RenderOfflineAtRate: resampled on the
    device, latency-compensated; segment_samples and max_samples_per_pass then count model-rate frames).  None: NA_RenderOffline."""
    jobs, xs, ys, many = _render_jobs(model, x, quality)
    opts = _render_options(segment_samples, max_samples_per_pass, wait_limit_ms)
    lib = capi.load_library()
    rc = (lib.NA_RenderOffline(jobs, len(xs), C.byref(opts)) if external_rate is None
          else lib.NA_RenderOfflineAtRate(jobs, len(xs), C.byref(opts), int(external_rate)))
    if rc != 0:
        raise NeuralAudioError(capi.last_error())
    return ys if many else ys[0]


def debug_render_tap(model, x=None, quality=1.0, external_rate=48000, **options):
    """Test hook (NA_DebugSetRenderTap): render_offline(..., external_rate=...) that also returns job 0's model-rate input and output,
    (out, u, v)."""
    lib = capi.load_library()
    first = model[0] if isinstance(model, (list, tuple)) else (model, x, quality)
    n = np.asarray(first[1]).size
    info = resample_plan(external_rate, first[0].GetModelProcessRate(), 1)
    m = resample_model_frames(external_rate, info["model_rate"], 1, n + info["latency_samples"])
    u = np.zeros(max(m, 1), np.float32)
    v = np.zeros(max(m, 1), np.float32)
    lib.NA_DebugSetRenderTap(_fptr(u), _fptr(v), m)
    try:
        out = render_offline(model, x, quality, external_rate=external_rate, **options)
    finally:
        lib.NA_DebugSetRenderTap(None, None, 0)
    return out, u[:m], v[:m]


def render_plan(model, x=None, quality=1.0, segment_samples=0, max_samples_per_pass=0, external_rate=None):
    """The plan render_offline would run (NA_RenderPlan; no device needed): segments, lead, segment_samples, row_samples, passes,
    streams, estimated_ms and -- with a device -- the kernel of the first segment.  `x` may be an array or a sample count.
    external_rate: the plan of render_offline(..., external_rate=...) (NA_RenderPlanAtRate): the same figures in model-rate frames plus
    "resample", the resampling plan of job 0's rate pair."""
    def as_signal(v):
        return np.zeros(int(v), dtype=np.float32) if np.isscalar(v) else v
    if isinstance(model, (list, tuple)):
        model = [(s[0], as_signal(s[1])) + tuple(s[2:]) for s in model]
    else:
        x = as_signal(x)
    jobs, xs, ys, _ = _render_jobs(model, x, quality)
    opts = _render_options(segment_samples, max_samples_per_pass, 0.0)
    info = capi.NA_RenderPlanInfo()
    rs = capi.NA_ResampleInfo()
    lib = capi.load_library()
    rc = (lib.NA_RenderPlan(jobs, len(xs), C.byref(opts), C.byref(info)) if external_rate is None
          else lib.NA_RenderPlanAtRate(jobs, len(xs), C.byref(opts), int(external_rate), C.byref(info), C.byref(rs)))
    if rc != 0:
        raise NeuralAudioError(capi.last_error())
    plan = {"segments": info.segments, "lead": info.lead, "segment_samples": info.segmentSamples, "row_samples": info.rowSamples,
            "passes": info.passes, "streams": info.streams, "estimated_ms": info.estimatedMs, "kernel": info.kernel.decode()}
    if external_rate is not None:
        plan["resample"] = _resample_info(rs)
    return plan
