"""ctypes binding of libNeuralAudioCAPI.so -- the reference-side binding a maintainer would write.

Everything here goes through the C ABI declared in include/NeuralAudioCApi.h (the 15 legacy symbols
of the reference's NeuralAudioCAPI) and include/neuralaudio_amd.h (the additive NA_* batch API).
There is no Python compute path and no CPU fallback: if the shared library (with its embedded gfx950
code objects) is missing, importing this module raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# NA_LIB_SUFFIX selects a tuning build (tools/ablate.sh); unset in normal use
_SUFFIX = os.environ.get("NA_LIB_SUFFIX", "")
LIB_PATH = (os.path.join(os.path.dirname(_HERE), "tools", "variants", "libNeuralAudioCAPI%s.so" % _SUFFIX) if _SUFFIX
            else os.path.join(_HERE, "libNeuralAudioCAPI.so"))

LEGACY_SYMBOLS = [
    "CreateLoader", "DeleteLoader", "CreateModelFromFile", "DeleteModel", "SetLSTMLoadMode", "SetWaveNetLoadMode",
    "SetAudioInputLevelDBu", "SetDefaultMaxAudioBufferSize", "GetLoadMode", "IsStatic", "SetMaxAudioBufferSize",
    "GetRecommendedInputDBAdjustment", "GetRecommendedOutputDBAdjustment", "GetSampleRate", "Process",
]

NA_SYMBOLS = [
    "NA_GetLastError", "NA_GetDeviceCount", "NA_GetVersion", "NA_CreateModelFromFileUtf8", "NA_CreateModelFromString",
    "NA_SetDevice", "NA_SetDefaultQualityScaleFactor", "NA_SetExternalSampleRate", "NA_HasQualityScaling",
    "NA_GetQualityScaleFactor", "NA_SetQualityScaleFactor", "NA_GetReceptiveFieldSize", "NA_Prewarm", "NA_GetMetadata",
    "NA_GetModelVersion", "NA_BatchCreate", "NA_BatchDestroy", "NA_BatchAddStreams", "NA_BatchNumStreams",
    "NA_BatchSetQuality", "NA_BatchGetActiveSubModel", "NA_BatchPrewarm", "NA_BatchProcess", "NA_BatchProcessDevice",
    "NA_BatchSynchronize", "NA_BatchGetHipStream", "NA_BatchAlgorithmicBytesPerSample", "NA_BatchMacsPerSample",
    "NA_BatchStateBytes", "NA_BatchStreamPackFactor", "NA_BatchStreamKernelName", "NA_DebugSetTraceBuffer", "NA_DebugSetWaveNetSpec", "NA_DebugSetRecurrentQuadMin", "NA_DebugRecurrentQuadLaunches", "NA_RegisterHostBuffer", "NA_UnregisterHostBuffer", "NA_BatchStreamInputLimit", "NA_BatchRemoveStreams", "NA_MultiCreate", "NA_MultiDestroy", "NA_MultiAddStreams", "NA_MultiCommit", "NA_MultiNumStreams", "NA_MultiNumShards", "NA_MultiShardRange", "NA_MultiProcess", "NA_MultiSubmit", "NA_MultiCollect", "NA_MultiSetQuality", "NA_ShardByCost", "NA_ModelStreamCost", "NA_BatchNumLiveStreams", "NA_BatchIsLive", "NA_SetWaveNetMathMode", "NA_SetLSTMMathMode", "NA_SetCompositeModelLoadMode",
    "NA_IsQualityChangeRealtimeSafe", "NA_ProcessChecked", "NA_BatchSubmit", "NA_BatchCollect", "NA_BatchNextInput", "NA_BatchOutputView", "NA_BatchIsQualityChangeRealtimeSafe", "NA_DebugClassifyNam", "NA_DebugPackedWeights", "NA_DebugSplitPlan", "NA_ModelKernelInfo", "NA_BatchStreamRangeEvents", "NA_MultiSetFanIn", "NA_MultiGatheredOutput", "NA_RcclAvailable",
    "NA_BatchMarkTime", "NA_BatchWaitMarks", "NA_BatchElapsedMs", "NA_BatchUsesHalfLaunches", "NA_DebugSetRcclApi", "NA_BatchWaitOutputs", "NA_BatchUsesResidentLaunch", "NA_BatchSetResidentLaunch",
    "NA_BatchSetWaitLimitMs", "NA_BatchGetWaitLimitMs", "NA_BatchIsBroken", "NA_DebugStallDevice", "NA_DebugLastHostRoute", "NA_DebugMultiLastHostRoute",
    "NA_RenderOffline", "NA_RenderPlan",
    "NA_BatchStreamSnapshotBytes", "NA_ModelSnapshotBytes", "NA_ModelSnapshotFingerprint", "NA_BatchSaveStreams", "NA_BatchLoadStreams",
    "NA_SaveModelState", "NA_LoadModelState", "NA_DebugSnapshotLaunches",
    "NA_ResamplePlan", "NA_ResamplePrototype", "NA_ResampleModelFrames", "NA_BatchSetResampling", "NA_BatchGetResampleInfo",
    "NA_SetResampleToExternalRate", "NA_GetProcessLatencySamples", "NA_GetModelProcessRate", "NA_DebugResampleTap",
    "NA_RenderOfflineAtRate", "NA_RenderPlanAtRate", "NA_DebugSetRenderTap", "NA_MultiSetResampling", "NA_MultiGetResampleInfo",
    "NA_BatchReserveStreams", "NA_BatchActivateStream", "NA_BatchParkStream", "NA_BatchIsParked", "NA_BatchFindParked", "NA_BatchNumParked",
    "NA_DebugDeviceResourceCalls", "NA_DebugRecurrentPlan", "NA_DebugRecurrentShapePlan", "NA_DebugRecurrentKernel",
    "NA_DebugWaveNetKernel", "NA_DebugWaveNetLaunch",
    "NA_BatchEnableOutputStage", "NA_BatchSetStreamGain", "NA_BatchGetStreamGain", "NA_BatchHandover", "NA_BatchHandoverRemaining",
    "NA_BatchEnableCabinetStage", "NA_BatchGetCabinetInfo", "NA_BatchLoadIR", "NA_BatchUnloadIR", "NA_BatchSetStreamIR", "NA_BatchGetStreamIR",
    "NA_BatchStreamIRFadeRemaining", "NA_DebugRunCabinetStage", "NA_DebugCabinetLaunches",
    "NA_BatchEnableReverbStage", "NA_BatchGetReverbInfo", "NA_BatchLoadReverbIR", "NA_BatchUnloadReverbIR", "NA_BatchSetStreamReverb",
    "NA_BatchGetStreamReverb", "NA_BatchStreamReverbFadeRemaining", "NA_DebugRunReverbStage", "NA_DebugReverbLaunches", "NA_DebugReverbTwiddles",
    "NA_DelayParamsFromMs", "NA_BatchEnableDelayStage", "NA_BatchGetDelayInfo", "NA_BatchSetStreamDelay", "NA_BatchGetStreamDelay",
    "NA_BatchStreamDelayFadeRemaining", "NA_DebugRunDelayStage", "NA_DebugDelayLaunches",
    "NA_CompressorParamsFromDb", "NA_BatchEnableCompressorStage", "NA_BatchGetCompressorInfo", "NA_BatchSetStreamCompressor",
    "NA_BatchGetStreamCompressor", "NA_BatchStreamCompressorFadeRemaining", "NA_BatchStreamCompressorGain", "NA_DebugRunCompressorStage",
    "NA_DebugCompressorLaunches",
    "NA_ModParamsFromMs", "NA_BatchEnableModStage", "NA_BatchGetModInfo", "NA_BatchSetStreamMod", "NA_BatchGetStreamMod",
    "NA_BatchStreamModFadeRemaining", "NA_DebugRunModStage", "NA_DebugModLaunches",
    "NA_GateParamsFromDb", "NA_BatchEnableGateStage", "NA_BatchGetGateInfo", "NA_BatchSetStreamGate", "NA_BatchGetStreamGate",
    "NA_BatchStreamGateGain", "NA_DebugGateLaunches",
    "NA_EqSectionFromDesign", "NA_BatchEnableEqStage", "NA_BatchGetEqInfo", "NA_BatchSetStreamEq", "NA_BatchGetStreamEq",
    "NA_BatchStreamEqFadeRemaining", "NA_DebugEqLaunches", "NA_DebugRunEqStage",
    "NA_BatchEnableMeterStage", "NA_BatchGetMeterInfo", "NA_BatchSetStreamMeter", "NA_BatchGetStreamMeter", "NA_BatchReadStreamMeter",
    "NA_DebugMeterLaunches",
    "NA_BatchEnableTunerStage", "NA_BatchGetTunerInfo", "NA_BatchSetStreamTuner", "NA_BatchGetStreamTuner", "NA_BatchReadStreamTuner",
    "NA_TunerParamsFromRange", "NA_TunerPitch", "NA_DebugTunerLaunches",
    "NA_BatchEnableMixStage", "NA_BatchGetMixInfo", "NA_BatchSetMixGroup", "NA_BatchClearMixGroup", "NA_BatchGetStreamMix",
    "NA_BatchMixRampRemaining", "NA_MixGainsFromPan", "NA_DebugMixLaunches", "NA_DebugMixStashLaunches", "NA_DebugRunMixStage",
]


class NA_RenderJob(C.Structure):
    _fields_ = [("model", C.c_void_p), ("quality", C.c_float), ("input", C.POINTER(C.c_float)), ("output", C.POINTER(C.c_float)),
                ("numSamples", C.c_size_t)]


class NA_RenderOptions(C.Structure):
    _fields_ = [("segmentSamples", C.c_size_t), ("maxSamplesPerPass", C.c_size_t), ("waitLimitMs", C.c_double)]


class NA_RenderPlanInfo(C.Structure):
    _fields_ = [("segments", C.c_longlong), ("lead", C.c_int), ("segmentSamples", C.c_longlong), ("rowSamples", C.c_longlong),
                ("passes", C.c_int), ("streams", C.c_int), ("estimatedMs", C.c_double), ("kernel", C.c_char * 64)]


class NA_ResampleInfo(C.Structure):
    _fields_ = [("externalRate", C.c_int), ("modelRate", C.c_int), ("ticksExternal", C.c_int), ("ticksModel", C.c_int),
                ("tapsUp", C.c_int), ("tapsDown", C.c_int), ("quantum", C.c_int), ("latencySamples", C.c_int),
                ("prototypeLength", C.c_int)]


class NA_CabinetInfo(C.Structure):
    _fields_ = [("maxTaps", C.c_int), ("ringSamples", C.c_int), ("pieceSamples", C.c_int), ("numIRs", C.c_int), ("deviceBytes", C.c_longlong)]


class NA_ReverbInfo(C.Structure):
    _fields_ = [("maxTaps", C.c_int), ("partitionSamples", C.c_int), ("slots", C.c_int), ("pieceSamples", C.c_int), ("numIRs", C.c_int),
                ("deviceBytes", C.c_longlong)]


class NA_DelayParams(C.Structure):
    _fields_ = [("delaySamples", C.c_int), ("feedback", C.c_float), ("lowpassCoeff", C.c_float), ("highpassCoeff", C.c_float),
                ("wet", C.c_float), ("dry", C.c_float)]


class NA_DelayInfo(C.Structure):
    _fields_ = [("maxDelaySamples", C.c_int), ("ringSamples", C.c_int), ("pieceSamples", C.c_int), ("numDelays", C.c_int),
                ("deviceBytes", C.c_longlong)]


NA_COMPRESSOR_CURVE_POINTS = 513


class NA_CompressorParams(C.Structure):
    _fields_ = [("attackCoeff", C.c_float), ("releaseCoeff", C.c_float), ("curve", C.c_float * NA_COMPRESSOR_CURVE_POINTS)]


class NA_CompressorInfo(C.Structure):
    _fields_ = [("curvePoints", C.c_int), ("numCompressors", C.c_int), ("deviceBytes", C.c_longlong)]


class NA_ModParams(C.Structure):
    _fields_ = [("baseSamples", C.c_float), ("depthSamples", C.c_float), ("phaseInc", C.c_uint), ("shape", C.c_int), ("numVoices", C.c_int),
                ("voicePhase", C.c_uint * 4), ("voiceGain", C.c_float * 4), ("feedback", C.c_float), ("wet", C.c_float), ("dry", C.c_float),
                ("tremoloDepth", C.c_float)]


class NA_ModInfo(C.Structure):
    _fields_ = [("maxDelaySamples", C.c_int), ("ringSamples", C.c_int), ("pieceSamples", C.c_int), ("numMods", C.c_int),
                ("deviceBytes", C.c_longlong)]


class NA_GateParams(C.Structure):
    _fields_ = [("openPower", C.c_float), ("closePower", C.c_float), ("floorGain", C.c_float), ("detectorCoeff", C.c_float),
                ("attackSamples", C.c_int), ("holdSamples", C.c_int), ("releaseSamples", C.c_int)]


class NA_GateInfo(C.Structure):
    _fields_ = [("gainSamples", C.c_int), ("numGates", C.c_int), ("deviceBytes", C.c_longlong)]


NA_EQ_MAX_SECTIONS = 8


class NA_EqSection(C.Structure):
    _fields_ = [("b0", C.c_double), ("b1", C.c_double), ("b2", C.c_double), ("a1", C.c_double), ("a2", C.c_double)]


class NA_EqInfo(C.Structure):
    _fields_ = [("maxSections", C.c_int), ("numEntries", C.c_int), ("deviceBytes", C.c_longlong)]


class NA_MeterParams(C.Structure):
    _fields_ = [("windowSamples", C.c_int), ("clipLevelIn", C.c_float), ("clipLevelOut", C.c_float)]


class NA_MeterTap(C.Structure):
    _fields_ = [("energy", C.c_ulonglong), ("oversTotal", C.c_ulonglong), ("peak", C.c_float), ("peakHold", C.c_float),
                ("overs", C.c_uint), ("reserved", C.c_uint)]


class NA_MeterReading(C.Structure):
    _fields_ = [("windows", C.c_ulonglong), ("in_", NA_MeterTap), ("out", NA_MeterTap), ("gateGainMin", C.c_float), ("gateGainLast", C.c_float),
                ("windowSamples", C.c_int), ("reserved", C.c_int)]


class NA_MeterInfo(C.Structure):
    _fields_ = [("numMeters", C.c_int), ("deviceBytes", C.c_longlong)]


class NA_TunerParams(C.Structure):
    _fields_ = [("decimation", C.c_int), ("windowSamples", C.c_int), ("minLag", C.c_int), ("maxLag", C.c_int), ("hopSamples", C.c_int), ("phase", C.c_int),
                ("thresholdQ10", C.c_int), ("reserved", C.c_int), ("minEnergy", C.c_ulonglong)]


class NA_TunerReading(C.Structure):
    _fields_ = [("evaluations", C.c_ulonglong), ("position", C.c_longlong), ("r", C.c_longlong * 3), ("e0", C.c_ulonglong), ("e", C.c_ulonglong * 3),
                ("lag", C.c_int), ("decimation", C.c_int)]


class NA_TunerInfo(C.Structure):
    _fields_ = [("numTuners", C.c_int), ("deviceBytes", C.c_longlong)]


NA_MIX_MAX_MEMBERS = 8
NA_MIX_TAP_OUT = 0
NA_MIX_TAP_DRY = 1


class NA_MixInfo(C.Structure):
    _fields_ = [("maxMembers", C.c_int), ("numGroups", C.c_int), ("drySamples", C.c_int), ("deviceBytes", C.c_longlong)]


_lib = None


def load_library():
    """Load the shared library; raises OSError if it has not been built (run __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError("libNeuralAudioCAPI.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; "
                      "g.build()'` (there is no CPU fallback)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    fp = C.POINTER(C.c_float)
    vp = C.c_void_p
    sig = {
        "CreateLoader": (vp, []),
        "DeleteLoader": (None, [vp]),
        "CreateModelFromFile": (vp, [vp, C.c_wchar_p]),
        "DeleteModel": (None, [vp]),
        "SetLSTMLoadMode": (None, [vp, C.c_int]),
        "SetWaveNetLoadMode": (None, [vp, C.c_int]),
        "SetAudioInputLevelDBu": (None, [vp, C.c_float]),
        "SetDefaultMaxAudioBufferSize": (None, [vp, C.c_int]),
        "GetLoadMode": (C.c_int, [vp]),
        "IsStatic": (C.c_bool, [vp]),
        "SetMaxAudioBufferSize": (None, [vp, C.c_int]),
        "GetRecommendedInputDBAdjustment": (C.c_float, [vp]),
        "GetRecommendedOutputDBAdjustment": (C.c_float, [vp]),
        "GetSampleRate": (C.c_float, [vp]),
        "Process": (None, [vp, fp, fp, C.c_size_t]),
        "NA_GetLastError": (C.c_char_p, []),
        "NA_GetDeviceCount": (C.c_int, []),
        "NA_GetVersion": (C.c_char_p, []),
        "NA_CreateModelFromFileUtf8": (vp, [vp, C.c_char_p, C.c_int]),
        "NA_CreateModelFromString": (vp, [vp, C.c_char_p, C.c_char_p, C.c_int]),
        "NA_SetDevice": (None, [vp, C.c_int]),
        "NA_SetDefaultQualityScaleFactor": (None, [vp, C.c_float]),
        "NA_SetExternalSampleRate": (None, [vp, C.c_int]),
        "NA_HasQualityScaling": (C.c_int, [vp]),
        "NA_GetQualityScaleFactor": (C.c_float, [vp]),
        "NA_SetQualityScaleFactor": (None, [vp, C.c_float]),
        "NA_GetReceptiveFieldSize": (C.c_int, [vp]),
        "NA_Prewarm": (C.c_int, [vp]),
        "NA_GetMetadata": (C.c_int, [vp, C.c_char_p, C.c_char_p, C.c_int]),
        "NA_GetModelVersion": (C.c_int, [vp, C.c_char_p, C.c_int]),
        "NA_BatchCreate": (vp, [C.c_int, vp]),
        "NA_BatchDestroy": (None, [vp]),
        "NA_BatchAddStreams": (C.c_int, [vp, vp, C.c_float, C.c_int, C.c_int]),
        "NA_BatchNumStreams": (C.c_int, [vp]),
        "NA_BatchSetQuality": (C.c_int, [vp, C.c_int, C.c_float]),
        "NA_BatchGetActiveSubModel": (C.c_int, [vp, C.c_int]),
        "NA_BatchPrewarm": (C.c_int, [vp, C.c_int]),
        "NA_BatchProcess": (C.c_int, [vp, fp, fp, C.c_size_t]),
        "NA_BatchProcessDevice": (C.c_int, [vp, vp, vp, C.c_size_t, C.c_long, C.c_long]),
        "NA_BatchSynchronize": (C.c_int, [vp]),
        "NA_BatchGetHipStream": (vp, [vp]),
        "NA_BatchMarkTime": (C.c_int, [vp, C.c_int]),
        "NA_BatchWaitMarks": (C.c_int, [vp]),
        "NA_BatchElapsedMs": (C.c_float, [vp]),
        "NA_BatchUsesHalfLaunches": (C.c_int, [vp]),
        "NA_BatchUsesResidentLaunch": (C.c_int, [vp]),
        "NA_BatchSetResidentLaunch": (C.c_int, [vp, C.c_int]),
        "NA_BatchWaitOutputs": (C.c_int, [vp]),
        "NA_BatchSetWaitLimitMs": (C.c_int, [vp, C.c_double]),
        "NA_BatchGetWaitLimitMs": (C.c_double, [vp]),
        "NA_BatchIsBroken": (C.c_int, [vp]),
        "NA_DebugStallDevice": (C.c_int, [vp, C.c_double]),
        "NA_DebugLastHostRoute": (C.c_int, [vp]),
        "NA_DebugMultiLastHostRoute": (C.c_int, [vp, C.c_int]),
        "NA_BatchAlgorithmicBytesPerSample": (C.c_double, [vp, C.c_int]),
        "NA_BatchMacsPerSample": (C.c_double, [vp]),
        "NA_BatchStateBytes": (C.c_double, [vp]),
        "NA_BatchStreamPackFactor": (C.c_int, [vp, C.c_int]),
        "NA_BatchStreamKernelName": (C.c_char_p, [vp, C.c_int]),
        "NA_DebugSetTraceBuffer": (None, [vp]),
        "NA_DebugSetWaveNetSpec": (None, [C.c_int]),
        "NA_DebugSetRcclApi": (None, [C.c_int, C.c_int, C.c_int]),
        "NA_DebugSetRecurrentQuadMin": (C.c_int, [C.c_int]),
        "NA_DebugRecurrentQuadLaunches": (C.c_longlong, []),
        "NA_RegisterHostBuffer": (C.c_int, [C.c_void_p, C.c_size_t]),
        "NA_UnregisterHostBuffer": (C.c_int, [C.c_void_p]),
        "NA_BatchStreamInputLimit": (C.c_float, [vp, C.c_int]),
        "NA_BatchRemoveStreams": (C.c_int, [vp, C.c_int, C.c_int]),
        "NA_BatchReserveStreams": (C.c_int, [vp, vp, C.c_int, C.c_int]),
        "NA_BatchActivateStream": (C.c_int, [vp, C.c_int, C.c_float]),
        "NA_BatchParkStream": (C.c_int, [vp, C.c_int]),
        "NA_BatchIsParked": (C.c_int, [vp, C.c_int]),
        "NA_BatchFindParked": (C.c_int, [vp, vp]),
        "NA_BatchNumParked": (C.c_int, [vp]),
        "NA_DebugDeviceResourceCalls": (C.c_longlong, []),
        "NA_BatchEnableOutputStage": (C.c_int, [vp]),
        "NA_BatchSetStreamGain": (C.c_int, [vp, C.c_int, C.c_float, C.c_int]),
        "NA_BatchGetStreamGain": (C.c_float, [vp, C.c_int]),
        "NA_BatchHandover": (C.c_int, [vp, C.c_int, C.c_int, C.c_float, C.c_int]),
        "NA_BatchHandoverRemaining": (C.c_int, [vp, C.c_int]),
        "NA_BatchEnableCabinetStage": (C.c_int, [vp, C.c_int]),
        "NA_BatchGetCabinetInfo": (C.c_int, [vp, C.POINTER(NA_CabinetInfo)]),
        "NA_BatchLoadIR": (C.c_int, [vp, fp, C.c_int]),
        "NA_BatchUnloadIR": (C.c_int, [vp, C.c_int]),
        "NA_BatchSetStreamIR": (C.c_int, [vp, C.c_int, C.c_int, C.c_int]),
        "NA_BatchGetStreamIR": (C.c_int, [vp, C.c_int]),
        "NA_BatchStreamIRFadeRemaining": (C.c_int, [vp, C.c_int]),
        "NA_DebugRunCabinetStage": (C.c_int, [vp, fp, C.c_long, C.c_size_t]),
        "NA_DebugCabinetLaunches": (C.c_longlong, []),
        "NA_BatchEnableReverbStage": (C.c_int, [vp, C.c_int]),
        "NA_BatchGetReverbInfo": (C.c_int, [vp, C.POINTER(NA_ReverbInfo)]),
        "NA_BatchLoadReverbIR": (C.c_int, [vp, fp, C.c_int]),
        "NA_BatchUnloadReverbIR": (C.c_int, [vp, C.c_int]),
        "NA_BatchSetStreamReverb": (C.c_int, [vp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int]),
        "NA_BatchGetStreamReverb": (C.c_int, [vp, C.c_int, fp, fp]),
        "NA_BatchStreamReverbFadeRemaining": (C.c_int, [vp, C.c_int]),
        "NA_DebugRunReverbStage": (C.c_int, [vp, fp, C.c_long, C.c_size_t]),
        "NA_DebugReverbLaunches": (C.c_longlong, []),
        "NA_DebugReverbTwiddles": (C.c_int, [fp, C.c_int]),
        "NA_DelayParamsFromMs": (C.c_int, [C.c_int] + [C.c_double] * 6 + [C.POINTER(NA_DelayParams)]),
        "NA_BatchEnableDelayStage": (C.c_int, [vp, C.c_int]),
        "NA_BatchGetDelayInfo": (C.c_int, [vp, C.POINTER(NA_DelayInfo)]),
        "NA_BatchSetStreamDelay": (C.c_int, [vp, C.c_int, C.POINTER(NA_DelayParams), C.c_int]),
        "NA_BatchGetStreamDelay": (C.c_int, [vp, C.c_int, C.POINTER(NA_DelayParams)]),
        "NA_BatchStreamDelayFadeRemaining": (C.c_int, [vp, C.c_int]),
        "NA_DebugRunDelayStage": (C.c_int, [vp, fp, C.c_long, C.c_size_t]),
        "NA_DebugDelayLaunches": (C.c_longlong, []),
        "NA_CompressorParamsFromDb": (C.c_int, [C.c_int] + [C.c_float] * 6 + [C.POINTER(NA_CompressorParams)]),
        "NA_BatchEnableCompressorStage": (C.c_int, [vp]),
        "NA_BatchGetCompressorInfo": (C.c_int, [vp, C.POINTER(NA_CompressorInfo)]),
        "NA_BatchSetStreamCompressor": (C.c_int, [vp, C.c_int, C.POINTER(NA_CompressorParams), C.c_int]),
        "NA_BatchGetStreamCompressor": (C.c_int, [vp, C.c_int, C.POINTER(NA_CompressorParams)]),
        "NA_BatchStreamCompressorFadeRemaining": (C.c_int, [vp, C.c_int]),
        "NA_BatchStreamCompressorGain": (C.c_float, [vp, C.c_int]),
        "NA_DebugRunCompressorStage": (C.c_int, [vp, fp, C.c_long, C.c_size_t]),
        "NA_DebugCompressorLaunches": (C.c_longlong, []),
        "NA_ModParamsFromMs": (C.c_int, [C.c_int] + [C.c_double] * 3 + [C.c_int] * 2 + [C.c_double] * 4 + [C.POINTER(NA_ModParams)]),
        "NA_BatchEnableModStage": (C.c_int, [vp, C.c_int]),
        "NA_BatchGetModInfo": (C.c_int, [vp, C.POINTER(NA_ModInfo)]),
        "NA_BatchSetStreamMod": (C.c_int, [vp, C.c_int, C.POINTER(NA_ModParams), C.c_int]),
        "NA_BatchGetStreamMod": (C.c_int, [vp, C.c_int, C.POINTER(NA_ModParams)]),
        "NA_BatchStreamModFadeRemaining": (C.c_int, [vp, C.c_int]),
        "NA_DebugRunModStage": (C.c_int, [vp, fp, C.c_long, C.c_size_t]),
        "NA_DebugModLaunches": (C.c_longlong, []),
        "NA_GateParamsFromDb": (C.c_int, [C.c_int] + [C.c_float] * 7 + [C.POINTER(NA_GateParams)]),
        "NA_BatchEnableGateStage": (C.c_int, [vp]),
        "NA_BatchGetGateInfo": (C.c_int, [vp, C.POINTER(NA_GateInfo)]),
        "NA_BatchSetStreamGate": (C.c_int, [vp, C.c_int, C.POINTER(NA_GateParams), C.c_int]),
        "NA_BatchGetStreamGate": (C.c_int, [vp, C.c_int, C.POINTER(NA_GateParams)]),
        "NA_BatchStreamGateGain": (C.c_float, [vp, C.c_int]),
        "NA_DebugGateLaunches": (C.c_longlong, []),
        "NA_BatchEnableMeterStage": (C.c_int, [vp]),
        "NA_BatchGetMeterInfo": (C.c_int, [vp, C.POINTER(NA_MeterInfo)]),
        "NA_BatchSetStreamMeter": (C.c_int, [vp, C.c_int, C.POINTER(NA_MeterParams)]),
        "NA_BatchGetStreamMeter": (C.c_int, [vp, C.c_int, C.POINTER(NA_MeterParams)]),
        "NA_BatchReadStreamMeter": (C.c_int, [vp, C.c_int, C.POINTER(NA_MeterReading)]),
        "NA_DebugMeterLaunches": (C.c_longlong, []),
        "NA_BatchEnableTunerStage": (C.c_int, [vp]),
        "NA_BatchGetTunerInfo": (C.c_int, [vp, C.POINTER(NA_TunerInfo)]),
        "NA_BatchSetStreamTuner": (C.c_int, [vp, C.c_int, C.POINTER(NA_TunerParams)]),
        "NA_BatchGetStreamTuner": (C.c_int, [vp, C.c_int, C.POINTER(NA_TunerParams)]),
        "NA_BatchReadStreamTuner": (C.c_int, [vp, C.c_int, C.POINTER(NA_TunerReading)]),
        "NA_TunerParamsFromRange": (C.c_int, [C.c_double] * 4 + [C.POINTER(NA_TunerParams)]),
        "NA_TunerPitch": (C.c_int, [C.POINTER(NA_TunerReading), C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "NA_DebugTunerLaunches": (C.c_longlong, []),
        "NA_BatchEnableMixStage": (C.c_int, [vp]),
        "NA_BatchGetMixInfo": (C.c_int, [vp, C.POINTER(NA_MixInfo)]),
        "NA_BatchSetMixGroup": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int]),
        "NA_BatchClearMixGroup": (C.c_int, [vp, C.c_int]),
        "NA_BatchGetStreamMix": (C.c_int, [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float)]),
        "NA_BatchMixRampRemaining": (C.c_int, [vp, C.c_int]),
        "NA_MixGainsFromPan": (C.c_int, [C.c_double, C.c_double, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
        "NA_DebugMixLaunches": (C.c_longlong, []),
        "NA_DebugMixStashLaunches": (C.c_longlong, []),
        "NA_DebugRunMixStage": (C.c_int, [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_long, C.c_size_t]),
        "NA_EqSectionFromDesign": (C.c_int, [C.c_int] + [C.c_double] * 4 + [C.POINTER(NA_EqSection)]),
        "NA_BatchEnableEqStage": (C.c_int, [vp]),
        "NA_BatchGetEqInfo": (C.c_int, [vp, C.POINTER(NA_EqInfo)]),
        "NA_BatchSetStreamEq": (C.c_int, [vp, C.c_int, C.POINTER(NA_EqSection), C.c_int, C.c_int]),
        "NA_BatchGetStreamEq": (C.c_int, [vp, C.c_int, C.POINTER(NA_EqSection), C.c_int]),
        "NA_BatchStreamEqFadeRemaining": (C.c_int, [vp, C.c_int]),
        "NA_DebugEqLaunches": (C.c_longlong, []),
        "NA_DebugRunEqStage": (C.c_int, [vp, fp, C.c_long, C.c_size_t]),
        "NA_DebugRecurrentPlan": (C.c_int, [vp, C.POINTER(C.c_int)]),
        "NA_DebugRecurrentShapePlan": (C.c_int, [C.c_int] * 8 + [C.POINTER(C.c_int)]),
        "NA_DebugRecurrentKernel": (C.c_int, [C.c_int] * 9 + [C.c_char_p, C.c_int]),
        "NA_DebugWaveNetKernel": (C.c_int, [vp, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), fp, C.c_char_p, C.c_int]),
        "NA_DebugWaveNetLaunch": (C.c_int, [C.c_int] * 3 + [C.POINTER(C.c_int)] + [C.c_int] * 4 + [C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "NA_MultiCreate": (vp, [C.POINTER(C.c_int), C.c_int]),
        "NA_MultiDestroy": (None, [vp]),
        "NA_MultiAddStreams": (C.c_int, [vp, vp, C.c_float, C.c_int, C.c_int]),
        "NA_MultiCommit": (C.c_int, [vp]),
        "NA_MultiNumStreams": (C.c_int, [vp]),
        "NA_MultiNumShards": (C.c_int, [vp]),
        "NA_MultiShardRange": (C.c_int, [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "NA_MultiProcess": (C.c_int, [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_size_t]),
        "NA_MultiSubmit": (C.c_int, [vp, C.POINTER(C.c_float), C.c_size_t]),
        "NA_MultiCollect": (C.c_int, [vp, C.c_int, C.POINTER(C.c_float)]),
        "NA_MultiSetQuality": (C.c_int, [vp, C.c_int, C.c_float]),
        "NA_ShardByCost": (C.c_int, [C.POINTER(C.c_double), C.c_int, C.c_int, C.POINTER(C.c_int)]),
        "NA_ModelStreamCost": (C.c_double, [vp, C.c_float]),
        "NA_BatchStreamRangeEvents": (C.c_int, [vp, C.c_int]),
        "NA_MultiSetFanIn": (C.c_int, [vp, C.c_int]),
        "NA_MultiGatheredOutput": (vp, [vp, C.c_int]),
        "NA_RcclAvailable": (C.c_int, []),
        "NA_ModelKernelInfo": (C.c_int, [vp, C.c_float, C.c_int, C.c_char_p, C.c_int, fp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "NA_BatchNumLiveStreams": (C.c_int, [vp]),
        "NA_BatchIsLive": (C.c_int, [vp, C.c_int]),
        "NA_SetWaveNetMathMode": (None, [vp, C.c_int]),
        "NA_SetLSTMMathMode": (None, [vp, C.c_int]),
        "NA_SetCompositeModelLoadMode": (None, [vp, C.c_int]),
        "NA_IsQualityChangeRealtimeSafe": (C.c_int, [vp, C.c_float]),
        "NA_ProcessChecked": (C.c_int, [vp, fp, fp, C.c_size_t]),
        "NA_BatchSubmit": (C.c_int, [vp, fp, C.c_size_t]),
        "NA_BatchCollect": (C.c_int, [vp, C.c_int, fp]),
        "NA_BatchNextInput": (fp, [vp, C.c_size_t]),
        "NA_BatchOutputView": (fp, [vp, C.c_int]),
        "NA_BatchIsQualityChangeRealtimeSafe": (C.c_int, [vp, C.c_int, C.c_float]),
        "NA_DebugClassifyNam": (C.c_int, [C.c_char_p]),
        "NA_DebugPackedWeights": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_int]),
        "NA_RenderOffline": (C.c_int, [C.POINTER(NA_RenderJob), C.c_int, C.POINTER(NA_RenderOptions)]),
        "NA_RenderPlan": (C.c_int, [C.POINTER(NA_RenderJob), C.c_int, C.POINTER(NA_RenderOptions), C.POINTER(NA_RenderPlanInfo)]),
        "NA_BatchStreamSnapshotBytes": (C.c_longlong, [vp, C.c_int]),
        "NA_ModelSnapshotBytes": (C.c_longlong, [vp]),
        "NA_ModelSnapshotFingerprint": (C.c_ulonglong, [vp]),
        "NA_BatchSaveStreams": (C.c_int, [vp, C.POINTER(C.c_int), C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
        "NA_BatchLoadStreams": (C.c_int, [vp, C.POINTER(C.c_int), C.c_int, vp, C.c_size_t]),
        "NA_SaveModelState": (C.c_int, [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]),
        "NA_LoadModelState": (C.c_int, [vp, vp, C.c_size_t]),
        "NA_DebugSnapshotLaunches": (C.c_longlong, []),
        "NA_ResamplePlan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(NA_ResampleInfo)]),
        "NA_ResamplePrototype": (C.c_int, [C.c_int, C.c_int, fp, C.c_int]),
        "NA_ResampleModelFrames": (C.c_longlong, [C.c_int, C.c_int, C.c_int, C.c_longlong]),
        "NA_BatchSetResampling": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int]),
        "NA_BatchGetResampleInfo": (C.c_int, [vp, C.POINTER(NA_ResampleInfo)]),
        "NA_SetResampleToExternalRate": (None, [vp, C.c_int]),
        "NA_GetProcessLatencySamples": (C.c_int, [vp]),
        "NA_GetModelProcessRate": (C.c_int, [vp]),
        "NA_DebugResampleTap": (C.c_int, [vp, fp, fp, C.c_longlong, C.POINTER(C.c_int)]),
        "NA_RenderOfflineAtRate": (C.c_int, [C.POINTER(NA_RenderJob), C.c_int, C.POINTER(NA_RenderOptions), C.c_int]),
        "NA_RenderPlanAtRate": (C.c_int, [C.POINTER(NA_RenderJob), C.c_int, C.POINTER(NA_RenderOptions), C.c_int, C.POINTER(NA_RenderPlanInfo),
                                          C.POINTER(NA_ResampleInfo)]),
        "NA_DebugSetRenderTap": (None, [fp, fp, C.c_longlong]),
        "NA_MultiSetResampling": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int]),
        "NA_MultiGetResampleInfo": (C.c_int, [vp, C.POINTER(NA_ResampleInfo)]),
        "NA_DebugSplitPlan": (C.c_int, [vp, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_ushort), C.c_longlong, C.POINTER(C.c_longlong)]),
    }
    for name, (res, args) in sig.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            # a tuning build from an older source tree (NA_LIB_SUFFIX: A/B benches against it) may lack the newest additive entry
            # points; the default library must have every one of them
            if os.environ.get("NA_LIB_SUFFIX") and name.startswith("NA_"):
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error():
    return load_library().NA_GetLastError().decode("utf-8", "replace")


def device_count():
    return int(load_library().NA_GetDeviceCount())
