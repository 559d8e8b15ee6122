// capi.cpp -- extern "C" surface of libNeuralAudioCAPI.so: the 15 legacy symbols of the reference's
// NeuralAudioCAPI (NeuralAudioCAPI/NeuralAudioCApi.cpp:4-97) plus the additive NA_* batch API
// (include/neuralaudio_amd.h).  No exception crosses this boundary.
#include <cstring>
#include <cwchar>
#include <string>

#include "neuralaudio_amd.h"
#include "multi_gpu.h"
#include "offline_render.h"
#include "resample.h"
#include "stream_snapshot.h"
#include "neural_model_impl.h"
#include "lstm_launch.h"
#include "wavenet_choice.h"
#include "wavenet_launch.h"
#include "wavenet_plan.h"
#include "tuning.h"

struct NeuralModel
{
	NeuralAudio::NeuralModel* model;
};

struct NeuralModelLoader
{
	NeuralAudio::NeuralModelLoader* loader;
};

struct NA_Batch
{
	na::GpuBatch* batch;
};

struct NA_MultiBatch
{
	na::MultiGpuBatch* multi;
};

namespace
{
	thread_local std::string g_lastError;

	void SetError(const char* what) { g_lastError = what ? what : "unknown error"; }

	template <typename F>
	int Guard(F&& f)
	{
		try
		{
			f();
			return 0;
		}
		catch (const std::exception& e)
		{
			SetError(e.what());
		}
		catch (...)
		{
			SetError("unknown exception");
		}
		return -1;
	}

	// An NA_Batch* entry point: `f` runs on the batch under Guard; a null batch is an error with the entry point's name in front
	template <typename F>
	int BatchCall(NA_Batch* batch, const char* who, F&& f)
	{
		return Guard([&] {
			if (!batch) throw std::runtime_error(std::string(who) + ": null batch (NA_BatchCreate fails where no HIP device is visible: there is no CPU fallback)");
			f(*batch->batch);
		});
	}

	// ... one that returns what `f` returns, or `failed` (the value the header documents for an error)
	template <typename T, typename F>
	T BatchValue(NA_Batch* batch, const char* who, T failed, F&& f)
	{
		T value = failed;
		return BatchCall(batch, who, [&](na::GpuBatch& b) { value = f(b); }) == 0 ? value : failed;
	}

	// wchar_t is UTF-32 on Linux and UTF-16 on Windows (the C# caller marshals LPWStr, NativeApi.cs:17)
	std::string WideToUtf8(const wchar_t* w)
	{
		std::string out;
		if (!w) return out;
		for (; *w; ++w)
		{
			unsigned long cp = (unsigned long)*w;
			if (sizeof(wchar_t) == 2 && cp >= 0xD800 && cp <= 0xDBFF && w[1] >= 0xDC00 && w[1] <= 0xDFFF)
			{
				cp = 0x10000 + ((cp - 0xD800) << 10) + ((unsigned long)w[1] - 0xDC00);
				++w;
			}
			if (cp < 0x80) out.push_back((char)cp);
			else if (cp < 0x800)
			{
				out.push_back((char)(0xC0 | (cp >> 6)));
				out.push_back((char)(0x80 | (cp & 0x3F)));
			}
			else if (cp < 0x10000)
			{
				out.push_back((char)(0xE0 | (cp >> 12)));
				out.push_back((char)(0x80 | ((cp >> 6) & 0x3F)));
				out.push_back((char)(0x80 | (cp & 0x3F)));
			}
			else
			{
				out.push_back((char)(0xF0 | (cp >> 18)));
				out.push_back((char)(0x80 | ((cp >> 12) & 0x3F)));
				out.push_back((char)(0x80 | ((cp >> 6) & 0x3F)));
				out.push_back((char)(0x80 | (cp & 0x3F)));
			}
		}
		return out;
	}

	NeuralModel* Wrap(NeuralAudio::NeuralModel* m)
	{
		if (!m) return nullptr;
		NeuralModel* w = new NeuralModel();
		w->model = m;
		return w;
	}

	int CopyOut(const std::string& s, char* buf, int bufSize)
	{
		if (buf && bufSize > 0)
		{
			const size_t n = std::min((size_t)bufSize - 1, s.size());
			memcpy(buf, s.data(), n);
			buf[n] = 0;
		}
		return (int)s.size();
	}
}

extern "C" {

// ---------------------------------------------------------------- legacy symbols (reference NeuralAudioCApi.h:18-46)

NeuralModelLoader* CreateLoader(void)
{
	NeuralModelLoader* loader = nullptr;
	Guard([&] {
		loader = new NeuralModelLoader();
		loader->loader = new NeuralAudio::NeuralModelLoader();
	});
	return loader;
}

void DeleteLoader(NeuralModelLoader* loader)
{
	if (!loader) return;
	delete loader->loader;
	delete loader;
}

NeuralModel* CreateModelFromFile(NeuralModelLoader* loader, const wchar_t* modelPath)
{
	NeuralModel* result = nullptr;
	Guard([&] {
		if (!loader || !modelPath) throw std::runtime_error("CreateModelFromFile: null argument");
		NeuralAudio::NeuralModel* m = loader->loader->CreateFromFile(std::filesystem::path(WideToUtf8(modelPath)));
		if (!m) SetError("model file not found or not supported");
		result = Wrap(m);
	});
	return result;
}

void DeleteModel(NeuralModel* model)
{
	if (!model) return;
	delete model->model;
	delete model;
}

void SetLSTMLoadMode(NeuralModelLoader* loader, int loadMode)
{
	if (loader) loader->loader->SetLSTMLoadMode((NeuralAudio::EModelLoadMode)loadMode);
}

void SetWaveNetLoadMode(NeuralModelLoader* loader, int loadMode)
{
	if (loader) loader->loader->SetWaveNetLoadMode((NeuralAudio::EModelLoadMode)loadMode);
}

void SetAudioInputLevelDBu(NeuralModelLoader* loader, float audioDBu)
{
	if (loader) loader->loader->SetAudioInputLevelDBu(audioDBu);
}

void SetDefaultMaxAudioBufferSize(NeuralModelLoader* loader, int maxSize)
{
	if (loader) loader->loader->SetDefaultMaxAudioBufferSize(maxSize);
}

int GetLoadMode(NeuralModel* model) { return model ? (int)model->model->GetLoadMode() : 0; }

bool IsStatic(NeuralModel* model) { return model ? model->model->IsStatic() : false; }

void SetMaxAudioBufferSize(NeuralModel* model, int maxSize)
{
	if (model) model->model->SetMaxAudioBufferSize(maxSize);
}

float GetRecommendedInputDBAdjustment(NeuralModel* model) { return model ? model->model->GetRecommendedInputDBAdjustment() : 0.0f; }

float GetRecommendedOutputDBAdjustment(NeuralModel* model) { return model ? model->model->GetRecommendedOutputDBAdjustment() : 0.0f; }

float GetSampleRate(NeuralModel* model) { return model ? model->model->GetSampleRate() : 0.0f; }

void Process(NeuralModel* model, float* input, float* output, size_t numSamples)
{
	(void)NA_ProcessChecked(model, input, output, numSamples);
}

// ---------------------------------------------------------------- additive API (include/neuralaudio_amd.h)

const char* NA_GetLastError(void) { return g_lastError.c_str(); }

int NA_GetDeviceCount(void) { return na::VisibleDeviceCount(); }

const char* NA_GetVersion(void) { return "neuralaudio_amd 0.1.0 (gfx950)"; }

NeuralModel* NA_CreateModelFromFileUtf8(NeuralModelLoader* loader, const char* utf8Path, int doPrewarm)
{
	NeuralModel* result = nullptr;
	Guard([&] {
		if (!loader || !utf8Path) throw std::runtime_error("NA_CreateModelFromFileUtf8: null argument");
		NeuralAudio::NeuralModel* m = loader->loader->CreateFromFile(std::filesystem::path(std::string(utf8Path)), doPrewarm != 0);
		if (!m) SetError("model file not found or not supported");
		result = Wrap(m);
	});
	return result;
}

NeuralModel* NA_CreateModelFromString(NeuralModelLoader* loader, const char* jsonText, const char* extension, int doPrewarm)
{
	NeuralModel* result = nullptr;
	Guard([&] {
		if (!loader || !jsonText || !extension) throw std::runtime_error("NA_CreateModelFromString: null argument");
		NeuralAudio::NeuralModel* m = loader->loader->CreateFromString(jsonText, std::filesystem::path(std::string(extension)), doPrewarm != 0);
		if (!m) SetError("model not supported");
		result = Wrap(m);
	});
	return result;
}

// The legacy Process() cannot report failure; an audio host must never be handed uninitialised memory, so a failed call
// (no device, HIP error) returns silence and leaves the reason in NA_GetLastError().
int NA_ProcessChecked(NeuralModel* model, float* input, float* output, size_t numSamples)
{
	if (!model || !output)
	{
		SetError("Process: null argument");
		return -1;
	}
	const int rc = Guard([&] { model->model->Process(input, output, numSamples); });
	if (rc != 0) memset(output, 0, numSamples * sizeof(float));
	return rc;
}

void NA_SetWaveNetMathMode(NeuralModelLoader* loader, int mathMode)
{
	if (loader) loader->loader->SetWaveNetMathMode(mathMode == 1 ? NeuralAudio::EMathMode::StdMath : NeuralAudio::EMathMode::FastMath);
}

void NA_SetLSTMMathMode(NeuralModelLoader* loader, int mathMode)
{
	if (loader) loader->loader->SetLSTMMathMode(mathMode == 1 ? NeuralAudio::EMathMode::StdMath : NeuralAudio::EMathMode::FastMath);
}

void NA_SetCompositeModelLoadMode(NeuralModelLoader* loader, int loadMode)
{
	if (loader) loader->loader->SetCompositeModelLoadMode(loadMode == 1 ? NeuralAudio::ECompositeModelLoadMode::OnDemand : NeuralAudio::ECompositeModelLoadMode::LoadAll);
}

int NA_IsQualityChangeRealtimeSafe(NeuralModel* model, float newQuality)
{
	return (model && model->model->IsQualityChangeRealtimeSafe(newQuality)) ? 1 : 0;
}

// bit 0: NAMIsA2(version), bit 1: NAMIsA2Standard(model) -- the reference's engine-selection predicates, exposed for tests
#ifndef NA_RELEASE
int NA_DebugClassifyNam(const char* jsonText)
{
	int r = -1;
	Guard([&] {
		const na::Json j = na::Json::Parse(jsonText ? jsonText : "");
		const std::string v = (j.IsObject() && j.Contains("version") && j.At("version").IsString()) ? j.At("version").AsString() : "";
		r = (na::NAMIsA2(v) ? 1 : 0) | (na::NAMIsA2Standard(j) ? 2 : 0);
	});
	return r;
}
#endif

// Stream packing, host side only (no GPU needed; tests): the pack factor the model would run with in a large batch (1: none) and, when
// `out` is given, the flat weights of the packed virtual model (wavenet_plan.cpp PackWaveNetDesc); returns their count, -1 on failure.
#ifndef NA_RELEASE
int NA_DebugPackedWeights(NeuralModel* model, int* packFactor, float* out, int capacity)
{
	int r = -1;
	Guard([&] {
		NeuralAudio::GpuModel* gm = model ? dynamic_cast<NeuralAudio::GpuModel*>(model->model) : nullptr;
		if (!gm) throw std::runtime_error("NA_DebugPackedWeights: not a model of this library");
		const auto& lm = gm->GetLoadedModel();
		if (lm->subModels.size() != 1 || lm->subModels[0].desc->kind != na::MODEL_WAVENET)
		{
			if (packFactor) *packFactor = 1;
			r = 0;
			return;
		}
		const na::WaveNetDesc& wn = lm->subModels[0].desc->wavenet;
		const int P = na::WaveNetPackFactor(wn);
		if (packFactor) *packFactor = P;
		if (P < 2)
		{
			r = 0;
			return;
		}
		const bool dense = na::WaveNetDenseFor(wn, P, na::WaveNetKnobs::FromTuning()); // (the layout a batch would give it: four Nano streams at 16 / 8 channels)
		const na::WaveNetDesc v = na::PackWaveNetDesc(wn, P, dense);
		na::ValidateWaveNetDesc(v); // weight count and chaining of the virtual model
		const na::WaveNetPlan plan = na::BuildPackedWaveNetPlan(wn, P, dense);
		if (plan.pack != P || plan.splitFastT != 2) throw std::runtime_error("NA_DebugPackedWeights: the packed plan is not a fast split-kernel plan");
		r = (int)v.weights.size();
		if (out)
			for (int i = 0; i < r && i < capacity; i++) out[i] = v.weights[(size_t)i];
	});
	return r;
}
#endif

// The f16-split plan of a WaveNet model as an unpacked batch stream would run it (wavenet_plan.cpp BuildSplit), host side only: 16 ints
// per stage into stages[stageCapacity] (WnSplitStage), the A-operand image (f16 bit patterns, 512 per operand) into wsplit[wsplitCapacity];
// returns the stage count, -1 on failure.
#ifndef NA_RELEASE
int NA_DebugSplitPlan(NeuralModel* model, int* stages, int stageCapacity, unsigned short* wsplit, long long wsplitCapacity, long long* wsplitCount)
{
	int r = -1;
	Guard([&] {
		NeuralAudio::GpuModel* gm = model ? dynamic_cast<NeuralAudio::GpuModel*>(model->model) : nullptr;
		if (!gm) throw std::runtime_error("NA_DebugSplitPlan: not a model of this library");
		const auto& lm = gm->GetLoadedModel();
		if (lm->subModels.size() != 1 || lm->subModels[0].desc->kind != na::MODEL_WAVENET) throw std::runtime_error("NA_DebugSplitPlan: not a WaveNet");
		const na::WaveNetPlan plan = na::BuildWaveNetPlan(lm->subModels[0].desc->wavenet, true);
		static_assert(sizeof(na::WnSplitStage) == 16 * sizeof(int), "16 ints per stage");
		r = (int)plan.sstages.size();
		if (stages) memcpy(stages, plan.sstages.data(), sizeof(na::WnSplitStage) * (size_t)std::min(r, stageCapacity));
		if (wsplitCount) *wsplitCount = (long long)plan.wsplit.size();
		if (wsplit) memcpy(wsplit, plan.wsplit.data(), sizeof(uint16_t) * (size_t)std::min<long long>((long long)plan.wsplit.size(), wsplitCapacity));
	});
	return r;
}
#endif

// The same plan for a shape alone (cell: 0 LSTM, 1 GRU; tail*: the dense / conv1d chain of a keras stack, zeros for the classic head), with
// rpl > 0 / forceL2w >= 0 in place of the tuning knobs NA_REC_RPL / NA_REC_L2W.  Returns 1 if the loader's shape predicate for this
// kernel admits the shape (lstm_dev.h RecurrentWaveShape), 0 if not, -1 on a bad argument.
#ifndef NA_RELEASE
int NA_DebugRecurrentShapePlan(int cell, int hidden, int numLayers, int tailLayers, int tailWidth, int tailHistory, int rpl, int forceL2w, int out[6])
{
	if (!out || (cell != 0 && cell != 1) || hidden < 1 || numLayers < 0 || tailLayers < 0) return -1;
	const na::RecurrentPlan p = na::RecurrentWavePlan(cell == 1 ? na::LSTM_CELL_GRU : na::LSTM_CELL_LSTM, hidden, numLayers, tailLayers, tailWidth, tailHistory, true, rpl, forceL2w);
	out[0] = p.runs; out[1] = p.waves; out[2] = p.rowsPerLane; out[3] = p.l2w; out[4] = p.headInLoop; out[5] = (int)p.ldsBytes;
	return na::RecurrentWaveShape(hidden, numLayers, tailLayers > 0 ? tailWidth : 0, tailLayers > 0 ? tailHistory : 0) ? 1 : 0;
}
#endif

// Which kernel runs a recurrent model of this shape (lstm_dev.h RecurrentKernelFor -- what a model group asks once and its launches obey),
// host side only.  knobMask: bit 0 NA_LSTM_NO_DPP, 1 NA_GRU_NO_DPP, 2 NA_LSTM_LANE_KERNEL, 3 NA_LSTM_NO_WAVE_RT, 4 NA_REC_NO_DPP32, 5 NA_REC_L2W; rpl:
// NA_REC_RPL (0: one row per lane) -- the environment is not read.  knobMask -1: the process's own tuning knobs (rpl is ignored).  Returns
// the RecurrentKernel value (0: no kernel takes the shape) and writes the kernel's name, -1 on a bad argument.
#ifndef NA_RELEASE
int NA_DebugRecurrentKernel(int cell, int hidden, int numLayers, int tailLayers, int tailWidth, int tailHistory, int haveWT, int knobMask, int rpl, char* outName, int cap)
{
	if ((cell != 0 && cell != 1) || hidden < 1 || numLayers < 0 || tailLayers < 0 || knobMask < -1 || knobMask > 63) return -1;
	const int b = knobMask;
	const na::RecurrentKnobs k = b < 0 ? na::RecurrentKnobs::FromTuning()
		: na::RecurrentKnobs{ (b & 1) != 0, (b & 2) != 0, (b & 4) != 0, (b & 8) != 0, (b & 16) != 0, rpl > 0 ? rpl : 1, (b & 32) != 0 };
	const na::RecurrentKernel kernel = na::RecurrentKernelFor(cell == 1 ? na::LSTM_CELL_GRU : na::LSTM_CELL_LSTM, hidden, numLayers, tailLayers, tailWidth, tailHistory,
		haveWT != 0, k).kernel;
	if (outName && cap > 0) snprintf(outName, (size_t)cap, "%s", na::RecurrentKernelName(kernel));
	return (int)kernel;
}
#endif

// The WaveNet counterparts (wavenet_choice.h), host side only; the environment is not read.  Knobs: bit i of knobMask set = knob i takes
// knobs[i], every other knob its default; knobMask -1 = the process's own tuning knobs.  Knob order: NA_WN_KERNEL (1 split, 2 frame,
// 3 generic), NA_WN_PACK, NA_WN_PAD off, NA_WN_DENSE, NA_SP_T, NA_SP_SPB, NA_SP_GEN, NA_SP_NO_T1, NA_FR_PF, NA_FR_SPB, chains on (NA_WN_SPEC).
#ifndef NA_RELEASE
static bool DebugWaveNetKnobs(int knobMask, const int* v, na::WaveNetKnobs& k)
{
	if (knobMask == -1)
	{
		k = na::WaveNetKnobs::FromTuning();
		return true;
	}
	if (knobMask < 0 || knobMask >= (1 << 11) || (knobMask != 0 && !v)) return false;
	auto has = [&](int i) { return (knobMask >> i & 1) != 0; };
	if (has(0)) k.wnKernel = v[0];
	if (has(1)) k.wnPack = v[1];
	if (has(2)) k.wnPadOff = v[2] != 0;
	if (has(3)) k.wnDense = v[3];
	if (has(4)) k.spT = v[4];
	if (has(5)) k.spSpb = v[5];
	if (has(6)) k.spGen = v[6] != 0;
	if (has(7)) k.spNoT1 = v[7] != 0;
	if (has(8)) k.frPrefetch = v[8];
	if (has(9)) k.frSpb = v[9];
	if (has(10)) k.specOn = v[10] != 0;
	return true;
}

// What a batch's model group would decide for `streams` streams of the model at `quality` (WaveNetKernelFor): out = { family (1 f16-split,
// 2 frame, 3 generic), pack, dense, packed or padded, specialised chain (WnSpecArch), LaunchKind, range proven, weights ok }, the input
// limit and the reported kernel name; 0, or -1 on a bad argument or a model that is not a WaveNet.
int NA_DebugWaveNetKernel(NeuralModel* model, float quality, int streams, int knobMask, const int* knobs, int out[8], float* inputLimit, char* outName, int cap)
{
	int r = -1;
	Guard([&] {
		NeuralAudio::GpuModel* gm = model ? dynamic_cast<NeuralAudio::GpuModel*>(model->model) : nullptr;
		na::WaveNetKnobs k;
		if (!gm || !out || !DebugWaveNetKnobs(knobMask, knobs, k)) throw std::runtime_error("NA_DebugWaveNetKernel: bad argument");
		const auto& lm = gm->GetLoadedModel();
		if (lm->subModels.empty()) throw std::runtime_error("NA_DebugWaveNetKernel: empty model");
		const na::ModelDesc& d = *lm->subModels[(size_t)(lm->isComposite ? lm->ModelIndexFromQuality(quality) : 0)].desc;
		if (d.kind != na::MODEL_WAVENET) throw std::runtime_error("NA_DebugWaveNetKernel: not a WaveNet");
		const na::WaveNetGroupChoice c = na::WaveNetKernelFor(d.wavenet, (!lm->isComposite && lm->subModels.size() == 1) ? streams : 0, k);
		const int ints[8] = { (int)c.family, c.pack, c.dense, c.isVirtual, c.specArch, (int)c.kind, c.rangeProven, c.weightsOk };
		memcpy(out, ints, sizeof(ints));
		if (inputLimit) *inputLimit = c.inputLimit;
		if (outName && cap > 0) snprintf(outName, (size_t)cap, "%s", c.KernelName(k.specOn));
		r = 0;
	});
	return r;
}

// What one launch decides (WaveNetLaunchFor).  groupFacts: 8 ints per group = { specialised chain, pack, split_fast_T, streams, index lists
// present, max_a4_floats, max_G, max_split_ops }.  out = { kernel (WnLaunchKernel: 0 none, 1 chain, 2 chain table, 3 interpreter, 4 frame,
// 5 cut the list into launches of eight), error of a refusal, chain family member (WnChain), NF, SPB, NT, T, WPS, GEN, PK, PF }; 0, -1 on a bad argument.
int NA_DebugWaveNetLaunch(int frame, int n, int numGroups, const int* groupFacts, int sharing, int beyondCache, int cus, int knobMask, const int* knobs, int out[11])
{
	int r = -1;
	Guard([&] {
		na::WaveNetKnobs k;
		if (!out || numGroups < 0 || (numGroups > 0 && !groupFacts) || !DebugWaveNetKnobs(knobMask, knobs, k)) throw std::runtime_error("NA_DebugWaveNetLaunch: bad argument");
		std::vector<na::WaveNetGroupFacts> facts((size_t)numGroups);
		for (int i = 0; i < numGroups; i++)
		{
			const int* g = groupFacts + 8 * i;
			facts[(size_t)i] = { g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7] };
		}
		const na::WaveNetLaunchChoice c = na::WaveNetLaunchFor({ frame != 0, n, facts.data(), numGroups, sharing, beyondCache != 0, cus }, k);
		const int ints[11] = { (int)c.kernel, c.error, (int)c.chain, c.nf, c.spb, c.nt, c.t, c.wps, c.gen, c.pk, c.pf };
		memcpy(out, ints, sizeof(ints));
		r = 0;
	});
	return r;
}
#endif

// The runtime-shaped recurrent kernel's plan for a recurrent model (lstm_dev.h RecurrentPlan -- what the launcher reads), host side
// only: out = { runs on RecurrentWaveRtKernel, waves per stream, gate rows per lane, weights streamed from L2, head inside the sample
// loop, dynamic LDS bytes }; 0, or -1 when the model is not a single recurrent one.
#ifndef NA_RELEASE
int NA_DebugRecurrentPlan(NeuralModel* model, int out[6])
{
	int r = -1;
	Guard([&] {
		NeuralAudio::GpuModel* gm = model ? dynamic_cast<NeuralAudio::GpuModel*>(model->model) : nullptr;
		if (!gm || !out) throw std::runtime_error("NA_DebugRecurrentPlan: not a model of this library");
		const auto& lm = gm->GetLoadedModel();
		if (lm->subModels.size() != 1 || lm->subModels[0].desc->kind != na::MODEL_LSTM) throw std::runtime_error("NA_DebugRecurrentPlan: not a recurrent model");
		const na::LSTMDesc& d = lm->subModels[0].desc->lstm;
		int tailWidth = 0, tailHistory = 0;
		na::RecurrentTailDims(d, tailWidth, tailHistory);
		const na::RecurrentPlan p = na::RecurrentWavePlan(d.cell == na::CELL_GRU ? na::LSTM_CELL_GRU : na::LSTM_CELL_LSTM, d.hiddenSize, d.numLayers, (int)d.tail.size(),
			tailWidth, tailHistory);
		out[0] = p.runs; out[1] = p.waves; out[2] = p.rowsPerLane; out[3] = p.l2w; out[4] = p.headInLoop; out[5] = (int)p.ldsBytes;
		r = 0;
	});
	return r;
}
#endif

void NA_SetDevice(NeuralModelLoader* loader, int device)
{
	if (loader) loader->loader->SetDevice(device);
}

void NA_SetDefaultQualityScaleFactor(NeuralModelLoader* loader, float quality)
{
	if (loader) loader->loader->SetDefaultQualityScaleFactor(quality);
}

void NA_SetExternalSampleRate(NeuralModelLoader* loader, int sampleRate)
{
	if (loader) loader->loader->SetExternalSampleRate(sampleRate);
}

int NA_HasQualityScaling(NeuralModel* model) { return (model && model->model->HasQualityScaling()) ? 1 : 0; }

float NA_GetQualityScaleFactor(NeuralModel* model) { return model ? model->model->GetQualityScaleFactor() : 1.0f; }

void NA_SetQualityScaleFactor(NeuralModel* model, float quality)
{
	if (model) Guard([&] { model->model->SetQualityScaleFactor(quality); });
}

int NA_GetReceptiveFieldSize(NeuralModel* model) { return model ? model->model->GetReceptiveFieldSize() : -1; }

int NA_Prewarm(NeuralModel* model)
{
	if (!model) return -1;
	return Guard([&] { model->model->Prewarm(); });
}

int NA_GetMetadata(NeuralModel* model, const char* fieldName, char* buf, int bufSize)
{
	if (!model || !fieldName) return -1;
	return CopyOut(model->model->GetMetadata(fieldName), buf, bufSize);
}

int NA_GetModelVersion(NeuralModel* model, char* buf, int bufSize)
{
	if (!model) return -1;
	return CopyOut(model->model->GetModelVersion(), buf, bufSize);
}

NA_Batch* NA_BatchCreate(int device, void* hipStream)
{
	NA_Batch* b = nullptr;
	Guard([&] {
		na::GpuBatch* gb = new na::GpuBatch(device, reinterpret_cast<hipStream_t>(hipStream));
		b = new NA_Batch();
		b->batch = gb;
	});
	return b;
}

void NA_BatchDestroy(NA_Batch* batch)
{
	if (!batch) return;
	Guard([&] { delete batch->batch; });
	delete batch;
}

int NA_BatchAddStreams(NA_Batch* batch, NeuralModel* model, float quality, int count, int doPrewarm)
{
	int first = -1;
	const int rc = Guard([&] {
		if (!batch || !model || count < 1) throw std::runtime_error("NA_BatchAddStreams: bad argument");
		NeuralAudio::GpuModel* gm = dynamic_cast<NeuralAudio::GpuModel*>(model->model);
		if (!gm) throw std::runtime_error("NA_BatchAddStreams: model was not created by this library");
		first = batch->batch->AddStreams(gm->GetLoadedModel(), quality, count, doPrewarm != 0, gm->IsOnDemand());
	});
	return rc == 0 ? first : -1;
}

// ---- the stream pool (gpu_batch.h ReserveStreams / ActivateStream / ParkStream) ----
int NA_BatchReserveStreams(NA_Batch* batch, NeuralModel* model, int count, int doPrewarm)
{
	return BatchValue(batch, "NA_BatchReserveStreams", -1, [&](na::GpuBatch& b) {
		if (!model || count < 1) throw std::runtime_error("NA_BatchReserveStreams: bad argument");
		NeuralAudio::GpuModel* gm = dynamic_cast<NeuralAudio::GpuModel*>(model->model);
		if (!gm) throw std::runtime_error("NA_BatchReserveStreams: model was not created by this library");
		return b.ReserveStreams(gm->GetLoadedModel(), count, doPrewarm != 0);
	});
}

int NA_BatchActivateStream(NA_Batch* batch, int stream, float quality)
{
	return BatchCall(batch, "NA_BatchActivateStream", [&](na::GpuBatch& b) { b.ActivateStream(stream, quality); });
}

int NA_BatchParkStream(NA_Batch* batch, int stream)
{
	return BatchCall(batch, "NA_BatchParkStream", [&](na::GpuBatch& b) { b.ParkStream(stream); });
}

int NA_BatchIsParked(NA_Batch* batch, int stream) { return (batch && batch->batch->IsParked(stream)) ? 1 : 0; }

int NA_BatchFindParked(NA_Batch* batch, NeuralModel* model)
{
	NeuralAudio::GpuModel* gm = (batch && model) ? dynamic_cast<NeuralAudio::GpuModel*>(model->model) : nullptr;
	return gm ? batch->batch->FindParked(gm->GetLoadedModel().get()) : -1;
}

int NA_BatchNumParked(NA_Batch* batch) { return batch ? batch->batch->NumParked() : -1; }

// ---- the output stage (gpu_batch.h EnableOutputStage / SetStreamGain / Handover) ----
int NA_BatchEnableOutputStage(NA_Batch* batch)
{
	return BatchCall(batch, "NA_BatchEnableOutputStage", [&](na::GpuBatch& b) { b.EnableOutputStage(); });
}

int NA_BatchSetStreamGain(NA_Batch* batch, int stream, float gain, int rampSamples)
{
	return BatchCall(batch, "NA_BatchSetStreamGain", [&](na::GpuBatch& b) { b.SetStreamGain(stream, gain, rampSamples); });
}

float NA_BatchGetStreamGain(NA_Batch* batch, int stream)
{
	return BatchValue(batch, "NA_BatchGetStreamGain", -1.0f, [&](na::GpuBatch& b) { return b.GetStreamGain(stream); });
}

int NA_BatchHandover(NA_Batch* batch, int from, int to, float quality, int fadeSamples)
{
	return BatchCall(batch, "NA_BatchHandover", [&](na::GpuBatch& b) { b.Handover(from, to, quality, fadeSamples); });
}

int NA_BatchHandoverRemaining(NA_Batch* batch, int stream)
{
	return BatchValue(batch, "NA_BatchHandoverRemaining", -1, [&](na::GpuBatch& b) { return b.HandoverRemaining(stream); });
}

// ---- the cabinet stage (gpu_batch.h EnableCabinetStage / LoadIR / SetStreamIR) ----
int NA_BatchEnableCabinetStage(NA_Batch* batch, int maxTaps)
{
	return BatchCall(batch, "NA_BatchEnableCabinetStage", [&](na::GpuBatch& b) { b.EnableCabinetStage(maxTaps); });
}

int NA_BatchGetCabinetInfo(NA_Batch* batch, NA_CabinetInfo* info)
{
	return BatchCall(batch, "NA_BatchGetCabinetInfo", [&](na::GpuBatch& b) {
		if (!info) throw std::runtime_error("NA_BatchGetCabinetInfo: bad argument");
		const na::CabinetStageInfo i = b.GetCabinetInfo();
		info->maxTaps = i.maxTaps;
		info->ringSamples = i.ringSamples;
		info->pieceSamples = i.pieceSamples;
		info->numIRs = i.numIRs;
		info->deviceBytes = i.deviceBytes;
	});
}

int NA_BatchLoadIR(NA_Batch* batch, const float* taps, int numTaps)
{
	return BatchValue(batch, "NA_BatchLoadIR", -1, [&](na::GpuBatch& b) { return b.LoadIR(taps, numTaps); });
}

int NA_BatchUnloadIR(NA_Batch* batch, int ir)
{
	return BatchCall(batch, "NA_BatchUnloadIR", [&](na::GpuBatch& b) { b.UnloadIR(ir); });
}

int NA_BatchSetStreamIR(NA_Batch* batch, int stream, int ir, int fadeSamples)
{
	return BatchCall(batch, "NA_BatchSetStreamIR", [&](na::GpuBatch& b) { b.SetStreamIR(stream, ir, fadeSamples); });
}

int NA_BatchGetStreamIR(NA_Batch* batch, int stream)
{
	return BatchValue(batch, "NA_BatchGetStreamIR", -2, [&](na::GpuBatch& b) { return b.GetStreamIR(stream); });
}

int NA_BatchStreamIRFadeRemaining(NA_Batch* batch, int stream)
{
	return BatchValue(batch, "NA_BatchStreamIRFadeRemaining", -1, [&](na::GpuBatch& b) { return b.StreamIRFadeRemaining(stream); });
}

#ifndef NA_RELEASE
int NA_DebugRunCabinetStage(NA_Batch* batch, float* hostRows, long stride, size_t n)
{
	return Guard([&] {
		if (!batch) throw std::runtime_error("NA_DebugRunCabinetStage: null batch");
		batch->batch->DebugRunCabinetStage(hostRows, stride, n);
	});
}
long long NA_DebugCabinetLaunches(void) { return (long long)na::CabinetStageLaunches(); }
#endif

// ---- the reverb stage (gpu_batch.h EnableReverbStage / LoadReverbIR / SetStreamReverb) ----
int NA_BatchEnableReverbStage(NA_Batch* batch, int maxTaps)
{
	return BatchCall(batch, "NA_BatchEnableReverbStage", [&](na::GpuBatch& b) { b.EnableReverbStage(maxTaps); });
}

int NA_BatchGetReverbInfo(NA_Batch* batch, NA_ReverbInfo* info)
{
	return BatchCall(batch, "NA_BatchGetReverbInfo", [&](na::GpuBatch& b) {
		if (!info) throw std::runtime_error("NA_BatchGetReverbInfo: bad argument");
		const na::ReverbStageInfo i = b.GetReverbInfo();
		info->maxTaps = i.maxTaps;
		info->partitionSamples = i.partitionSamples;
		info->slots = i.slots;
		info->pieceSamples = i.pieceSamples;
		info->numIRs = i.numIRs;
		info->deviceBytes = i.deviceBytes;
	});
}

int NA_BatchLoadReverbIR(NA_Batch* batch, const float* taps, int numTaps)
{
	return BatchValue(batch, "NA_BatchLoadReverbIR", -1, [&](na::GpuBatch& b) { return b.LoadReverbIR(taps, numTaps); });
}

int NA_BatchUnloadReverbIR(NA_Batch* batch, int ir)
{
	return BatchCall(batch, "NA_BatchUnloadReverbIR", [&](na::GpuBatch& b) { b.UnloadReverbIR(ir); });
}

int NA_BatchSetStreamReverb(NA_Batch* batch, int stream, int ir, float wet, float dry, int fadeSamples)
{
	return BatchCall(batch, "NA_BatchSetStreamReverb", [&](na::GpuBatch& b) { b.SetStreamReverb(stream, ir, wet, dry, fadeSamples); });
}

int NA_BatchGetStreamReverb(NA_Batch* batch, int stream, float* wet, float* dry)
{
	return BatchValue(batch, "NA_BatchGetStreamReverb", -2, [&](na::GpuBatch& b) { return b.GetStreamReverb(stream, wet, dry); });
}

int NA_BatchStreamReverbFadeRemaining(NA_Batch* batch, int stream)
{
	return BatchValue(batch, "NA_BatchStreamReverbFadeRemaining", -1, [&](na::GpuBatch& b) { return b.StreamReverbFadeRemaining(stream); });
}

#ifndef NA_RELEASE
int NA_DebugRunReverbStage(NA_Batch* batch, float* hostRows, long stride, size_t n)
{
	return Guard([&] {
		if (!batch) throw std::runtime_error("NA_DebugRunReverbStage: null batch");
		batch->batch->DebugRunReverbStage(hostRows, stride, n);
	});
}
long long NA_DebugReverbLaunches(void) { return (long long)na::ReverbStageLaunches(); }
int NA_DebugReverbTwiddles(float* out, int floats)
{
	if (!out || floats < na::kRevPoints) return -1;
	std::copy(na::ReverbTwiddles(), na::ReverbTwiddles() + na::kRevPoints, out);
	return na::kRevPoints;
}
#endif

// ---- the delay stage (gpu_batch.h EnableDelayStage / SetStreamDelay) ----
namespace
{
	void DelayParamsIn(const NA_DelayParams& p, na::DelayParams& d)
	{
		d.delaySamples = p.delaySamples;
		d.feedback = p.feedback;
		d.lowpassCoeff = p.lowpassCoeff;
		d.highpassCoeff = p.highpassCoeff;
		d.wet = p.wet;
		d.dry = p.dry;
	}
	void DelayParamsOut(const na::DelayParams& d, NA_DelayParams* p)
	{
		p->delaySamples = d.delaySamples;
		p->feedback = d.feedback;
		p->lowpassCoeff = d.lowpassCoeff;
		p->highpassCoeff = d.highpassCoeff;
		p->wet = d.wet;
		p->dry = d.dry;
	}
}

int NA_DelayParamsFromMs(int sampleRate, double delayMs, double feedback, double lowCutHz, double highCutHz, double wetDb, double dryDb, NA_DelayParams* out)
{
	return Guard([&] {
		if (!out) throw std::runtime_error("NA_DelayParamsFromMs: bad argument");
		na::DelayParams d;
		if (const char* why = na::DelayParamsFromMs(sampleRate, delayMs, feedback, lowCutHz, highCutHz, wetDb, dryDb, d))
			throw std::runtime_error(std::string("NA_DelayParamsFromMs: ") + why);
		DelayParamsOut(d, out);
	});
}

int NA_BatchEnableDelayStage(NA_Batch* batch, int maxDelaySamples)
{
	return BatchCall(batch, "NA_BatchEnableDelayStage", [&](na::GpuBatch& b) { b.EnableDelayStage(maxDelaySamples); });
}

int NA_BatchGetDelayInfo(NA_Batch* batch, NA_DelayInfo* info)
{
	return BatchCall(batch, "NA_BatchGetDelayInfo", [&](na::GpuBatch& b) {
		if (!info) throw std::runtime_error("NA_BatchGetDelayInfo: bad argument");
		const na::DelayStageInfo i = b.GetDelayInfo();
		info->maxDelaySamples = i.maxDelaySamples;
		info->ringSamples = i.ringSamples;
		info->pieceSamples = i.pieceSamples;
		info->numDelays = i.numDelays;
		info->deviceBytes = i.deviceBytes;
	});
}

int NA_BatchSetStreamDelay(NA_Batch* batch, int stream, const NA_DelayParams* params, int fadeSamples)
{
	return BatchCall(batch, "NA_BatchSetStreamDelay", [&](na::GpuBatch& b) {
		if (!params)
		{
			b.SetStreamDelay(stream, nullptr, fadeSamples);
			return;
		}
		na::DelayParams d;
		DelayParamsIn(*params, d);
		b.SetStreamDelay(stream, &d, fadeSamples);
	});
}

int NA_BatchGetStreamDelay(NA_Batch* batch, int stream, NA_DelayParams* out)
{
	return BatchValue(batch, "NA_BatchGetStreamDelay", -1, [&](na::GpuBatch& b) {
		na::DelayParams d;
		const int has = b.GetStreamDelay(stream, d) ? 1 : 0;
		if (has && out) DelayParamsOut(d, out);
		return has;
	});
}

int NA_BatchStreamDelayFadeRemaining(NA_Batch* batch, int stream)
{
	return BatchValue(batch, "NA_BatchStreamDelayFadeRemaining", -1, [&](na::GpuBatch& b) { return b.StreamDelayFadeRemaining(stream); });
}

#ifndef NA_RELEASE
int NA_DebugRunDelayStage(NA_Batch* batch, float* hostRows, long stride, size_t n)
{
	return Guard([&] {
		if (!batch) throw std::runtime_error("NA_DebugRunDelayStage: null batch");
		batch->batch->DebugRunDelayStage(hostRows, stride, n);
	});
}
long long NA_DebugDelayLaunches(void) { return (long long)na::DelayStageLaunches(); }
#endif

// ---- the compressor stage (gpu_batch.h EnableCompressorStage / SetStreamCompressor) ----
static_assert(sizeof(NA_CompressorParams) == sizeof(na::CompParams) && sizeof(NA_CompressorParams) == 515 * sizeof(float), "NA_CompressorParams is CompParams, field for field");
namespace
{
	void CompParamsIn(const NA_CompressorParams& p, na::CompParams& c)
	{
		c.attackCoeff = p.attackCoeff;
		c.releaseCoeff = p.releaseCoeff;
		std::memcpy(c.curve, p.curve, sizeof(c.curve));
	}
	void CompParamsOut(const na::CompParams& c, NA_CompressorParams* p)
	{
		p->attackCoeff = c.attackCoeff;
		p->releaseCoeff = c.releaseCoeff;
		std::memcpy(p->curve, c.curve, sizeof(p->curve));
	}
}

int NA_CompressorParamsFromDb(int sampleRate, float thresholdDb, float ratio, float kneeDb, float makeupDb, float attackMs, float releaseMs, NA_CompressorParams* out)
{
	return Guard([&] {
		if (!out) throw std::runtime_error("NA_CompressorParamsFromDb: bad argument");
		na::CompParams c;
		const std::string why = na::CompParamsFromDb(sampleRate, thresholdDb, ratio, kneeDb, makeupDb, attackMs, releaseMs, c);
		if (!why.empty()) throw std::runtime_error("NA_CompressorParamsFromDb: " + why);
		CompParamsOut(c, out);
	});
}

int NA_BatchEnableCompressorStage(NA_Batch* batch)
{
	return BatchCall(batch, "NA_BatchEnableCompressorStage", [&](na::GpuBatch& b) { b.EnableCompressorStage(); });
}

int NA_BatchGetCompressorInfo(NA_Batch* batch, NA_CompressorInfo* info)
{
	return BatchCall(batch, "NA_BatchGetCompressorInfo", [&](na::GpuBatch& b) {
		if (!info) throw std::runtime_error("NA_BatchGetCompressorInfo: bad argument");
		const na::CompressorStageInfo i = b.GetCompressorInfo();
		info->curvePoints = i.curvePoints;
		info->numCompressors = i.numCompressors;
		info->deviceBytes = i.deviceBytes;
	});
}

int NA_BatchSetStreamCompressor(NA_Batch* batch, int stream, const NA_CompressorParams* params, int fadeSamples)
{
	return BatchCall(batch, "NA_BatchSetStreamCompressor", [&](na::GpuBatch& b) {
		if (!params)
		{
			b.SetStreamCompressor(stream, nullptr, fadeSamples);
			return;
		}
		na::CompParams c;
		CompParamsIn(*params, c);
		b.SetStreamCompressor(stream, &c, fadeSamples);
	});
}

int NA_BatchGetStreamCompressor(NA_Batch* batch, int stream, NA_CompressorParams* out)
{
	return BatchValue(batch, "NA_BatchGetStreamCompressor", -1, [&](na::GpuBatch& b) {
		na::CompParams c;
		const int has = b.GetStreamCompressor(stream, c) ? 1 : 0;
		if (has && out) CompParamsOut(c, out);
		return has;
	});
}

int NA_BatchStreamCompressorFadeRemaining(NA_Batch* batch, int stream)
{
	return BatchValue(batch, "NA_BatchStreamCompressorFadeRemaining", -1, [&](na::GpuBatch& b) { return b.StreamCompressorFadeRemaining(stream); });
}

float NA_BatchStreamCompressorGain(NA_Batch* batch, int stream)
{
	return BatchValue(batch, "NA_BatchStreamCompressorGain", -1.0f, [&](na::GpuBatch& b) { return b.StreamCompressorGain(stream); });
}

#ifndef NA_RELEASE
int NA_DebugRunCompressorStage(NA_Batch* batch, float* hostRows, long stride, size_t n)
{
	return Guard([&] {
		if (!batch) throw std::runtime_error("NA_DebugRunCompressorStage: null batch");
		batch->batch->DebugRunCompressorStage(hostRows, stride, n);
	});
}
long long NA_DebugCompressorLaunches(void) { return (long long)na::CompressorStageLaunches(); }
#endif

// ---- the modulation stage (gpu_batch.h EnableModStage / SetStreamMod) ----
static_assert(sizeof(NA_ModParams) == sizeof(na::ModParams) && sizeof(NA_ModParams) == 68, "NA_ModParams is ModParams, field for field");
static_assert(NA_MOD_TRIANGLE == na::kModTriangle && NA_MOD_SINE == na::kModSine, "the shapes' constants");
namespace
{
	void ModParamsIn(const NA_ModParams& p, na::ModParams& c)
	{
		c.baseSamples = p.baseSamples;
		c.depthSamples = p.depthSamples;
		c.phaseInc = p.phaseInc;
		c.shape = p.shape;
		c.numVoices = p.numVoices;
		for (int v = 0; v < na::kModMaxVoices; v++)
		{
			c.voicePhase[v] = p.voicePhase[v];
			c.voiceGain[v] = p.voiceGain[v];
		}
		c.feedback = p.feedback;
		c.wet = p.wet;
		c.dry = p.dry;
		c.tremoloDepth = p.tremoloDepth;
	}
	void ModParamsOut(const na::ModParams& c, NA_ModParams* p)
	{
		p->baseSamples = c.baseSamples;
		p->depthSamples = c.depthSamples;
		p->phaseInc = c.phaseInc;
		p->shape = c.shape;
		p->numVoices = c.numVoices;
		for (int v = 0; v < na::kModMaxVoices; v++)
		{
			p->voicePhase[v] = c.voicePhase[v];
			p->voiceGain[v] = c.voiceGain[v];
		}
		p->feedback = c.feedback;
		p->wet = c.wet;
		p->dry = c.dry;
		p->tremoloDepth = c.tremoloDepth;
	}
}

int NA_ModParamsFromMs(int sampleRate, double baseMs, double depthMs, double rateHz, int shape, int voices, double feedback, double wetDb, double dryDb, double tremoloDepth,
	NA_ModParams* out)
{
	return Guard([&] {
		if (!out) throw std::runtime_error("NA_ModParamsFromMs: bad argument");
		na::ModParams c;
		if (const char* why = na::ModParamsFromMs(sampleRate, baseMs, depthMs, rateHz, shape, voices, feedback, wetDb, dryDb, tremoloDepth, c))
			throw std::runtime_error(std::string("NA_ModParamsFromMs: ") + why);
		ModParamsOut(c, out);
	});
}

int NA_BatchEnableModStage(NA_Batch* batch, int maxDelaySamples)
{
	return BatchCall(batch, "NA_BatchEnableModStage", [&](na::GpuBatch& b) { b.EnableModStage(maxDelaySamples); });
}

int NA_BatchGetModInfo(NA_Batch* batch, NA_ModInfo* info)
{
	return BatchCall(batch, "NA_BatchGetModInfo", [&](na::GpuBatch& b) {
		if (!info) throw std::runtime_error("NA_BatchGetModInfo: bad argument");
		const na::ModStageInfo i = b.GetModInfo();
		info->maxDelaySamples = i.maxDelaySamples;
		info->ringSamples = i.ringSamples;
		info->pieceSamples = i.pieceSamples;
		info->numMods = i.numMods;
		info->deviceBytes = i.deviceBytes;
	});
}

int NA_BatchSetStreamMod(NA_Batch* batch, int stream, const NA_ModParams* params, int fadeSamples)
{
	return BatchCall(batch, "NA_BatchSetStreamMod", [&](na::GpuBatch& b) {
		if (!params)
		{
			b.SetStreamMod(stream, nullptr, fadeSamples);
			return;
		}
		na::ModParams c;
		ModParamsIn(*params, c);
		b.SetStreamMod(stream, &c, fadeSamples);
	});
}

int NA_BatchGetStreamMod(NA_Batch* batch, int stream, NA_ModParams* out)
{
	return BatchValue(batch, "NA_BatchGetStreamMod", -1, [&](na::GpuBatch& b) {
		na::ModParams c;
		const int has = b.GetStreamMod(stream, c) ? 1 : 0;
		if (has && out) ModParamsOut(c, out);
		return has;
	});
}

int NA_BatchStreamModFadeRemaining(NA_Batch* batch, int stream)
{
	return BatchValue(batch, "NA_BatchStreamModFadeRemaining", -1, [&](na::GpuBatch& b) { return b.StreamModFadeRemaining(stream); });
}

#ifndef NA_RELEASE
int NA_DebugRunModStage(NA_Batch* batch, float* hostRows, long stride, size_t n)
{
	return Guard([&] {
		if (!batch) throw std::runtime_error("NA_DebugRunModStage: null batch");
		batch->batch->DebugRunModStage(hostRows, stride, n);
	});
}
long long NA_DebugModLaunches(void) { return (long long)na::ModStageLaunches(); }
#endif

// ---- the gate stage (gpu_batch.h EnableGateStage / SetStreamGate) ----
namespace
{
	void GateParamsIn(const NA_GateParams& p, na::GateParams& g)
	{
		g.openPower = p.openPower;
		g.closePower = p.closePower;
		g.floorGain = p.floorGain;
		g.detectorCoeff = p.detectorCoeff;
		g.attackSamples = p.attackSamples;
		g.holdSamples = p.holdSamples;
		g.releaseSamples = p.releaseSamples;
	}
	void GateParamsOut(const na::GateParams& g, NA_GateParams* p)
	{
		p->openPower = g.openPower;
		p->closePower = g.closePower;
		p->floorGain = g.floorGain;
		p->detectorCoeff = g.detectorCoeff;
		p->attackSamples = g.attackSamples;
		p->holdSamples = g.holdSamples;
		p->releaseSamples = g.releaseSamples;
	}
}

int NA_GateParamsFromDb(int sampleRate, float openDb, float closeDb, float floorDb, float detectorMs, float attackMs, float holdMs, float releaseMs, NA_GateParams* out)
{
	return Guard([&] {
		if (!out) throw std::runtime_error("NA_GateParamsFromDb: bad argument");
		na::GateParams g;
		if (const char* why = na::GateParamsFromDb(sampleRate, openDb, closeDb, floorDb, detectorMs, attackMs, holdMs, releaseMs, g))
			throw std::runtime_error(std::string("NA_GateParamsFromDb: ") + why);
		GateParamsOut(g, out);
	});
}

int NA_BatchEnableGateStage(NA_Batch* batch)
{
	return BatchCall(batch, "NA_BatchEnableGateStage", [&](na::GpuBatch& b) { b.EnableGateStage(); });
}

int NA_BatchGetGateInfo(NA_Batch* batch, NA_GateInfo* info)
{
	return BatchCall(batch, "NA_BatchGetGateInfo", [&](na::GpuBatch& b) {
		if (!info) throw std::runtime_error("NA_BatchGetGateInfo: bad argument");
		const na::GateStageInfo i = b.GetGateInfo();
		info->gainSamples = i.gainSamples;
		info->numGates = i.numGates;
		info->deviceBytes = i.deviceBytes;
	});
}

int NA_BatchSetStreamGate(NA_Batch* batch, int stream, const NA_GateParams* params, int startOpen)
{
	return BatchCall(batch, "NA_BatchSetStreamGate", [&](na::GpuBatch& b) {
		if (!params)
		{
			b.SetStreamGate(stream, nullptr, false);
			return;
		}
		na::GateParams g;
		GateParamsIn(*params, g);
		b.SetStreamGate(stream, &g, startOpen != 0);
	});
}

int NA_BatchGetStreamGate(NA_Batch* batch, int stream, NA_GateParams* out)
{
	return BatchValue(batch, "NA_BatchGetStreamGate", -1, [&](na::GpuBatch& b) {
		na::GateParams g;
		const int has = b.GetStreamGate(stream, g) ? 1 : 0;
		if (has && out) GateParamsOut(g, out);
		return has;
	});
}

float NA_BatchStreamGateGain(NA_Batch* batch, int stream)
{
	return BatchValue(batch, "NA_BatchStreamGateGain", -1.0f, [&](na::GpuBatch& b) { return b.StreamGateGain(stream); });
}

#ifndef NA_RELEASE
long long NA_DebugGateLaunches(void) { return (long long)na::GateStageLaunches(); }
#endif

// ---- the meter stage (gpu_batch.h EnableMeterStage / SetStreamMeter / ReadStreamMeter) ----
static_assert(sizeof(NA_MeterTap) == sizeof(na::MeterTapReading) && sizeof(NA_MeterReading) == sizeof(na::MeterReading), "NA_MeterReading is MeterReading, field for field");

int NA_BatchEnableMeterStage(NA_Batch* batch)
{
	return BatchCall(batch, "NA_BatchEnableMeterStage", [&](na::GpuBatch& b) { b.EnableMeterStage(); });
}

int NA_BatchGetMeterInfo(NA_Batch* batch, NA_MeterInfo* info)
{
	return BatchCall(batch, "NA_BatchGetMeterInfo", [&](na::GpuBatch& b) {
		if (!info) throw std::runtime_error("NA_BatchGetMeterInfo: bad argument");
		const na::MeterStageInfo i = b.GetMeterInfo();
		info->numMeters = i.numMeters;
		info->deviceBytes = i.deviceBytes;
	});
}

int NA_BatchSetStreamMeter(NA_Batch* batch, int stream, const NA_MeterParams* params)
{
	return BatchCall(batch, "NA_BatchSetStreamMeter", [&](na::GpuBatch& b) {
		if (!params)
		{
			b.SetStreamMeter(stream, nullptr);
			return;
		}
		na::MeterParams m;
		m.windowSamples = params->windowSamples;
		m.clipLevelIn = params->clipLevelIn;
		m.clipLevelOut = params->clipLevelOut;
		b.SetStreamMeter(stream, &m);
	});
}

int NA_BatchGetStreamMeter(NA_Batch* batch, int stream, NA_MeterParams* out)
{
	return BatchValue(batch, "NA_BatchGetStreamMeter", -1, [&](na::GpuBatch& b) {
		na::MeterParams m;
		const int has = b.GetStreamMeter(stream, m) ? 1 : 0;
		if (has && out)
		{
			out->windowSamples = m.windowSamples;
			out->clipLevelIn = m.clipLevelIn;
			out->clipLevelOut = m.clipLevelOut;
		}
		return has;
	});
}

int NA_BatchReadStreamMeter(NA_Batch* batch, int stream, NA_MeterReading* out)
{
	return BatchValue(batch, "NA_BatchReadStreamMeter", -1, [&](na::GpuBatch& b) {
		na::MeterReading r;
		const int has = b.ReadStreamMeter(stream, r) ? 1 : 0;
		if (has && out) memcpy(out, &r, sizeof(r));
		return has;
	});
}

#ifndef NA_RELEASE
long long NA_DebugMeterLaunches(void) { return (long long)na::MeterStageLaunches(); }
#endif

// ---- the tuner stage (gpu_batch.h EnableTunerStage / SetStreamTuner / ReadStreamTuner) ----
static_assert(sizeof(NA_TunerParams) == sizeof(na::TunerParams) && sizeof(NA_TunerReading) == sizeof(na::TunerReading), "NA_TunerParams / NA_TunerReading are TunerParams / TunerReading, field for field");

int NA_BatchEnableTunerStage(NA_Batch* batch)
{
	return BatchCall(batch, "NA_BatchEnableTunerStage", [&](na::GpuBatch& b) { b.EnableTunerStage(); });
}

int NA_BatchGetTunerInfo(NA_Batch* batch, NA_TunerInfo* info)
{
	return BatchCall(batch, "NA_BatchGetTunerInfo", [&](na::GpuBatch& b) {
		if (!info) throw std::runtime_error("NA_BatchGetTunerInfo: bad argument");
		const na::TunerStageInfo i = b.GetTunerInfo();
		info->numTuners = i.numTuners;
		info->deviceBytes = i.deviceBytes;
	});
}

int NA_BatchSetStreamTuner(NA_Batch* batch, int stream, const NA_TunerParams* params)
{
	return BatchCall(batch, "NA_BatchSetStreamTuner", [&](na::GpuBatch& b) {
		if (!params)
		{
			b.SetStreamTuner(stream, nullptr);
			return;
		}
		na::TunerParams t;
		memcpy(&t, params, sizeof(t));
		b.SetStreamTuner(stream, &t);
	});
}

int NA_BatchGetStreamTuner(NA_Batch* batch, int stream, NA_TunerParams* out)
{
	return BatchValue(batch, "NA_BatchGetStreamTuner", -1, [&](na::GpuBatch& b) {
		na::TunerParams t;
		const int has = b.GetStreamTuner(stream, t) ? 1 : 0;
		if (has && out) memcpy(out, &t, sizeof(t));
		return has;
	});
}

int NA_BatchReadStreamTuner(NA_Batch* batch, int stream, NA_TunerReading* out)
{
	return BatchValue(batch, "NA_BatchReadStreamTuner", -1, [&](na::GpuBatch& b) {
		na::TunerReading r;
		const int has = b.ReadStreamTuner(stream, r) ? 1 : 0;
		if (has && out) memcpy(out, &r, sizeof(r));
		return has;
	});
}

int NA_TunerParamsFromRange(double sampleRate, double lowestHz, double highestHz, double evaluationsPerSecond, NA_TunerParams* out)
{
	return Guard([&] {
		if (!out) throw std::runtime_error("NA_TunerParamsFromRange: bad argument");
		na::TunerParams t;
		if (const char* why = na::TunerParamsFromRange(sampleRate, lowestHz, highestHz, evaluationsPerSecond, t)) throw std::runtime_error(std::string("NA_TunerParamsFromRange: ") + why);
		memcpy(out, &t, sizeof(t));
	});
}

int NA_TunerPitch(const NA_TunerReading* reading, double sampleRate, double* hz, double* clarity)
{
	int has = 0;
	const int rc = Guard([&] {
		if (!reading || !(sampleRate > 0.0)) throw std::runtime_error("NA_TunerPitch: bad argument");
		na::TunerReading r;
		memcpy(&r, reading, sizeof(r));
		double f = 0.0, c = 0.0;
		has = na::TunerPitch(r, sampleRate, f, c) ? 1 : 0;
		if (hz) *hz = f;
		if (clarity) *clarity = c;
	});
	return rc != 0 ? -1 : has;
}

#ifndef NA_RELEASE
long long NA_DebugTunerLaunches(void) { return (long long)na::TunerStageLaunches(); }
#endif

// ---- the mix stage (gpu_batch.h EnableMixStage / SetMixGroup) ----
static_assert(NA_MIX_MAX_MEMBERS == na::kMixMaxMembers && NA_MIX_TAP_OUT == na::kMixTapOut && NA_MIX_TAP_DRY == na::kMixTapDry, "the header's mix constants are mix_stage.h's");

int NA_BatchEnableMixStage(NA_Batch* batch)
{
	return BatchCall(batch, "NA_BatchEnableMixStage", [&](na::GpuBatch& b) { b.EnableMixStage(); });
}

int NA_BatchGetMixInfo(NA_Batch* batch, NA_MixInfo* info)
{
	return BatchCall(batch, "NA_BatchGetMixInfo", [&](na::GpuBatch& b) {
		if (!info) throw std::runtime_error("NA_BatchGetMixInfo: bad argument");
		const na::MixStageInfo i = b.GetMixInfo();
		info->maxMembers = i.maxMembers;
		info->numGroups = i.numGroups;
		info->drySamples = i.drySamples;
		info->deviceBytes = i.deviceBytes;
	});
}

int NA_BatchSetMixGroup(NA_Batch* batch, const int* streams, const int* taps, int numMembers, int numOutputs, const float* gains, int rampSamples)
{
	return BatchCall(batch, "NA_BatchSetMixGroup", [&](na::GpuBatch& b) { b.SetMixGroup(streams, taps, numMembers, numOutputs, gains, rampSamples); });
}

int NA_BatchClearMixGroup(NA_Batch* batch, int stream)
{
	return BatchCall(batch, "NA_BatchClearMixGroup", [&](na::GpuBatch& b) { b.ClearMixGroup(stream); });
}

int NA_BatchGetStreamMix(NA_Batch* batch, int stream, int* streams, int* taps, int capacity, int* numOutputs, float* gains)
{
	return BatchValue(batch, "NA_BatchGetStreamMix", -1, [&](na::GpuBatch& b) { return b.GetStreamMix(stream, streams, taps, capacity, numOutputs, gains); });
}

int NA_BatchMixRampRemaining(NA_Batch* batch, int stream)
{
	return BatchValue(batch, "NA_BatchMixRampRemaining", -1, [&](na::GpuBatch& b) { return b.MixRampRemaining(stream); });
}

int NA_MixGainsFromPan(double levelDb, double pan, float* left, float* right)
{
	return Guard([&] {
		if (!left || !right) throw std::runtime_error("NA_MixGainsFromPan: bad argument");
		if (!std::isfinite(levelDb) || !std::isfinite(pan)) throw std::runtime_error("NA_MixGainsFromPan: every argument must be finite");
		if (pan < -1.0 || pan > 1.0) throw std::runtime_error("NA_MixGainsFromPan: pan must lie in [-1, 1]");
		const double level = std::pow(10.0, levelDb / 20.0);
		const double angle = (pan + 1.0) * (3.14159265358979323846 / 4.0);
		// (the ends are exact by rule: cos(pi / 2) in double is 6e-17, not 0)
		*left = pan == 1.0 ? 0.0f : pan == -1.0 ? (float)level : (float)(level * std::cos(angle));
		*right = pan == -1.0 ? 0.0f : pan == 1.0 ? (float)level : (float)(level * std::sin(angle));
	});
}

#ifndef NA_RELEASE
long long NA_DebugMixLaunches(void) { return (long long)na::MixStageLaunches(); }
long long NA_DebugMixStashLaunches(void) { return (long long)na::MixStashLaunches(); }
int NA_DebugRunMixStage(NA_Batch* batch, const float* hostIn, float* hostRows, long stride, size_t n)
{
	return Guard([&] {
		if (!batch) throw std::runtime_error("NA_DebugRunMixStage: null batch");
		batch->batch->DebugRunMixStage(hostIn, hostRows, stride, n);
	});
}
#endif

// ---- the EQ stage (gpu_batch.h EnableEqStage / SetStreamEq) ----
static_assert(sizeof(NA_EqSection) == sizeof(na::EqSection) && NA_EQ_MAX_SECTIONS == na::kEqMaxSections, "NA_EqSection is na::EqSection");
namespace
{
	void EqSectionIn(const NA_EqSection& p, na::EqSection& s)
	{
		s.b0 = p.b0;
		s.b1 = p.b1;
		s.b2 = p.b2;
		s.a1 = p.a1;
		s.a2 = p.a2;
	}
	void EqSectionOut(const na::EqSection& s, NA_EqSection* p)
	{
		p->b0 = s.b0;
		p->b1 = s.b1;
		p->b2 = s.b2;
		p->a1 = s.a1;
		p->a2 = s.a2;
	}
}

int NA_EqSectionFromDesign(int kind, double sampleRate, double freqHz, double q, double gainDb, NA_EqSection* out)
{
	return Guard([&] {
		if (!out) throw std::runtime_error("NA_EqSectionFromDesign: bad argument");
		na::EqSection s;
		if (const char* why = na::EqSectionFromDesign(kind, sampleRate, freqHz, q, gainDb, s)) throw std::runtime_error(std::string("NA_EqSectionFromDesign: ") + why);
		EqSectionOut(s, out);
	});
}

int NA_BatchEnableEqStage(NA_Batch* batch)
{
	return BatchCall(batch, "NA_BatchEnableEqStage", [&](na::GpuBatch& b) { b.EnableEqStage(); });
}

int NA_BatchGetEqInfo(NA_Batch* batch, NA_EqInfo* info)
{
	return BatchCall(batch, "NA_BatchGetEqInfo", [&](na::GpuBatch& b) {
		if (!info) throw std::runtime_error("NA_BatchGetEqInfo: bad argument");
		const na::EqStageInfo i = b.GetEqInfo();
		info->maxSections = i.maxSections;
		info->numEntries = i.numEntries;
		info->deviceBytes = i.deviceBytes;
	});
}

int NA_BatchSetStreamEq(NA_Batch* batch, int stream, const NA_EqSection* sections, int numSections, int fadeSamples)
{
	return BatchCall(batch, "NA_BatchSetStreamEq", [&](na::GpuBatch& b) {
		na::EqSection s[na::kEqMaxSections];
		if (sections)
			for (int i = 0; i < std::min(std::max(numSections, 0), na::kEqMaxSections); i++) EqSectionIn(sections[i], s[i]);
		b.SetStreamEq(stream, sections ? s : nullptr, numSections, fadeSamples);
	});
}

int NA_BatchGetStreamEq(NA_Batch* batch, int stream, NA_EqSection* out, int capacity)
{
	return BatchValue(batch, "NA_BatchGetStreamEq", -1, [&](na::GpuBatch& b) {
		na::EqSection s[na::kEqMaxSections];
		const int count = b.GetStreamEq(stream, s, na::kEqMaxSections);
		if (out)
			for (int i = 0; i < std::min(count, capacity); i++) EqSectionOut(s[i], &out[i]);
		return count;
	});
}

int NA_BatchStreamEqFadeRemaining(NA_Batch* batch, int stream)
{
	return BatchValue(batch, "NA_BatchStreamEqFadeRemaining", -1, [&](na::GpuBatch& b) { return b.StreamEqFadeRemaining(stream); });
}

#ifndef NA_RELEASE
long long NA_DebugEqLaunches(void) { return (long long)na::EqStageLaunches(); }
int NA_DebugRunEqStage(NA_Batch* batch, float* hostRows, long stride, size_t n)
{
	return Guard([&] {
		if (!batch) throw std::runtime_error("NA_DebugRunEqStage: null batch");
		batch->batch->DebugRunEqStage(hostRows, stride, n);
	});
}
#endif

#ifndef NA_RELEASE
long long NA_DebugDeviceResourceCalls(void) { return na::DeviceResourceCalls(); }
#endif

int NA_BatchNumStreams(NA_Batch* batch) { return batch ? batch->batch->NumStreams() : -1; }

int NA_BatchNumLiveStreams(NA_Batch* batch) { return batch ? batch->batch->NumLiveStreams() : -1; }

int NA_BatchIsLive(NA_Batch* batch, int stream) { return (batch && batch->batch->IsLive(stream)) ? 1 : 0; }

int NA_BatchRemoveStreams(NA_Batch* batch, int first, int count)
{
	if (!batch) return -1;
	return Guard([&] { batch->batch->RemoveStreams(first, count); });
}

// ---- stream snapshots (csrc/stream_snapshot.h) ----
namespace
{
	NeuralAudio::GpuModel* OwnModel(NeuralModel* model, const char* who)
	{
		NeuralAudio::GpuModel* gm = model ? dynamic_cast<NeuralAudio::GpuModel*>(model->model) : nullptr;
		if (!gm) throw std::runtime_error(std::string(who) + ": model is null or was not created by this library");
		return gm;
	}
}

long long NA_BatchStreamSnapshotBytes(NA_Batch* batch, int stream)
{
	long long n = -1;
	Guard([&] {
		if (!batch) throw std::runtime_error("NA_BatchStreamSnapshotBytes: null batch");
		n = (long long)batch->batch->StreamSnapshotBytes(stream);
	});
	return n;
}

long long NA_ModelSnapshotBytes(NeuralModel* model)
{
	long long n = -1;
	Guard([&] { n = (long long)na::SnapshotBytes(*OwnModel(model, "NA_ModelSnapshotBytes")->GetLoadedModel()); });
	return n;
}

unsigned long long NA_ModelSnapshotFingerprint(NeuralModel* model)
{
	unsigned long long f = 0;
	Guard([&] { f = na::ModelFingerprint(*OwnModel(model, "NA_ModelSnapshotFingerprint")->GetLoadedModel()); });
	return f;
}

int NA_BatchSaveStreams(NA_Batch* batch, const int* streams, int count, void* buf, size_t capacity, size_t* written)
{
	if (written) *written = 0;
	return Guard([&] {
		if (!batch) throw std::runtime_error("NA_BatchSaveStreams: null batch (a batch needs a HIP device: there is no host-side stream state)");
		const size_t need = batch->batch->SaveStreams(streams, count, buf, capacity);
		if (written) *written = need;
		if (need > capacity) throw std::runtime_error("NA_BatchSaveStreams: buffer too small: " + std::to_string(need) + " bytes needed, " + std::to_string(capacity) + " given");
	});
}

int NA_BatchLoadStreams(NA_Batch* batch, const int* streams, int count, const void* buf, size_t bytes)
{
	return Guard([&] {
		if (!batch) throw std::runtime_error("NA_BatchLoadStreams: null batch (a batch needs a HIP device: there is no host-side stream state)");
		batch->batch->LoadStreams(streams, count, buf, bytes);
	});
}

int NA_SaveModelState(NeuralModel* model, void* buf, size_t capacity, size_t* written)
{
	if (written) *written = 0;
	return Guard([&] {
		const size_t need = OwnModel(model, "NA_SaveModelState")->SaveState(buf, capacity);
		if (written) *written = need;
		if (need > capacity) throw std::runtime_error("NA_SaveModelState: buffer too small: " + std::to_string(need) + " bytes needed, " + std::to_string(capacity) + " given");
	});
}

int NA_LoadModelState(NeuralModel* model, const void* buf, size_t bytes)
{
	return Guard([&] { OwnModel(model, "NA_LoadModelState")->LoadState(buf, bytes); });
}

#ifndef NA_RELEASE
long long NA_DebugSnapshotLaunches(void) { return na::SnapshotKernelLaunches(); }
#endif

int NA_BatchSetQuality(NA_Batch* batch, int stream, float quality)
{
	if (!batch) return -1;
	return Guard([&] { batch->batch->SetQuality(stream, quality); });
}

int NA_BatchIsQualityChangeRealtimeSafe(NA_Batch* batch, int stream, float quality)
{
	int safe = 0;
	if (!batch) return 0;
	Guard([&] { safe = batch->batch->IsQualityChangeRealtimeSafe(stream, quality) ? 1 : 0; });
	return safe;
}

int NA_BatchGetActiveSubModel(NA_Batch* batch, int stream)
{
	int idx = -1;
	if (!batch) return -1;
	Guard([&] { idx = batch->batch->GetActiveSubModel(stream); });
	return idx;
}

int NA_BatchPrewarm(NA_Batch* batch, int stream)
{
	if (!batch) return -1;
	return Guard([&] {
		if (stream >= 0) batch->batch->Prewarm(stream);
		else
			for (int s = 0; s < batch->batch->NumStreams(); s++)
				if (!batch->batch->IsParked(s)) batch->batch->Prewarm(s); // (a parked stream is armed already)
	});
}

int NA_BatchProcess(NA_Batch* batch, const float* in, float* out, size_t n)
{
	if (!batch || !out)
	{
		SetError("NA_BatchProcess: null argument");
		return -1;
	}
	const int rc = Guard([&] { batch->batch->ProcessHost(in, out, n); });
	// (an audio host must never be handed stale or uninitialised rows: a failed buffer is silence, like the legacy Process)
	if (rc != 0) memset(out, 0, (size_t)batch->batch->NumStreams() * n * sizeof(float));
	return rc;
}

int NA_RegisterHostBuffer(void* ptr, size_t bytes)
{
	return Guard([&] {
		std::string error;
		if (!na::RegisterHostBuffer(ptr, bytes, error)) throw std::runtime_error(error);
	});
}

int NA_UnregisterHostBuffer(void* ptr) { return na::UnregisterHostBuffer(ptr) ? 0 : -1; }

int NA_BatchSubmit(NA_Batch* batch, const float* in, size_t n)
{
	int ticket = -1;
	if (!batch) return -1;
	const int rc = Guard([&] { ticket = batch->batch->Submit(in, n); });
	return rc == 0 ? ticket : -1;
}

int NA_BatchCollect(NA_Batch* batch, int ticket, float* out)
{
	if (!batch) return -1;
	return Guard([&] { batch->batch->Collect(ticket, out); });
}

float* NA_BatchNextInput(NA_Batch* batch, size_t n)
{
	float* ptr = nullptr;
	if (!batch) return nullptr;
	Guard([&] { ptr = batch->batch->NextInput(n); });
	return ptr;
}

const float* NA_BatchOutputView(NA_Batch* batch, int ticket)
{
	const float* ptr = nullptr;
	if (!batch) return nullptr;
	Guard([&] { ptr = batch->batch->OutputView(ticket); });
	return ptr;
}

int NA_BatchProcessDevice(NA_Batch* batch, const float* dIn, float* dOut, size_t n, long inStride, long outStride)
{
	if (!batch) return -1;
	return Guard([&] { batch->batch->ProcessDevice(dIn, dOut, n, inStride, outStride); });
}

int NA_BatchSynchronize(NA_Batch* batch)
{
	if (!batch) return -1;
	return Guard([&] { batch->batch->Synchronize(); });
}

int NA_BatchSetWaitLimitMs(NA_Batch* batch, double milliseconds)
{
	if (!batch) return -1;
	batch->batch->SetWaitLimitMs(milliseconds);
	return 0;
}

double NA_BatchGetWaitLimitMs(NA_Batch* batch) { return batch ? batch->batch->GetWaitLimitMs() : 0.0; }

int NA_BatchIsBroken(NA_Batch* batch) { return (batch && batch->batch->IsBroken()) ? 1 : 0; }

#ifndef NA_RELEASE
int NA_DebugStallDevice(NA_Batch* batch, double milliseconds)
{
	if (!batch) return -1;
	return Guard([&] { batch->batch->DebugStallDevice(milliseconds); });
}

int NA_DebugLastHostRoute(NA_Batch* batch) { return batch ? batch->batch->DebugLastHostRoute() : -1; }

int NA_DebugMultiLastHostRoute(NA_MultiBatch* mb, int shard)
{
	int route = -1;
	if (mb) Guard([&] { route = mb->multi->DebugShardLastHostRoute(shard); });
	return route;
}
#endif

void* NA_BatchGetHipStream(NA_Batch* batch) { return batch ? reinterpret_cast<void*>(batch->batch->GetStream()) : nullptr; }

int NA_BatchMarkTime(NA_Batch* batch, int which)
{
	if (!batch) return -1;
	return Guard([&] { batch->batch->MarkTime(which); });
}

int NA_BatchWaitMarks(NA_Batch* batch)
{
	if (!batch) return -1;
	return Guard([&] { batch->batch->WaitMarks(); });
}

float NA_BatchElapsedMs(NA_Batch* batch)
{
	if (!batch) return -1.0f;
	float ms = -1.0f;
	return Guard([&] { ms = batch->batch->ElapsedMs(); }) == 0 ? ms : -1.0f;
}

int NA_BatchUsesHalfLaunches(NA_Batch* batch) { return batch && batch->batch->UsesHalfLaunches() ? 1 : 0; }
int NA_BatchSetResidentLaunch(NA_Batch* batch, int on)
{
	if (!batch) return -1;
	return Guard([&] { batch->batch->SetResidentLaunch(on != 0); });
}
int NA_BatchUsesResidentLaunch(NA_Batch* batch) { return batch && batch->batch->UsesResidentLaunch() ? 1 : 0; }

int NA_BatchWaitOutputs(NA_Batch* batch)
{
	if (!batch) return -1;
	return Guard([&] { batch->batch->WaitOutputs(); });
}

double NA_BatchAlgorithmicBytesPerSample(NA_Batch* batch, int blockFrames)
{
	return batch ? batch->batch->AlgorithmicBytesPerSample(blockFrames) : 0.0;
}

double NA_BatchMacsPerSample(NA_Batch* batch) { return batch ? batch->batch->MacsPerSample() : 0.0; }

float NA_BatchStreamInputLimit(NA_Batch* batch, int stream)
{
	try { return batch ? batch->batch->StreamInputLimit(stream) : 0.0f; }
	catch (...) { return 0.0f; }
}

// ---- multi-GPU host (multi_gpu.h) ---------------------------------------------------------------------------------------------
int NA_ShardByCost(const double* cost, int n, int parts, int* bounds)
{
	return Guard([&] {
		if (!cost && n > 0) throw std::runtime_error("NA_ShardByCost: bad argument");
		if (!bounds) throw std::runtime_error("NA_ShardByCost: bad argument");
		const std::vector<int> b = na::ShardByCost(cost, n, parts);
		for (size_t i = 0; i < b.size(); i++) bounds[i] = b[i];
	});
}

double NA_ModelStreamCost(NeuralModel* model, float quality)
{
	double c = -1.0;
	Guard([&] {
		NeuralAudio::GpuModel* gm = model ? dynamic_cast<NeuralAudio::GpuModel*>(model->model) : nullptr;
		if (!gm) throw std::runtime_error("NA_ModelStreamCost: model was not created by this library");
		c = na::EstimateStreamCost(*gm->GetLoadedModel(), quality);
	});
	return c;
}

// Host side only (no GPU needed): which WaveNet kernel family a batch of `streams` streams of the model would run on, and the static
// range proof of the f16-split kernels behind the choice (wavenet_plan.cpp)
int NA_ModelKernelInfo(NeuralModel* model, float quality, int streams, char* kernelBuf, int bufSize, float* inputLimit, int* rangeProven, int* weightsOk, int* packFactor)
{
	int r = -1;
	Guard([&] {
		NeuralAudio::GpuModel* gm = model ? dynamic_cast<NeuralAudio::GpuModel*>(model->model) : nullptr;
		if (!gm) throw std::runtime_error("NA_ModelKernelInfo: model was not created by this library");
		const na::ModelKernelInfo info = na::PredictModelKernel(*gm->GetLoadedModel(), quality, streams);
		if (kernelBuf && bufSize > 0)
		{
			strncpy(kernelBuf, info.kernel, (size_t)bufSize - 1);
			kernelBuf[bufSize - 1] = 0;
		}
		if (inputLimit) *inputLimit = info.inputLimit;
		if (rangeProven) *rangeProven = info.rangeProven ? 1 : 0;
		if (weightsOk) *weightsOk = info.weightsOk ? 1 : 0;
		if (packFactor) *packFactor = info.pack;
		r = 0;
	});
	return r;
}

int NA_BatchStreamRangeEvents(NA_Batch* b, int stream)
{
	int r = -1;
	Guard([&] {
		if (!b) throw std::runtime_error("NA_BatchStreamRangeEvents: null batch");
		r = b->batch->StreamRangeEvents(stream);
	});
	return r;
}

NA_MultiBatch* NA_MultiCreate(const int* devices, int numDevices)
{
	NA_MultiBatch* mb = nullptr;
	Guard([&] {
		if (!devices || numDevices < 1) throw std::runtime_error("NA_MultiCreate: bad argument");
		na::MultiGpuBatch* m = new na::MultiGpuBatch(std::vector<int>(devices, devices + numDevices));
		mb = new NA_MultiBatch{ m };
	});
	return mb;
}

void NA_MultiDestroy(NA_MultiBatch* mb)
{
	if (!mb) return;
	Guard([&] { delete mb->multi; });
	delete mb;
}

int NA_MultiAddStreams(NA_MultiBatch* mb, NeuralModel* model, float quality, int count, int doPrewarm)
{
	int first = -1;
	const int rc = Guard([&] {
		NeuralAudio::GpuModel* gm = (mb && model) ? dynamic_cast<NeuralAudio::GpuModel*>(model->model) : nullptr;
		if (!gm || count < 1) throw std::runtime_error("NA_MultiAddStreams: bad argument");
		first = mb->multi->AddStreams(gm->GetLoadedModel(), quality, count, doPrewarm != 0, gm->IsOnDemand());
	});
	return rc == 0 ? first : -1;
}

int NA_MultiCommit(NA_MultiBatch* mb)
{
	if (!mb) return -1;
	return Guard([&] { mb->multi->Commit(); });
}

int NA_MultiNumStreams(NA_MultiBatch* mb) { return mb ? mb->multi->NumStreams() : -1; }
int NA_MultiNumShards(NA_MultiBatch* mb) { return mb ? mb->multi->NumShards() : -1; }

int NA_MultiShardRange(NA_MultiBatch* mb, int shard, int* begin, int* end, int* device)
{
	if (!mb) return -1;
	return Guard([&] {
		int b = 0, e = 0, d = 0;
		mb->multi->ShardRange(shard, b, e, d);
		if (begin) *begin = b;
		if (end) *end = e;
		if (device) *device = d;
	});
}

int NA_MultiProcess(NA_MultiBatch* mb, const float* in, float* out, size_t n)
{
	if (!mb || !in || !out) return -1;
	return Guard([&] { mb->multi->Process(in, out, n); });
}

int NA_MultiSubmit(NA_MultiBatch* mb, const float* in, size_t n)
{
	int ticket = -1;
	if (!mb || !in) return -1;
	const int rc = Guard([&] { ticket = mb->multi->Submit(in, n); });
	return rc == 0 ? ticket : -1;
}

int NA_MultiCollect(NA_MultiBatch* mb, int ticket, float* out)
{
	if (!mb) return -1;
	return Guard([&] { mb->multi->Collect(ticket, out); });
}

// 0 = host rows (default), 1 = RCCL (see multi_gpu.h FanIn); before NA_MultiCommit / the first NA_MultiProcess
int NA_MultiSetFanIn(NA_MultiBatch* mb, int mode)
{
	if (!mb) return -1;
	return Guard([&] {
		if (mode != 0 && mode != 1) throw std::runtime_error("NA_MultiSetFanIn: mode must be 0 (host rows) or 1 (RCCL)");
		mb->multi->SetFanIn(mode == 1 ? na::MultiGpuBatch::FanIn::Rccl : na::MultiGpuBatch::FanIn::HostRows);
	});
}

const float* NA_MultiGatheredOutput(NA_MultiBatch* mb, int shard)
{
	const float* p = nullptr;
	if (!mb) return nullptr;
	Guard([&] { p = mb->multi->GatheredOutput(shard); });
	return p;
}

// 1 when librccl.so can be loaded and exports every entry point the multi-GPU host binds (rccl_dyn.cpp); no GPU needed
int NA_RcclAvailable(void)
{
	int ok = 0;
	Guard([&] {
		std::string error;
		if (na::rccl::Load(error) == nullptr) throw std::runtime_error(error);
		ok = 1;
	});
	return ok;
}

#ifndef NA_RELEASE
void NA_DebugSetRcclApi(int mode, int failSendAt, int rendezvousMs)
{
	na::rccl::LoopbackConfigure(failSendAt, rendezvousMs);
	na::rccl::SetOverride(mode == 1 ? na::rccl::LoopbackApi() : nullptr);
}
#endif

int NA_MultiSetQuality(NA_MultiBatch* mb, int stream, float quality)
{
	if (!mb) return -1;
	return Guard([&] { mb->multi->SetQuality(stream, quality); });
}

#ifndef NA_RELEASE
void NA_DebugSetWaveNetSpec(int on) { na::SetWaveNetSpecEnabled(on != 0); }
#endif

#ifndef NA_RELEASE
int NA_DebugSetRecurrentQuadMin(int streams) { return na::SetRecurrentQuadMinStreams(streams); }
#endif

#ifndef NA_RELEASE
long long NA_DebugRecurrentQuadLaunches(void) { return (long long)na::RecurrentQuadLaunches(); }
#endif

#ifndef NA_RELEASE
void NA_DebugSetTraceBuffer(void* deviceBuffer) { na::SetWaveNetTraceBuffer(reinterpret_cast<long long*>(deviceBuffer)); }
#endif

double NA_BatchStateBytes(NA_Batch* batch) { return batch ? (double)batch->batch->StateBytes() : 0.0; }

const char* NA_BatchStreamKernelName(NA_Batch* batch, int stream)
{
	try { return batch ? batch->batch->StreamKernelName(stream) : ""; }
	catch (...) { return ""; }
}

int NA_BatchStreamPackFactor(NA_Batch* batch, int stream)
{
	try { return batch ? batch->batch->StreamPackFactor(stream) : 0; }
	catch (...) { return 0; }
}

// ---------------------------------------------------------------- offline rendering (csrc/offline_render.cpp)

namespace
{
	// jobs of the C ABI -> the renderer's, with the device they run on (job 0's model's); throws on a bad argument
	int RenderJobs(const NA_RenderJob* jobs, int numJobs, const NA_RenderOptions* opts, std::vector<na::RenderJobDesc>& out, na::RenderOptionsDesc& o)
	{
		if (!jobs) throw std::runtime_error("offline render: jobs is NULL");
		if (numJobs <= 0) throw std::runtime_error("offline render: numJobs must be >= 1");
		int device = -1;
		out.clear();
		for (int j = 0; j < numJobs; j++)
		{
			const NA_RenderJob& job = jobs[j];
			NeuralAudio::GpuModel* gm = job.model ? dynamic_cast<NeuralAudio::GpuModel*>(job.model->model) : nullptr;
			if (!job.model) throw std::runtime_error("offline render: job " + std::to_string(j) + " has a NULL model");
			if (!gm) throw std::runtime_error("offline render: job " + std::to_string(j) + ": model was not created by this library");
			if (device < 0) device = gm->GetDevice();
			else if (gm->GetDevice() != device) throw std::runtime_error("offline render: the jobs' models are on different devices");
			na::RenderJobDesc d;
			d.model = gm->GetLoadedModel();
			d.quality = job.quality;
			d.input = job.input;
			d.output = job.output;
			d.numSamples = job.numSamples;
			out.push_back(d);
		}
		o = na::RenderOptionsDesc();
		if (opts)
		{
			o.segmentSamples = opts->segmentSamples;
			o.maxSamplesPerPass = opts->maxSamplesPerPass;
			o.waitLimitMs = opts->waitLimitMs;
		}
		return device;
	}
}

namespace
{
	void FillRenderPlanInfo(const na::RenderPlan& p, const std::string& kernel, NA_RenderPlanInfo* info)
	{
		memset(info, 0, sizeof(*info));
		info->segments = p.segments;
		info->lead = p.lead;
		info->segmentSamples = p.stride > 0 ? p.stride : 0;
		info->rowSamples = p.rowSamples;
		info->passes = p.passes;
		info->streams = p.rows;
		info->estimatedMs = p.estimatedMs;
		strncpy(info->kernel, kernel.c_str(), sizeof(info->kernel) - 1);
	}
}

int NA_RenderOffline(const NA_RenderJob* jobs, int numJobs, const NA_RenderOptions* opts)
{
	return Guard([&] {
		std::vector<na::RenderJobDesc> js;
		na::RenderOptionsDesc o;
		const int device = RenderJobs(jobs, numJobs, opts, js, o);
		na::RenderOffline(js, o, device);
	});
}

int NA_RenderPlan(const NA_RenderJob* jobs, int numJobs, const NA_RenderOptions* opts, NA_RenderPlanInfo* info)
{
	return Guard([&] {
		if (!info) throw std::runtime_error("NA_RenderPlan: info is NULL");
		std::vector<na::RenderJobDesc> js;
		na::RenderOptionsDesc o;
		const int device = RenderJobs(jobs, numJobs, opts, js, o);
		std::string kernel;
		FillRenderPlanInfo(na::PlanOfflineRenderOn(js, o, device, &kernel), kernel, info);
	});
}

// ---------------------------------------------------------------- batch resampling (csrc/resample.cpp)

namespace
{
	void FillResampleInfo(const na::ResamplePlan& p, NA_ResampleInfo* info);
}

int NA_RenderOfflineAtRate(const NA_RenderJob* jobs, int numJobs, const NA_RenderOptions* opts, int externalRate)
{
	return Guard([&] {
		std::vector<na::RenderJobDesc> js;
		na::RenderOptionsDesc o;
		const int device = RenderJobs(jobs, numJobs, opts, js, o);
		na::RenderOfflineAtRate(js, o, device, externalRate);
	});
}

int NA_RenderPlanAtRate(const NA_RenderJob* jobs, int numJobs, const NA_RenderOptions* opts, int externalRate, NA_RenderPlanInfo* info, NA_ResampleInfo* resample)
{
	return Guard([&] {
		if (!info) throw std::runtime_error("NA_RenderPlanAtRate: info is NULL");
		std::vector<na::RenderJobDesc> js;
		na::RenderOptionsDesc o;
		const int device = RenderJobs(jobs, numJobs, opts, js, o);
		std::string kernel;
		na::ResamplePlan first;
		FillRenderPlanInfo(na::PlanOfflineRenderAtRateOn(js, o, device, externalRate, &kernel, &first), kernel, info);
		if (resample) FillResampleInfo(first, resample);
	});
}

#ifndef NA_RELEASE
void NA_DebugSetRenderTap(float* modelIn, float* modelOut, long long capacity) { na::SetRenderTap(modelIn, modelOut, capacity); }
#endif

int NA_MultiSetResampling(NA_MultiBatch* mb, int externalRate, int modelRate, int quantum, int maxFrames)
{
	return Guard([&] {
		if (!mb) throw std::runtime_error("NA_MultiSetResampling: null multi batch");
		mb->multi->SetResampling(externalRate, modelRate, quantum, maxFrames);
	});
}

int NA_MultiGetResampleInfo(NA_MultiBatch* mb, NA_ResampleInfo* info)
{
	return Guard([&] {
		if (!mb || !info) throw std::runtime_error("NA_MultiGetResampleInfo: null argument");
		FillResampleInfo(mb->multi->ResamplingPlan(), info);
	});
}

namespace
{
	void FillResampleInfo(const na::ResamplePlan& p, NA_ResampleInfo* info)
	{
		memset(info, 0, sizeof(*info));
		info->externalRate = p.externalRate;
		info->modelRate = p.modelRate;
		info->ticksExternal = p.te;
		info->ticksModel = p.tm;
		info->tapsUp = p.tapsUp;
		info->tapsDown = p.tapsDown;
		info->quantum = p.quantum;
		info->latencySamples = p.latency;
		info->prototypeLength = p.K;
	}
}

int NA_ResamplePlan(int externalRate, int modelRate, int quantum, NA_ResampleInfo* info)
{
	return Guard([&] {
		if (!info) throw std::runtime_error("NA_ResamplePlan: info is NULL");
		FillResampleInfo(na::PlanResampling(externalRate, modelRate, quantum), info);
	});
}

int NA_ResamplePrototype(int externalRate, int modelRate, float* buf, int capacity)
{
	int k = -1;
	Guard([&] {
		const na::ResamplePlan p = na::PlanResampling(externalRate, modelRate, 0);
		const std::vector<float> h = na::ResamplePrototype(p);
		if (buf && capacity > 0) memcpy(buf, h.data(), sizeof(float) * std::min((size_t)capacity, h.size()));
		k = (int)h.size();
	});
	return k;
}

long long NA_ResampleModelFrames(int externalRate, int modelRate, int quantum, long long externalSamples)
{
	long long frames = -1;
	Guard([&] {
		if (externalSamples < 0) throw std::runtime_error("NA_ResampleModelFrames: negative sample count");
		frames = na::PlanResampling(externalRate, modelRate, quantum).ModelFrames(externalSamples);
	});
	return frames;
}

int NA_BatchSetResampling(NA_Batch* batch, int externalRate, int modelRate, int quantum, int maxFrames)
{
	return Guard([&] {
		if (!batch) throw std::runtime_error("NA_BatchSetResampling: null batch");
		batch->batch->SetResampling(externalRate, modelRate, quantum, maxFrames);
	});
}

int NA_BatchGetResampleInfo(NA_Batch* batch, NA_ResampleInfo* info)
{
	return Guard([&] {
		if (!batch || !info) throw std::runtime_error("NA_BatchGetResampleInfo: null argument");
		FillResampleInfo(batch->batch->ResamplingPlan(), info);
	});
}

void NA_SetResampleToExternalRate(NeuralModelLoader* loader, int on)
{
	if (loader) loader->loader->SetResampleToExternalRate(on != 0);
}

int NA_GetProcessLatencySamples(NeuralModel* model)
{
	NeuralAudio::GpuModel* gm = model ? dynamic_cast<NeuralAudio::GpuModel*>(model->model) : nullptr;
	return gm ? gm->GetProcessLatencySamples() : 0;
}

int NA_GetModelProcessRate(NeuralModel* model)
{
	NeuralAudio::GpuModel* gm = model ? dynamic_cast<NeuralAudio::GpuModel*>(model->model) : nullptr;
	return gm ? gm->GetLoadedModel()->ProcessRate() : 0;
}

#ifndef NA_RELEASE
int NA_DebugResampleTap(NA_Batch* batch, float* modelIn, float* modelOut, long long capacityPerRow, int* frames)
{
	return Guard([&] {
		if (!batch) throw std::runtime_error("NA_DebugResampleTap: null batch");
		const int f = batch->batch->DebugResampleTap(modelIn, modelOut, capacityPerRow);
		if (frames) *frames = f;
	});
}
#endif

} // extern "C"
