// gpu_batch.h -- the batched multi-stream engine: owns device state for many independent audio
// streams on ONE GPU and runs the WaveNet / LSTM kernels over them, one launch per model group
// and block of <= 128 frames.
//
// The reference has no counterpart (it processes one stream per NeuralModel instance on the caller's
// thread, NeuralAudio/NeuralModel.h:127); this is the data-parallel axis the GPU path adds.  A
// single-stream NeuralModel (neural_model.cpp) is a GpuBatch with one stream.
#pragma once

#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "cabinet_stage.h"
#include "reverb_stage.h"
#include "compressor_stage.h"
#include "delay_stage.h"
#include "device_resources.h"
#include "eq_stage.h"
#include "gate_stage.h"
#include "host_route.h"
#include "launch_plan.h"
#include "meter_stage.h"
#include "mod_stage.h"
#include "mix_stage.h"
#include "tuner_stage.h"
#include "model_loader.h"
#include "output_stage.h"
#include "resample.h"
#include "tuning.h"
#include "wavenet_launch.h"

namespace na
{
	// Host blocks the caller registered (NA_RegisterHostBuffer: hipHostRegister, mapped): ProcessHost runs the kernels directly on them --
	// no staging copies.  RegisteredDevicePointer: the device address of `p` when [p, p + bytes) lies inside a registered block of
	// `device`'s process, else nullptr.
	bool RegisterHostBuffer(void* p, size_t bytes, std::string& error);
	bool UnregisterHostBuffer(void* p);
	void* RegisteredDevicePointer(const void* p, size_t bytes);

	class HipError : public std::runtime_error
	{
	public:
		HipError(hipError_t e, const char* what) : std::runtime_error(std::string(what) + ": " + hipGetErrorString(e)), code(e) {}
		hipError_t code;
	};

	void CheckHip(hipError_t e, const char* what);

	// returns the number of visible HIP devices (0 when there is no GPU / no driver); never throws
	int VisibleDeviceCount();

	// Relative cost of one stream of a model (what the multi-GPU sharder balances, multi_gpu.h): microseconds per 1024 streams x 128
	// frames of the kernel family that runs it, fitted to the round-3 measurements; host-side only (no device needed)
	double EstimateStreamCost(const LoadedModel& model, float quality);

	// Host-side prediction of the kernel family for a model (no device needed): "f16-split" | "frame" | "generic" | "recurrent", the
	// pack factor, and the static range proof of the f16-split kernels (wavenet_plan.h: splitRangeProven / splitWeightsOk / condLimit)
	struct ModelKernelInfo
	{
		const char* kernel = "";
		int pack = 1;
		float inputLimit = INFINITY;
		bool rangeProven = true, weightsOk = true;
	};
	ModelKernelInfo PredictModelKernel(const LoadedModel& model, float quality, int streams);

	struct CabinetStageInfo
	{
		int maxTaps = 0, ringSamples = 0, pieceSamples = 0, numIRs = 0;
		long long deviceBytes = 0;
	};

	struct ReverbStageInfo
	{
		int maxTaps = 0, partitionSamples = 0, slots = 0, pieceSamples = 0, numIRs = 0;
		long long deviceBytes = 0;
	};

	struct DelayStageInfo
	{
		int maxDelaySamples = 0, ringSamples = 0, pieceSamples = 0, numDelays = 0;
		long long deviceBytes = 0;
	};

	struct CompressorStageInfo
	{
		int curvePoints = 0, numCompressors = 0;
		long long deviceBytes = 0;
	};

	struct ModStageInfo
	{
		int maxDelaySamples = 0, ringSamples = 0, pieceSamples = 0, numMods = 0;
		long long deviceBytes = 0;
	};

	struct GateStageInfo
	{
		int gainSamples = 0, numGates = 0;
		long long deviceBytes = 0;
	};

	struct EqStageInfo
	{
		int maxSections = 0, numEntries = 0;
		long long deviceBytes = 0;
	};

	struct MeterStageInfo
	{
		int numMeters = 0;
		long long deviceBytes = 0;
	};

	struct TunerStageInfo
	{
		int numTuners = 0;
		long long deviceBytes = 0;
	};

	struct MixStageInfo
	{
		int maxMembers = 0, numGroups = 0, drySamples = 0;
		long long deviceBytes = 0;
	};

	class ModelGroup; // one per distinct ModelDesc: packed weights + state of all its streams

	class GpuBatch
	{
	public:
		// throws std::runtime_error if `device` is not a usable HIP device -- there is no CPU fallback
		// `borrowedStream` != nullptr: launch on the caller's HIP stream instead of creating one
		explicit GpuBatch(int device, hipStream_t borrowedStream = nullptr);
		~GpuBatch();

		GpuBatch(const GpuBatch&) = delete;
		GpuBatch& operator=(const GpuBatch&) = delete;

		// Adds a stream running `model`; its row in the [streams][n] input/output arrays is the returned id.
		// For a SlimmableContainer every submodel gets state, `quality` picks the active one.
		// onDemand = ECompositeModelLoadMode::OnDemand (CompositeModel.h:104-109): only the active submodel is prewarmed now, the
		// others when a quality change first selects them.
		int AddStream(const std::shared_ptr<const LoadedModel>& model, float quality, bool prewarm, bool onDemand = false);
		// `count` streams of the same model at once (one state reset / prewarm launch per model group); returns the first id
		int AddStreams(const std::shared_ptr<const LoadedModel>& model, float quality, int count, bool prewarm, bool onDemand = false);

		// Stream lifecycle (the reference's unit of lifetime is the model instance: NeuralAudioCApi.cpp:38-42 DeleteModel, CompositeModel.h:17-23):
		// RemoveStreams frees the state slots of streams [first, first + count) in every model group (also inside packed virtual streams)
		// and retires their ids; the rows keep their place in the [streams][n] arrays (input ignored, host-buffer output zero).  A later
		// AddStreams recycles retired ids -- the lowest retired id for count == 1, a run of `count` consecutive retired ids if there is
		// one -- before it appends new rows, and recycled state slots start from the same fresh / prewarmed state as new ones.
		// Not real-time safe (like AddStreams): call between buffers.
		void RemoveStreams(int first, int count);
		bool IsLive(int stream) const { return stream >= 0 && stream < (int)streams.size() && streams[(size_t)stream].live && !streams[(size_t)stream].parked; }

		// The stream pool: join and leave for a batch that never stops.  ReserveStreams is the set-up side (like AddStreams:
		// not real-time safe): `count` PARKED streams of `model` with everything they will ever need on the device -- rows, state slots of
		// every submodel, list capacity, resampling histories, the chains' streams, the re-arm staging -- each ARMED: in the state
		// AddStreams(count = 1, prewarm) leaves, every submodel prewarmed whatever the load mode.  A parked stream keeps its row (input
		// ignored, host output zero, device output row left alone) and is not live.  ActivateStream / ParkStream are host bookkeeping --
		// a member row, dirty lists, a pending re-arm -- and the processing call that follows enqueues, on the batch stream in front of
		// the model launches, the list upload, one re-arm launch per model group and (resampling) the zeroing of the row's histories: no
		// allocation, no stream or event creation, no host-side wait (a batch on its half-batch chains or the resident launch drains
		// them first, as after SetQuality).  A stream that was parked carries nothing over: it is re-armed before it runs again.
		int ReserveStreams(const std::shared_ptr<const LoadedModel>& model, int count, bool prewarm);
		void ActivateStream(int stream, float quality);
		void ParkStream(int stream); // only streams that came from ReserveStreams; the others leave through RemoveStreams
		bool IsParked(int stream) const { return stream >= 0 && stream < (int)streams.size() && streams[(size_t)stream].parked; }
		int FindParked(const LoadedModel* model) const; // the lowest parked id of that model, -1: none
		int NumParked() const { return numParked; }

		// The output stage (output_stage.h): per-stream ramped output gains and the cross-fade that hands a session from a
		// live stream to a parked one of another model.  EnableOutputStage is the set-up side: the device and pinned tables for the rows
		// the batch has (CreateStreams grows them).  SetStreamGain / Handover are host arithmetic on those tables; while an entry exists --
		// a gain != 1, a running ramp, a fade -- every processing call runs on the ordered path and enqueues, behind the join of its model
		// launches (behind the down kernel of a resampling batch, in front of the device-to-host copy of a host buffer), ONE table upload
		// from a ring of pinned tables and ONE launch that works in place on the rows the caller sees.  Without an entry the batch
		// launches exactly what it launches without the stage.
		void EnableOutputStage();
		bool HasOutputStage() const { return stages[kOutputStage] != nullptr; }
		void SetStreamGain(int stream, float gain, int rampSamples);
		float GetStreamGain(int stream) const; // the target; < 0: not a live or parked stream of the batch
		void Handover(int from, int to, float quality, int fadeSamples);
		int HandoverRemaining(int stream) const;

		// The cabinet stage (cabinet_stage.h): per-stream convolution of the row with an impulse response, behind the
		// model launches (and the down kernel of a resampling batch) and in front of the output stage.  EnableCabinetStage, LoadIR and
		// UnloadIR are the set-up side: a history ring per row (CreateStreams grows them), the tables, the IRs' taps on the device.
		// SetStreamIR is host arithmetic on those tables; while an entry exists -- a stream with an IR, or a fade towards dry -- every
		// processing call runs on the ordered path and enqueues ONE table upload and two launches per piece of kCabPieceSamples samples.
		// Without an entry the batch launches exactly what it launches without the stage.
		void EnableCabinetStage(int maxTaps);
		bool HasCabinetStage() const { return stages[kCabinetStage] != nullptr; }
		CabinetStageInfo GetCabinetInfo() const;
		int LoadIR(const float* taps, int numTaps);
		void UnloadIR(int ir);
		void SetStreamIR(int stream, int ir, int fadeSamples); // ir = -1: dry
		int GetStreamIR(int stream) const;                     // the target
		int StreamIRFadeRemaining(int stream) const;
		// test hook (NA_DebugRunCabinetStage): the stage of a call of n samples on host rows [NumStreams()][stride]; synchronous, set-up side
		void DebugRunCabinetStage(float* hostRows, long stride, size_t n);

		// The reverb stage (reverb_stage.h): per-stream partitioned FFT convolution of the row with a long impulse
		// response (up to kRevMaxTaps taps) and a wet / dry mix, behind the cabinet stage and in front of the output stage.
		// EnableReverbStage, LoadReverbIR and UnloadReverbIR are the set-up side: a sample ring, a ring of input spectra and the tail
		// blocks per row (CreateStreams grows them), the tables, the IRs' head taps and partition spectra on the device (LoadReverbIR
		// computes the spectra there and waits for them, under the wait limit).  SetStreamReverb is host arithmetic on those tables;
		// while an entry exists -- a stream with a reverb, or a fade towards none -- every processing call runs on the ordered path and
		// enqueues ONE table upload and two to four launches per piece of kRevPieceSamples samples.  Without an entry the batch launches
		// exactly what it launches without the stage.
		void EnableReverbStage(int maxTaps);
		bool HasReverbStage() const { return stages[kReverbStage] != nullptr; }
		ReverbStageInfo GetReverbInfo() const;
		int LoadReverbIR(const float* taps, int numTaps);
		void UnloadReverbIR(int ir);
		void SetStreamReverb(int stream, int ir, float wet, float dry, int fadeSamples); // ir = -1: no reverb
		int GetStreamReverb(int stream, float* wet, float* dry) const;                   // the target
		int StreamReverbFadeRemaining(int stream) const;
		// test hook (NA_DebugRunReverbStage): the stage of a call of n samples on host rows [NumStreams()][stride]; synchronous, set-up side
		void DebugRunReverbStage(float* hostRows, long stride, size_t n);

		// The delay stage (delay_stage.h): a per-stream echo -- a feedback delay line of up to kDelayMaxSamples samples with a
		// one-pole low-pass and high-pass in the loop and a wet / dry mix -- behind the cabinet stage and in front of the reverb stage.
		// EnableDelayStage is the set-up side: a ring and a filter state per row (CreateStreams grows them) and the tables.  SetStreamDelay
		// is host arithmetic on those tables; while an entry exists -- a stream with a delay, or a fade towards none -- every processing
		// call runs on the ordered path and enqueues ONE table upload and ONE launch per piece of kDelayPieceSamples samples.  Without an
		// entry the batch launches exactly what it launches without the stage.
		void EnableDelayStage(int maxDelaySamples);
		bool HasDelayStage() const { return stages[kDelayStage] != nullptr; }
		DelayStageInfo GetDelayInfo() const;
		void SetStreamDelay(int stream, const DelayParams* params, int fadeSamples); // nullptr: no delay
		bool GetStreamDelay(int stream, DelayParams& out) const;                     // the target; false: none
		int StreamDelayFadeRemaining(int stream) const;
		// test hook (NA_DebugRunDelayStage): the stage of a call of n samples on host rows [NumStreams()][stride]; synchronous, set-up side
		void DebugRunDelayStage(float* hostRows, long stride, size_t n);

		// The compressor stage (compressor_stage.h): a per-stream feed-forward compressor -- a branching peak follower on the
		// row's own samples, a gain curve of 513 knots read at the follower's level, a multiplication -- behind the cabinet stage and in
		// front of the delay stage.  EnableCompressorStage is the set-up side: two curve slots and a state per row (CreateStreams grows
		// them) and the tables, sized for the curves of both slots of every row.  SetStreamCompressor is host arithmetic on those tables;
		// while an entry exists -- a stream with a compressor, or a fade towards none -- every processing call runs on the ordered path
		// and enqueues ONE table upload and ONE launch, whatever n.  Without an entry the batch launches exactly what it launches without
		// the stage.
		void EnableCompressorStage();
		bool HasCompressorStage() const { return stages[kCompressorStage] != nullptr; }
		CompressorStageInfo GetCompressorInfo() const;
		void SetStreamCompressor(int stream, const CompParams* params, int fadeSamples); // nullptr: no compressor
		bool GetStreamCompressor(int stream, CompParams& out) const;                     // the target; false: none
		int StreamCompressorFadeRemaining(int stream) const;
		float StreamCompressorGain(int stream); // the g of the last sample produced; 1: no compressor.  Synchronises: a diagnostic
		// test hook (NA_DebugRunCompressorStage): the stage of a call of n samples on host rows [NumStreams()][stride]; synchronous, set-up side
		void DebugRunCompressorStage(float* hostRows, long stride, size_t n);

		// The modulation stage (mod_stage.h): per-stream chorus, flanger, vibrato and tremolo -- up to four voices that read a
		// line of up to kModMaxDelaySamples samples at a fractional, LFO-swept delay, a feedback of the first voice, a wet / dry mix and an
		// amplitude modulation -- behind the compressor stage and in front of the delay stage.  EnableModStage is the set-up side: a ring per
		// row (CreateStreams grows them) and the tables.  SetStreamMod is host arithmetic on those tables; while an entry exists -- a stream
		// with a modulation, or a fade towards none -- every processing call runs on the ordered path and enqueues ONE table upload and ONE
		// launch per piece of kModPieceSamples samples.  Without an entry the batch launches exactly what it launches without the stage.
		void EnableModStage(int maxDelaySamples);
		bool HasModStage() const { return stages[kModStage] != nullptr; }
		ModStageInfo GetModInfo() const;
		void SetStreamMod(int stream, const ModParams* params, int fadeSamples); // nullptr: no modulation
		bool GetStreamMod(int stream, ModParams& out) const;                     // the target; false: none
		int StreamModFadeRemaining(int stream) const;
		// test hook (NA_DebugRunModStage): the stage of a call of n samples on host rows [NumStreams()][stride]; synchronous, set-up side
		void DebugRunModStage(float* hostRows, long stride, size_t n);

		// The gate stage (gate_stage.h): a per-stream noise gate that listens to the stream's input row and scales the row
		// the models produced for it -- the detector launch in front of everything of the call, the apply launch first of the stages, in
		// front of the cabinet.  EnableGateStage is the set-up side: a state and a gain row per row (CreateStreams grows them; a call
		// longer than the gain rows grows those first, like any first use of a longer buffer) and the tables.  SetStreamGate is host
		// arithmetic on those tables; while an entry exists -- a stream with a gate, or one whose gate is being taken away -- every
		// processing call runs on the ordered path and enqueues ONE table upload and two launches, whatever n.  Without an entry the
		// batch launches exactly what it launches without the stage.
		void EnableGateStage();
		bool HasGateStage() const { return stages[kGateStage] != nullptr; }
		GateStageInfo GetGateInfo() const;
		void SetStreamGate(int stream, const GateParams* params, bool startOpen); // params == nullptr: the gate goes, click-free
		bool GetStreamGate(int stream, GateParams& out) const;                    // false: no gate (or one that is being taken away)
		float StreamGateGain(int stream); // the g of the last sample produced; synchronises the batch: a diagnostic

		// The EQ stage (eq_stage.h): a cascade of up to 8 biquad sections per stream in f64, applied to the row the models
		// produced behind the gate's apply and in front of the cabinet.  EnableEqStage is the set-up side: two slots of coefficients and
		// section states per row (CreateStreams grows them) and the tables.  SetStreamEq is host arithmetic on those tables; while an
		// entry exists -- a stream with a cascade, or one that fades to flat -- every processing call runs on the ordered path and
		// enqueues ONE table upload and ONE launch, whatever n.  Without an entry the batch launches exactly what it launches without
		// the stage.
		void EnableEqStage();
		bool HasEqStage() const { return stages[kEqStage] != nullptr; }
		EqStageInfo GetEqInfo() const;
		void SetStreamEq(int stream, const EqSection* sections, int numSections, int fadeSamples); // 0 sections: flat
		int GetStreamEq(int stream, EqSection* out, int capacity) const;                           // the target's section count
		int StreamEqFadeRemaining(int stream) const;
		// test hook (NA_DebugRunEqStage): the stage of a call of n samples on host rows [NumStreams()][stride]; synchronous, set-up side
		void DebugRunEqStage(float* hostRows, long stride, size_t n);

		// The meter stage (meter_stage.h): per-stream level meters on the input row (the IN tap, in front of the model
		// launches) and on the row the caller receives (the OUT tap, behind the output stage), and a gain-reduction meter on the gate's gain
		// of the same samples (the GATE tap).  It never writes an audio row.  EnableMeterStage is the set-up side: a state per row
		// (CreateStreams grows them), the tables and a result block per table.  SetStreamMeter is host arithmetic on those tables; while
		// an entry exists every processing call runs on the ordered path and enqueues ONE table upload, two launches and ONE result copy,
		// whatever n.  ReadStreamMeter never waits: it queries the ring's events and returns the newest reading that has arrived.
		// Without an entry the batch launches exactly what it launches without the stage.
		void EnableMeterStage();
		bool HasMeterStage() const { return stages[kMeterStage] != nullptr; }
		MeterStageInfo GetMeterInfo() const;
		void SetStreamMeter(int stream, const MeterParams* params); // params == nullptr: the meter goes at once
		bool GetStreamMeter(int stream, MeterParams& out) const;    // false: no meter
		bool ReadStreamMeter(int stream, MeterReading& out);        // false: no meter, or no completed window has arrived yet

		// The tuner stage (tuner_stage.h): a per-stream pitch reading of the input row -- an integer autocorrelation of the
		// decimated, quantised row every hopSamples, exact whatever the cut into calls -- behind the meter's IN tap in front of the model
		// launches.  It never writes an audio row.  EnableTunerStage is the set-up side: an open group and a ring of decimated samples per
		// row (CreateStreams grows them), the tables and a result block per table.  SetStreamTuner is host arithmetic on those tables;
		// while an entry exists every processing call runs on the ordered path and enqueues ONE table upload and ONE append launch per
		// piece of kTunerPieceSamples samples, and a call that holds an evaluation end of an entry ONE evaluate launch and ONE result
		// copy more.  ReadStreamTuner never waits: it queries the ring's events and returns the newest reading that has arrived.
		// Without an entry the batch launches exactly what it launches without the stage.
		void EnableTunerStage();
		bool HasTunerStage() const { return stages[kTunerStage] != nullptr; }
		TunerStageInfo GetTunerInfo() const;
		void SetStreamTuner(int stream, const TunerParams* params); // params == nullptr: the tuner goes at once
		bool GetStreamTuner(int stream, TunerParams& out) const;    // false: no tuner
		bool ReadStreamTuner(int stream, TunerReading& out);        // false: no tuner, or no evaluation has arrived yet

		// The mix stage (mix_stage.h): per-session mix groups -- the rows of up to 8 members (a stream's row as the output
		// stage left it, or the input row the caller passed for it) summed through a ramped D x M gain matrix into the rows of the first
		// D members -- behind the output stage and in front of the meter's OUT tap: the one stage in which rows meet.  EnableMixStage is
		// the set-up side: a block of two matrices and a row for stashed input per row (CreateStreams grows them; a call with a DRY
		// member longer than the stash rows grows those first, like any first use of a longer buffer) and the tables.  SetMixGroup /
		// ClearMixGroup are host arithmetic on those tables; while a group exists every processing call runs on the ordered path and
		// enqueues ONE table upload and ONE launch, whatever n and however many groups, and ONE stash launch in front of the models
		// while some group has a DRY member.  Without a group the batch launches exactly what it launches without the stage.
		void EnableMixStage();
		bool HasMixStage() const { return stages[kMixStage] != nullptr; }
		MixStageInfo GetMixInfo() const;
		void SetMixGroup(const int* streamIds, const int* taps, int numMembers, int numOutputs, const float* gains, int rampSamples); // taps == nullptr: all OUT
		void ClearMixGroup(int stream); // the group that names `stream` goes at once; none: nothing happens
		int GetStreamMix(int stream, int* streamIds, int* taps, int capacity, int* numOutputs, float* gains) const; // M; 0: no group
		int MixRampRemaining(int stream) const;
		bool HasDryMixGroup() const;
		// test hook (NA_DebugRunMixStage): the stage of a call of n samples on host rows [NumStreams()][stride], hostIn the input rows of
		// the same shape (may be nullptr when no group has a DRY member); synchronous, set-up side
		void DebugRunMixStage(const float* hostIn, float* hostRows, long stride, size_t n);

		// Stream snapshots (stream_snapshot.h): a stream's state as a relocatable blob -- it loads into any stream of the
		// same model file in any batch, device, process or kernel family.  SaveStreams writes the blobs of ids[0 .. count) back to back
		// into `buf` and returns their total size; with `capacity` short of it nothing is written (the caller sizes the buffer from the
		// return value).  LoadStreams reads blob i into stream ids[i]: every blob is checked against its destination's model before
		// anything is written (all or nothing; throws naming the reason); the stream takes over quality, active submodel, prewarmed
		// bits and the state of every submodel, and keeps its own load mode.  Both settle the batch first like RemoveStreams (resident
		// launch, half-batch chains, pipeline tickets, batch stream): not real-time safe, call between buffers.  One export / import
		// launch per model group and one device <-> host copy per call, whatever `count`.  SaveStreams changes nothing on the device.
		size_t StreamSnapshotBytes(int stream) const;
		size_t SaveStreams(const int* ids, int count, void* buf, size_t capacity);
		void LoadStreams(const int* ids, int count, const void* buf, size_t bytes);

		// Batch resampling (resample.h): a set-up call before the first AddStreams.  From then on every `n` of the processing
		// entry points counts EXTERNAL samples per row: an up kernel turns them into model frames (whole multiples of the block quantum, the
		// rest waits), the model runs on them through the ordinary launches, a down kernel produces the n output samples -- all on the
		// batch stream, in that order (no half-batch chains, no resident launch).  The output is the pipeline's answer delayed by a fixed
		// whole number of external samples (ResamplingPlan().latency) and does not depend on how the signal is cut into calls.
		// externalRate == modelRate: accepted, nothing changes.  AddStreams then refuses models whose model-side rate is not modelRate.
		void SetResampling(int externalRate, int modelRate, int quantum, int maxFrames);
		bool HasResamplingPlan() const { return resample != nullptr; }
		bool Resamples() const; // a plan with different rates is in effect
		const ResamplePlan& ResamplingPlan() const;
		long long ResampleSamplesTaken() const; // external samples the batch has taken so far (its phase); -1 without a plan
		// test hook (NA_DebugResampleTap): the model-rate input / output rows [streams][frames] of the last processing call (of its last
		// piece, where a call longer than 2048 external samples ran in several); synchronises
		int DebugResampleTap(float* modelIn, float* modelOut, long long capacityPerRow);

		int NumStreams() const { return (int)streams.size(); } // rows of the [streams][n] arrays (retired ids included)
		int NumLiveStreams() const { return (int)streams.size() - (int)retired.size() - numParked; }
		unsigned StreamPrewarmedMask(int stream) const; // bit k: submodel k of the stream had its prewarm

		// ScalableCompositeModel::SetQualityScaleFactor (CompositeModel.h:176-181): switches the active submodel,
		// the inactive one keeps its state untouched.
		void SetQuality(int stream, float quality);
		// CompositeModel::IsModelChangeRealtimeSafe (CompositeModel.h:44-50) for this engine: false when the switch would prewarm a
		// submodel (OnDemand) or force a hipGraph re-capture; true when it only re-uploads the pinned index lists asynchronously
		bool IsQualityChangeRealtimeSafe(int stream, float quality) const;
		float GetQuality(int stream) const;
		int GetActiveSubModel(int stream) const;

		// Re-establish the zero-input steady state of every submodel of `stream` (NeuralModel::Prewarm)
		void Prewarm(int stream);

		// in/out are DEVICE pointers, row s = stream s, `n` samples per row, rows `stride` floats apart.
		// Asynchronous on GetStream(). in == out is allowed.
		void ProcessDevice(const float* dIn, float* dOut, size_t n, long inStride, long outStride);

		// in/out are HOST pointers laid out [streams][n]; stages through pinned buffers; synchronous.
		void ProcessHost(const float* in, float* out, size_t n);
		// `in`: HOST rows [streams][n] (staged through the pinned block); `dOut`: DEVICE rows, `outStride` floats apart.  Asynchronous on
		// GetStream() once the input is staged -- the multi-GPU host's RCCL fan-in gathers the shards' device rows (multi_gpu.cpp).
		void ProcessHostToDevice(const float* in, float* dOut, size_t n, long outStride);
		// device copies of a model's weight tables (every group of the batch that runs one of `model`'s submodels, in submodel order):
		// what the multi-GPU host replicates from the first device that holds the model (RCCL fan-out)
		void WeightImages(const LoadedModel& model, std::vector<std::pair<void*, size_t>>& out) const;
		// Weight fan-out (multi-GPU host): while SetPeerWeights(true), a model group created by AddStreams allocates its weight images
		// without uploading them -- a peer device that holds the model sends them -- and the prewarm of its streams waits; WeightsArrived()
		// says the images are in place (on this batch's stream): device-side derivations and the deferred prewarms run, the mode ends.
		// Processing before WeightsArrived() is an error of the caller.
		void SetPeerWeights(bool on) { peerWeights = on; }
		bool AwaitsWeights() const { return !awaitingWeights.empty(); }
		void WeightsArrived();

		// Pipelined host-buffer interface: Submit() copies `in` ([streams][n], host) into a pinned slot and enqueues H2D (copy-in
		// stream), the kernels (batch stream) and D2H (copy-out stream); Collect() waits for that slot and copies the result out.
		// With two slots in flight the upload of buffer k+1 and the download of buffer k-1 overlap the kernels of buffer k.
		// Buffers are processed strictly in submission order (the streams' state depends on it).
		static constexpr int kPipelineSlots = 3;
		int Submit(const float* in, size_t n);       // returns a ticket; throws if all slots are in flight
		void Collect(int ticket, float* out);        // blocks until that buffer is done
		// Zero-copy variants: the caller writes the next buffer straight into the pinned staging memory the upload reads
		// (NextInput, then Submit(nullptr, n)) and reads results in place (Collect(ticket, nullptr), then OutputView: valid until
		// that slot is submitted again, kPipelineSlots submissions later).
		float* NextInput(size_t n);
		const float* OutputView(int ticket) const;
		size_t SlotFrames(int ticket) const { return (ticket >= 0 && ticket < kPipelineSlots) ? pipe[ticket].n : 0; } // frames per row of that submission
		size_t SlotRows(int ticket) const { return (ticket >= 0 && ticket < kPipelineSlots) ? pipe[ticket].rows : 0; } // rows of that submission

		// ---- bounded waits ------------------------------------------------------------------------------------------------------------
		// Process is called from a real-time thread that must get its call back (NeuralAudio/NeuralModel.h:127, README "one thread per
		// model"): every host-side wait of the processing paths -- stream and event waits, the polls of the resident launch's counters,
		// the timing marks -- has a wall-clock limit (default 2000 ms: NA_WAIT_LIMIT_MS; <= 0: none).  A wait that runs into it marks the
		// batch BROKEN and throws: the call returns (the C ABI: non-zero, NA_GetLastError(), output rows zeroed), and every later call on
		// the batch fails at once without touching the device -- the stream states are no longer what the caller thinks they are.  A
		// broken batch can only be destroyed; its destructor gives the device one more limit to come back and otherwise leaves the
		// device allocations alone (a kernel may still be writing them) instead of hanging in hipFree.
		void SetWaitLimitMs(double ms) { waitLimitMs = ms; }
		double GetWaitLimitMs() const { return waitLimitMs; }
		bool IsBroken() const { return broken; }
		const std::string& BrokenReason() const { return brokenWhy; }
		void WaitStreamBounded(hipStream_t s, const char* what); // hipStreamSynchronize with the limit
		void WaitEventBounded(hipEvent_t e, const char* what);   // hipEventSynchronize with the limit
		// test hook (NA_DebugStallDevice): a kernel that keeps the batch stream busy for `ms` milliseconds (at most 10 s), behind whatever
		// the stream holds -- a wedged device as far as every wait on this batch can tell
		void DebugStallDevice(double ms);
		// test hook (NA_DebugLastHostRoute): the HostRoute (host_route.h) the last processing call took, -1 before any
		int DebugLastHostRoute() const { return lastRoute; }

		void Synchronize();
		// every buffer handed to ProcessDevice so far has been processed (host-side wait).  Unlike Synchronize() it leaves the resident
		// launch on the chip; on a caller's / observed stream it is a synchronisation of that stream.
		void WaitOutputs();
		// Timing marks for bench.py (HIP events on EVERY stream this batch launches kernels on -- the batch stream and the two half-batch
		// streams): MarkTime(0) ... launches ... MarkTime(1); ElapsedMs() = the longest mark-to-mark span over those streams (after a
		// Synchronize()).  The caller's own events only see the stream it handed in.
		bool UsesHalfLaunches() const { return lastStepHalves; }
		// Opt-in (default: Tuning residentOn = NA_RESIDENT=1): large A1 Standard batches on the batch's own stream run as commands to ONE
		// launch that stays on the chip (gpu_batch_chains.cpp) instead of two free-running half-batch launches per buffer.
		void SetResidentLaunch(bool on);
		bool UsesResidentLaunch() const { return lastStepResident; } // the last device-pointer buffer went through the resident launch
		void MarkTime(int which);
		void WaitMarks(); // polls until the marks of MarkTime(1) are reached on every stream
		float ElapsedMs();
		// The batch's HIP stream.  Handing it out makes the batch order every launch on it from then on: until then a batch that created
		// its own stream may run a buffer as two free-running half-batch launches on internal streams (see halfStream below) -- nobody
		// outside can observe the order of work on a stream they never saw; NA_BatchSynchronize / the host-buffer entry points wait for all.
		hipStream_t GetStream();
		int GetDevice() const { return device; }

		// roofline bookkeeping for bench.py: stream-weighted algorithmic bytes / MACs per sample
		double AlgorithmicBytesPerSample(int blockFrames) const;
		double MacsPerSample() const;
		size_t StateBytes() const;
		const char* StreamKernelName(int stream) const; // which kernel runs the stream (rocprof name without template arguments)
		// range contract: samples beyond +-limit are clamped (NaN reads as silence) by the kernel that runs the stream; +inf for the f32 kernels
		float StreamInputLimit(int stream) const;
		// f16-split kernels on a model without a static range proof (the official A2 shapes): how often a value of the stream left the f16
		// range and was saturated -- (wave, block) pairs since the stream's last reset / prewarm; 0 means the output is the reference's to
		// the usual tolerance.  Synchronises the batch stream (a diagnostic, not for the audio path).
		int StreamRangeEvents(int stream);
		int StreamPackFactor(int stream) const; // > 1: the stream shares a kernel-level stream with others of its model (stream packing)

	private:
		struct StreamRef
		{
			std::shared_ptr<const LoadedModel> model;
			std::vector<std::pair<ModelGroup*, int>> members; // per submodel: (group, member index)
			int active = 0;
			float quality = 1.0f;
			bool onDemand = false;
			bool live = true;
			// the pool: `pooled` came from ReserveStreams; `parked` holds state slots but no member is active; `used` has run (or may have)
			// since it was last armed; `poolPrewarm` is the doPrewarm it was reserved with
			bool pooled = false, parked = false, used = false, poolPrewarm = false;
			std::vector<char> prewarmed; // per submodel: had its initial prewarm
		};
		std::vector<int> retired; // sorted ids of removed streams
		int numParked = 0;
		bool rearmPending = false;           // a group has members queued for re-arm / rows wait for zero histories: FlushRearms
		std::vector<int> pendingHistoryZero; // resampling batch: rows activated since the last processing call
		int CreateStreams(const std::shared_ptr<const LoadedModel>& model, float quality, int count, bool prewarm, bool onDemand, bool pool);
		void FlushRearms(); // top of every processing entry point, outside any graph capture
		// The per-stream stages.  StageId is THE place that states the chain: a processing call runs the stages with
		// entries in this order, and what the batch does for every stage is a loop over `stages` (null until the stage's Enable call).
		enum StageId { kGateStage, kEqStage, kCabinetStage, kCompressorStage, kModStage, kDelayStage, kReverbStage, kOutputStage, kMixStage, kMeterStage, kTunerStage, kNumStages };
		struct Stage // what the batch needs from any stage (the stages: gpu_batch_internal.h)
		{
			virtual ~Stage() = default;
			virtual bool HasEntries() const = 0;
			virtual void EnsureRows(GpuBatch& batch, int rows) = 0; // set-up side: device blocks and tables for `rows` rows
			virtual void Leave(int stream) = 0;                     // park / removal: nothing of the stream is carried over
			// a call with entries: in front of its model launches (the gate's detector, the mix stage's stash, the meter's IN tap, the tuner), and behind them in chain order
			virtual void BeforeModels(GpuBatch&, hipStream_t, const float*, size_t, long) {}
			virtual void Run(GpuBatch& batch, hipStream_t launch, float* dOut, size_t n, long outStride) = 0;
		};
		template <class Book, class Entry> struct StageOf;
		template <class Record> struct StageResults; // the result blocks of the stages that report to the host (meter, tuner)
		struct GateStage; struct EqStage; struct CabinetStage; struct CompressorStage; struct ModStage; struct DelayStage; struct ReverbStage; struct OutputStage; struct MixStage; struct MeterStage; struct TunerStage;
		std::unique_ptr<Stage> stages[kNumStages];
		template <class S> S& Require(const char* who) const;             // throws "<who>: <stage> not enabled (...)"
		template <class S> S& EnableStage();                              // every Enable*Stage call
		template <class S> S& SettableStage(int stream, const char* who); // a set call's preamble: usable, enabled, not parked, live
		void DebugRunStage(Stage& stage, const char* who, float* hostRows, long stride, size_t n, const float* hostIn = nullptr);
		bool StageHasEntries() const; // of any stage
		// the call runs ordered on ONE stream: up kernel -> model launches -> down kernel of a resampling batch, the stages behind the
		// model launches (no half-batch chains, no resident launch)
		bool RunsOrdered() const { return Resamples() || StageHasEntries(); }
		void RequireRow(int stream, const char* who) const; // throws "<who>: stream <s> is not a stream of the batch" (a parked one is)
		void StageParkFinished();        // top of every processing call: the `from` streams of the fades that ended in the last one are parked
		void StageLeave(int stream);     // park / removal: every stage lets go of it
		int AllocateIds(int count);
		void DropTrailingRetiredRows();
		// the kinds of the groups that have active streams once `leaving` has lost / `entering` has gained one, in group order (`active`:
		// those groups)
		std::vector<LaunchKind> ActiveKinds(const ModelGroup* leaving, const ModelGroup* entering, std::vector<ModelGroup*>* active = nullptr) const;
		void ZeroRetiredRows(float* hostRows, size_t n, size_t rows) const;

		ModelGroup* GroupFor(const std::shared_ptr<const ModelDesc>& desc, int packHint = 0);
		void EnsureStaging(size_t floats);

		int device;
		hipStream_t stream = nullptr;
		bool ownsStream = true;
		double waitLimitMs = DefaultWaitLimitMs();
		bool broken = false;
		std::string brokenWhy;
		static double DefaultWaitLimitMs();
		void CheckUsable() const; // throws when the batch is broken
		[[noreturn]] void Stall(const char* what);
		// a deadline of the current wait limit; Expired() is cheap enough for every turn of a poll loop
		struct Deadline
		{
			std::chrono::steady_clock::time_point end;
			bool limited;
			explicit Deadline(double ms) : end(std::chrono::steady_clock::now() + std::chrono::microseconds((long long)(ms > 0 ? ms * 1000.0 : 0))), limited(ms > 0) {}
			bool Expired() const { return limited && std::chrono::steady_clock::now() > end; }
		};
		hipEvent_t forkEvent = nullptr;

		// cached hipGraph of the multi-group fork/launch/join sequence (gpu_batch.cpp ReplayUnitsGraph)
		struct GraphKey
		{
			const float* dIn;
			float* dOut;
			size_t n;
			long inStride, outStride;
			unsigned long version;
		};
		struct GraphEntry
		{
			GraphKey key;
			hipGraphExec_t exec;
		};
		std::vector<GraphEntry> graphCache; // a handful of call signatures (hosts cycle through a few fixed buffers)
		unsigned long topologyVersion = 0;
		// the launch units of a buffer (launch_plan.h), planned again when the topology -- which groups have active streams -- changes
		struct
		{
			unsigned long version = ~0ul;
			std::vector<ModelGroup*> groups; // the groups with active streams, in group order: what the units' indices point at
			std::vector<LaunchUnit> units;
		} plan;
		void UpdatePlan();
		std::vector<WnFrameGroup> WaveNetArgs(const LaunchUnit& unit, bool groupOrder); // the arguments of a frame / split / packed unit's launch
		std::vector<std::unique_ptr<ModelGroup>> groups;
		std::vector<StreamRef> streams;
		bool peerWeights = false;
		std::vector<ModelGroup*> awaitingWeights;
		std::vector<std::pair<ModelGroup*, std::vector<int>>> pendingPrewarm;

		// snapshot staging (SaveStreams / LoadStreams): pinned host + device, 32-bit words, grown on demand
		uint32_t* snapHost = nullptr;
		uint32_t* snapDev = nullptr;
		size_t snapWords = 0;
		void EnsureSnapshotStaging(size_t words);
		void SettleForSnapshot(const int* ids, int count, const char* who);
		std::vector<std::pair<std::shared_ptr<const LoadedModel>, uint64_t>> fingerprints; // of the models of this batch's streams, computed once each
		uint64_t FingerprintOf(const std::shared_ptr<const LoadedModel>& model);

		float* hostStage = nullptr; // pinned
		float* devStage = nullptr;
		size_t stageFloats = 0;

		static constexpr int kMaxChains = 4;
		struct PipeSlot
		{
			float* hostIn = nullptr;  // pinned
			float* hostOut = nullptr; // pinned
			float* dev = nullptr;
			size_t floats = 0, n = 0;
			size_t rows = 0; // rows of the [streams][n] block this slot was submitted with
			std::vector<int> parkedRows; // ... and the rows that were parked then (host output zero)
			hipEvent_t uploaded = nullptr, computed = nullptr, downloaded = nullptr;
			hipStream_t own = nullptr; // upload, kernel and download of this slot's buffer, in order (batches that run as one launch)
			hipEvent_t halfDone[kMaxChains] = {}; // free-running half-batch chains (Submit): this buffer's kernel of each chain
			SlotWait wait = SlotWait::DownloadedEvent; // what Collect waits for: the route the ticket took (host_route.h)
			bool busy = false;
		};
		void DrainPipeline();
		// Two free-running chains: a batch whose active streams all run on the f16-split WaveNet kernels as ONE launch per buffer (one
		// model, or a mixed / packed batch that shares a fused launch; >= 512 kernel-level streams) can run a buffer as two launches of half
		// of every group's streams, each half on its own HIP stream, in submission order -- the halves never wait for each other (streams
		// are independent), so the tail of one launch overlaps the other half's work: 40.1 -> 37.4 us per 1024 x 128 buffer of kernel
		// time (tools/split_launch_probe2.py).  A call ordered on ONE stream cannot do this (it would have to join the halves every
		// call: 65.9 us); Submit / Collect can (Collect waits for both halves of its ticket), and so can NA_BatchProcessDevice on a batch
		// whose stream nobody else has seen.
		hipStream_t halfStream[kMaxChains] = {};
		int numChains = 2; // (tuning knob NA_HOST_CHAINS: 2 .. kMaxChains parts instead of halves)
		bool markOpen = false; // between MarkTime(0) and MarkTime(1): a chain stream created now gets its start mark right away
		bool lastStepHalves = false; // the last device-pointer / submitted buffer ran as two half-batch launches
		bool streamObserved = false; // GetStream() was called (or the stream is the caller's): launches are ordered on `stream`
		// The resident launch (gpu_batch_chains.cpp): one launch that stays on the chip and walks consecutive buffers, fed through a command
		// ring in pinned host memory -- for the batches the chains serve whose buffer is one launch of 128-frame A1 Standard blocks
		struct ResidentState;
		std::unique_ptr<ResidentState> residentState;
		std::vector<WaveNetGroupFacts> wnFacts; // scratch of LaunchWaveNetList: the facts of a list longer than a launch's kernarg segment (no allocation per buffer)
		WnLaunchTable wnTable[4]; // device tables of launch lists with more groups than a launch's kernarg segment holds (gpu_batch.cpp LaunchWaveNetList), by LaunchKind
		bool lastStepResident = false;
		bool residentWanted = Tuning::Get().residentOn;
		bool TryResident(const float* dIn, float* dOut, size_t n, long inStride, long outStride);
		bool ResidentConfigure();
		void ResidentEnsureRunning();
		void ResidentExitAfterPosted();
		void ResidentFinishMarked();
		void DrainResident(); // every posted command has run, the launch is gone (called by everything that touches state or the batch stream)
		// nothing of this batch is in flight anywhere: resident launch, half-batch chains, pipeline slots, the batch stream
		void Quiesce();
		struct HalfLists; // the two launch lists of the buffer (gpu_batch.cpp)
		std::unique_ptr<HalfLists> halfLists;
		bool PrepareHalves(size_t n);
		void ProcessDeviceOrdered(const float* dIn, float* dOut, size_t n, long inStride, long outStride);
		void BeginHalves();
		void LaunchChain(int h, const float* dIn, float* dOut, size_t n, long inStride, long outStride, bool hostRows);
		void LaunchHalves(const float* dIn, float* dOut, size_t n, long inStride, long outStride, hipEvent_t* done, bool hostRows);
		void JoinHalves(); // the half-batch chains are done (host-side wait); the next launches go to the batch stream again
		hipEvent_t marks[1 + kMaxChains][2] = {};
		// One processing call on `launch`, the one place that states its order (gpu_batch.cpp): the stages' BeforeModels,
		// ProcessResampledOn or LaunchModelsOn, then RunStages
		void ProcessDeviceOn(hipStream_t launch, const float* dIn, float* dOut, size_t n, long inStride, long outStride);
		void RunStages(hipStream_t launch, float* dOut, size_t n, long outStride); // the stages with entries, in StageId order
		// the model launches of a call, and their parts (gpu_batch.cpp)
		struct ModelCall; // (gpu_batch_internal.h)
		void LaunchModelsOn(hipStream_t launch, const float* dIn, float* dOut, size_t n, long inStride, long outStride);
		void LaunchWaveNetList(const ModelCall& c, LaunchKind which, const std::vector<WnFrameGroup>& list, hipStream_t s, bool prepareOnly);
		void LaunchRecurrentUnit(const ModelCall& c, hipStream_t s, bool prepareOnly);
		void RunUnit(const ModelCall& c, size_t u, hipStream_t s, bool prepareOnly);
		void ForkJoinUnits(const ModelCall& c);
		void ReplayUnitsGraph(const ModelCall& c);
		struct ResampleState; // (gpu_batch_internal.h)
		std::unique_ptr<ResampleState> resample;
		void ProcessResampledOn(hipStream_t launch, const float* dIn, float* dOut, size_t n, long inStride, long outStride);
		void EnsureResampleRows(int rows);           // set-up side only (AddStreams): histories and model-side rows for `rows` rows
		void EnsureResampleFrames(size_t n);         // model-side buffers for pieces of n external samples
		void ZeroResampleHistories(int first, int count);
		// set-up side: a zeroed [rows][rowFloats] block in place of `block`, the first `keepRows` rows copied over (resample.cpp)
		void GrowRowBlock(float*& block, size_t rowFloats, int keepRows, int rows, const char* mallocWhat, const char* what);
		// what is in flight where -- the ordering between the batch stream, the slot streams and the chain streams: the stream state makes
		// every kernel launch depend on the previous one
		struct InFlight; // (gpu_batch_internal.h)
		std::unique_ptr<InFlight> inFlight;
		void WaitChains(); // every chain stream is idle (host-side wait)
		int lastRoute = -1; // HostRoute of the last processing call (NA_DebugLastHostRoute)
		PipeSlot pipe[kPipelineSlots];
		hipStream_t copyIn = nullptr, copyOut = nullptr;
		int nextSlot = 0;
		bool EnsureSlotEvents(PipeSlot& s); // the slot's three events; true: created now
		void EnsurePipeSlot(PipeSlot& s, size_t floats);
		void EnsurePoolPipeline(); // ReserveStreams: what Submit / Collect would create on first use, whatever the number of launch units
	};
}
