// gpu_batch_internal.h -- declarations shared by the translation units of class GpuBatch (gpu_batch.cpp: lifecycle and launch
// dispatch; gpu_batch_chains.cpp: half-batch chains, resident launch, timing marks; gpu_batch_host.cpp: host-buffer entry points; gpu_batch_snapshot.cpp: stream snapshots)
#pragma once

#include "gpu_groups.h"
#include "resample.h"

namespace na
{
	struct GpuBatch::HalfLists
	{
		std::vector<WnFrameGroup> part[GpuBatch::kMaxChains];
		bool listsUploaded = false; // an index list went to the device on the batch stream while the lists were built
		bool compact = false;       // some group has compact rings: chunk lengths of WnCompactSafeFrames() only
		// every part is a contiguous range of rows (no index lists, no packed streams): the host can stage and collect a half by itself
		bool RowRangesOnly() const
		{
			for (const auto& list : part)
				for (const WnFrameGroup& g : list)
					if (g.slots != nullptr || g.pack > 1) return false;
			return true;
		}
	};

	// the resident launch of a batch (gpu_batch_chains.cpp): command ring, counters, the launch list it was started with
	struct GpuBatch::ResidentState
	{
		// host -> device words: fine-grained device memory written by the host through the BAR (one address for both sides); without a
		// large BAR a pinned, coherent host block (`ctrl` its host address, `dCtrl` its device address: the workgroups then poll over PCIe)
		ResidentCtrl* ctrl = nullptr;
		ResidentCtrl* dCtrl = nullptr;
		bool ctrlInDeviceMemory = false;
		ResidentStatus* status = nullptr;  // device -> host word: pinned, coherent host block ...
		ResidentStatus* dStatus = nullptr; // ... and its device address
		unsigned* dDone = nullptr;     // [RESIDENT_RING]
		unsigned* dWgDone = nullptr;   // [wgCapacity]
		int wgCapacity = 0;
		std::vector<WnFrameGroup> list;
		bool configured = false;       // `list` is the launch list of topology `topology`, its index lists are on the device
		bool unsupported = false;      // ... or that topology cannot run resident
		unsigned long topology = ~0ul;
		unsigned long long posted = 0; // sequence number of the last command posted
		unsigned long long base = 0;   // ... of the last command before this generation of launches (all of them done, wgDone zero)
		unsigned long long markPosted = 0; // `posted` at the closing timing mark
		bool launched = false;         // a launch of this generation is (or was) on the stream: `gen` is recorded behind it
		bool exitRequested = false;    // exitAfter was set without waiting (closing timing mark): the next command starts a new generation
		hipEvent_t gen = nullptr;
		int grid = 0;
		~ResidentState()
		{
			if (gen) (void)hipEventDestroy(gen);
			if (dDone) (void)CountedHipFree(dDone);
			if (dWgDone) (void)CountedHipFree(dWgDone);
			if (ctrl) (void)(ctrlInDeviceMemory ? CountedHipFree(ctrl) : CountedHipHostFree(ctrl));
			if (status) (void)CountedHipHostFree(status);
		}
	};

	// the model launches of one call (GpuBatch::LaunchModelsOn): its signature and the arguments gathered for the plan's launch units
	struct GpuBatch::ModelCall
	{
		const float* dIn;
		float* dOut;
		size_t n;
		long inStride, outStride;
		std::vector<std::vector<WnFrameGroup>> wnArgs; // per unit: the groups of a frame / split / packed unit
		std::vector<RecurrentGroup> recArgs;           // the groups of the recurrent unit
	};

	// a resampling batch (resample.cpp): the plan, the batch's counters, the coefficient tables, the per-row histories
	// and the fixed model-side buffers
	struct GpuBatch::ResampleState
	{
		ResamplePlan plan;
		long long E = 0, P = 0;    // external samples taken / model frames run so far: the batch's, not the streams'
		float* tableUp = nullptr;   // [te][tapsUp]
		float* tableDown = nullptr; // [tm][tapsDown]
		float* histUp = nullptr;    // [rowCapacity][plan.histUp]
		float* histDown = nullptr;  // [rowCapacity][plan.histDown]
		float* modelIn = nullptr;   // [rowCapacity][modelStride]
		float* modelOut = nullptr;
		int rowCapacity = 0;
		int pieceFrames = 0;        // a longer call runs in pieces of this many external samples (the LDS window of the stages)
		int sizedFrames = 0;        // external samples per piece the model-side buffers hold
		int modelStride = 0;
		int lastFrames = 0, lastRows = 0; // NA_DebugResampleTap: model frames and rows of the last piece
		~ResampleState()
		{
			for (float* p : { tableUp, tableDown, histUp, histDown, modelIn, modelOut })
				if (p) (void)CountedHipFree(p);
		}
	};

	// The ring of entry tables of a per-stream stage (output_stage.cpp, cabinet_stage.cpp): pinned and device blocks of `capacity` entries
	// and an event each.  One table more than buffers can be in flight (Submit): the table a call takes was read by a launch whose
	// ticket has been collected.  `inFlight` names the stage in the message of a wait that ran into the limit.
	template <class Entry>
	struct StageTables
	{
		static constexpr int kTables = GpuBatch::kPipelineSlots + 1;
		const char* inFlight;
		Entry* host[kTables] = {};     // pinned
		Entry* dev[kTables] = {};
		hipEvent_t done[kTables] = {}; // the launches that read dev[i] (and the upload that read host[i]) are over
		bool used[kTables] = {};
		int next = 0;
		int capacity = 0;              // entries per table
		explicit StageTables(const char* what) : inFlight(what) {}
		~StageTables()
		{
			for (int i = 0; i < kTables; i++)
			{
				if (host[i]) (void)CountedHipHostFree(host[i]);
				if (dev[i]) (void)CountedHipFree(dev[i]);
				if (done[i]) (void)hipEventDestroy(done[i]);
			}
		}
		// set-up side: the events, and tables of at least `want` entries (the launches that read the old ones are over before they go)
		void Ensure(GpuBatch& batch, int want)
		{
			for (hipEvent_t& e : done)
				if (!e) CheckHip(CountedHipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
			if (want <= capacity) return;
			for (int i = 0; i < kTables; i++)
			{
				if (used[i]) batch.WaitEventBounded(done[i], inFlight);
				used[i] = false;
				if (host[i]) (void)CountedHipHostFree(host[i]);
				if (dev[i]) (void)CountedHipFree(dev[i]);
				host[i] = dev[i] = nullptr;
			}
			capacity = 0;
			for (int i = 0; i < kTables; i++)
			{
				CheckHip(CountedHipHostMalloc(reinterpret_cast<void**>(&host[i]), (size_t)want * sizeof(Entry), hipHostMallocDefault), "hipHostMalloc");
				CheckHip(CountedHipMalloc(reinterpret_cast<void**>(&dev[i]), (size_t)want * sizeof(Entry)), "hipMalloc");
			}
			capacity = want;
		}
		// the next table, pinned block and device twin, once the launch that last read it is over (a bounded wait)
		struct Table
		{
			Entry *host, *dev;
		};
		Table Take(GpuBatch& batch)
		{
			if (used[next]) batch.WaitEventBounded(done[next], inFlight);
			return { host[next], dev[next] };
		}
		// behind the upload and the launches that read the table taken: the ring moves on
		void Commit(hipStream_t stream)
		{
			CheckHip(hipEventRecord(done[next], stream), "hipEventRecord");
			used[next] = true;
			next = (next + 1) % kTables;
		}
		long long Bytes() const { return (long long)kTables * capacity * (long long)sizeof(Entry); }
	};

	// the argument checks the stages' calls share: the texts are part of the interface (the tests match on them)
	inline std::string StreamId(int s) { return "stream " + std::to_string(s); }
	template <class Stage>
	Stage& RequireStage(const std::unique_ptr<Stage>& stage, const char* who)
	{
		if (!stage) throw std::runtime_error(std::string("neuralaudio_amd: ") + who + ": " + Stage::kNotEnabled);
		return *stage;
	}

	// the output stage of a batch (output_stage.h): the host mirror and the ring of entry tables
	struct GpuBatch::OutputStage
	{
		static constexpr const char* kNotEnabled = "output stage not enabled (NA_BatchEnableOutputStage)";
		OutputStageBook book;
		StageTables<OutStageEntry> tables{ "output stage: table in flight" };
	};
	hipError_t LaunchOutputStage(const OutStageLaunch& L, hipStream_t stream); // (output_stage_kernels.hip)

	// the cabinet stage of a batch (cabinet_stage.h): the host mirror, the rows' history rings, the IRs' taps (owned
	// through the book's ids) and the ring of entry tables
	struct GpuBatch::CabinetStage
	{
		static constexpr const char* kNotEnabled = "cabinet stage not enabled (NA_BatchEnableCabinetStage)";
		CabinetBook book;
		float* rings = nullptr;           // [ringRows][book.RingSamples()]
		int ringRows = 0;
		long long tapBytes = 0;           // device bytes of the loaded IRs
		StageTables<CabEntry> tables{ "cabinet stage: table in flight" };
		~CabinetStage();
	};
	hipError_t LaunchCabinetStage(const CabLaunch& L, hipStream_t stream); // (cabinet_stage_kernels.hip) the two launches of one piece

	// the gate stage of a batch (gate_stage.h): the host mirror, the rows' states and gain rows on the device, the ring of
	// entry tables, and -- between the detector and the apply launch of one call -- the table that call runs on
	struct GpuBatch::GateStage
	{
		static constexpr const char* kNotEnabled = "gate stage not enabled (NA_BatchEnableGateStage)";
		GateBook book;
		float* state = nullptr;           // [rowCapacity] GateState
		float* gains = nullptr;           // [rowCapacity][gainSamples]
		int rowCapacity = 0;
		int gainSamples = kGateMinGainSamples; // a power of two
		StageTables<GateEntry> tables{ "gate stage: table in flight" };
		const GateEntry* dev = nullptr;   // the device table the detector of this call read ...
		int count = 0;                    // ... and its entries; 0: the call has none
		~GateStage();
	};
	hipError_t LaunchGateDetect(const GateDetectLaunch& L, hipStream_t stream); // (gate_stage_kernels.hip)
	hipError_t LaunchGateApply(const GateApplyLaunch& L, hipStream_t stream);

	// the EQ stage of a batch (eq_stage.h): the host mirror, the rows' two slots of coefficients and section states on
	// the device, and the ring of tables -- entries, and behind them the coefficient sets of the set calls since the last call
	struct GpuBatch::EqStage
	{
		static constexpr const char* kNotEnabled = "eq stage not enabled (NA_BatchEnableEqStage)";
		EqBook book;
		float* coefs = nullptr;           // [rowCapacity][2] EqCoefSet
		float* state = nullptr;           // [rowCapacity][2][kEqMaxSections] EqSecState
		int rowCapacity = 0;
		StageTables<EqEntry> tables{ "eq stage: table in flight" };
		~EqStage();
	};
	hipError_t LaunchEqStage(const EqLaunch& L, hipStream_t stream); // (eq_stage_kernels.hip)

	bool HostDirect(); // (gpu_batch_host.cpp) the kernels read / write pinned host blocks themselves instead of the copy engines
}
